"""Pseudo-ECG, the parts that need no device: the host helpers of thunderbolt.jl_amd/ecg.py, the NumPy reference itself (tests/ecg_reference.py:
dipole limit; the identity "lead = Poisson difference" on the block set-up of the reference's test/integration/test_ecg.jl) and the places that
name the new entry points."""
import os

import numpy as np
import pytest

import ecg_reference as R
import transfer_reference as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("tb_ecg_create", "tb_ecg_destroy", "tb_ecg_npoints", "tb_ecg_fluxes_device", "tb_ecg_update", "tb_ecg_evaluate", "tb_ecg_leads", "tb_scrub_scale")


def block_setup(tb, kind):
    """test_ecg.jl: heart 6³ on [−1,1]³ with nodes mapped x → sign(x)·x², torso 16³ on [−2,2]³, heart = the torso cells with ‖x‖∞ ≤ 1"""
    heart = tb.generate_mesh(kind, (6, 6, 6))
    heart.xyz[:] = np.sign(heart.xyz) * heart.xyz ** 2
    torso = tb.generate_mesh(kind, (16, 16, 16), (-2, -2, -2), (2, 2, 2))
    torso.addcellset("heart", lambda x: np.abs(x).max() <= 1.0)
    return heart, torso


# ---- host helpers
def test_closest_vertex(tb):
    g = tb.generate_mesh(tb.Hexahedron, (4, 4, 4), (-2, -2, -2), (2, 2, 2))
    for x in ([0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [0.4, -1.1, 1.9], [5.0, 5.0, 5.0]):
        v = tb.get_closest_vertex(x, g)
        d = np.linalg.norm(g.xyz - np.asarray(x), axis=1)
        assert d[v] == d.min() and v == R.closest_vertex(x, g.xyz)
    assert (g.xyz[tb.get_closest_vertex([0.0, 0.0, 0.0], g)] == 0.0).all()
    # equally close vertices: the lowest id
    assert tb.get_closest_vertex([-1.5, -2.0, -2.0], g) == min(np.flatnonzero(np.isclose(np.linalg.norm(g.xyz - np.array([-1.5, -2.0, -2.0]), axis=1), 0.5)))


def test_lead_right_hand_sides(tb):
    rhs = tb.lead_right_hand_sides(10, [[3, 7], [0, 2, 4, 9]])
    assert rhs.shape == (2, 10)
    assert rhs[0, 3] == -1.0 and rhs[0, 7] == 1.0 and np.count_nonzero(rhs[0]) == 2
    assert rhs[1, 0] == -1.0 and (rhs[1, [2, 4, 9]] == 1.0 / 3.0).all() and np.count_nonzero(rhs[1]) == 4
    assert (rhs == R.lead_rhs(10, [[3, 7], [0, 2, 4, 9]])).all()
    with pytest.raises(ValueError):
        tb.lead_right_hand_sides(10, [[3]])


def test_heart_indicator_field_coefficient(tb):
    for kind in (tb.Hexahedron, tb.Tetrahedron):
        _, torso = block_setup(tb, kind)
        cells = torso.getcellset("heart")
        assert len(cells) == (512 if kind == tb.Hexahedron else 3072)
        for sub in ("heart", cells):
            c = tb.cellset_coefficient(torso, sub, inside=2.5, outside=0.0)
            assert isinstance(c, tb.FieldCoefficient) and c.data.shape == torso.conn.shape
            assert (c.data[cells] == 2.5).all() and c.data.sum() == 2.5 * len(cells) * torso.conn.shape[1]


def test_vertex_dofs(tb):
    g = tb.generate_mesh(tb.Tetrahedron, (2, 3, 2))
    dh = tb.DofHandler(g)
    n2d = tb.vertex_dofs(dh)
    assert sorted(n2d) == list(range(dh.ndofs)) and (n2d[g.conn] == dh.cell_dofs).all()
    assert np.abs(tb.dof_coordinates(dh)[n2d] - g.xyz).max() == 0.0


# ---- the NumPy reference against the dipole limit
@pytest.mark.parametrize("kind", ["hex", "tet"])
def test_reference_dipole_limit(tb, kind):
    """constant flux p in a 0.1-wide cube seen from distance 10: φ = −p·d̂ V / (4πκₜ d²) to 1e-3 (d̂ from the electrode to the cube)"""
    g = tb.generate_mesh(tb.Hexahedron if kind == "hex" else tb.Tetrahedron, (2, 2, 2), (-0.05, -0.05, -0.05), (0.05, 0.05, 0.05))
    xq, dO, _, _ = R.quadrature_geometry(g.xyz, g.conn)
    assert abs(dO.sum() - 1e-3) <= 1e-17
    p = np.array([0.3, -1.2, 0.7])
    flux = np.broadcast_to(p, xq.shape)
    kt = 1.7
    for e in ([10.0, 0.0, 0.0], [0.0, -10.0, 0.0], [6.0, 0.0, 8.0]):
        e = np.asarray(e)
        val, mag = R.plonsey(flux, xq, dO, e, kt)
        dhat = -e / np.linalg.norm(e)
        want = -(p @ dhat) * 1e-3 / (4.0 * np.pi * kt * 100.0)
        assert abs(val[0] - want) <= 1e-3 * abs(want) and mag[0] >= abs(val[0])


def test_reference_fluxes_of_a_linear_field(tb):
    g = tb.generate_mesh(tb.Hexahedron, (3, 4, 2), (0, 0, 0), (1, 1, 1), perturb=0.2)
    dh = tb.DofHandler(g)
    a = np.array([0.3, -1.1, 0.7])
    D = np.array([[2.0, 0.7, 0.1], [0.3, 1.5, -0.2], [0.35, -0.2, 1.0]])       # non-symmetric: D·∇φ, not ∇φ·D
    fl = R.fluxes(g.xyz, g.conn, dh.cell_dofs, tb.dof_coordinates(dh) @ a, D)
    assert np.abs(fl - D @ a).max() <= 1e-13 and np.abs(D @ a - a @ D).max() > 0.1


# ---- the identity lead = Poisson difference on the reference's block set-up
@pytest.mark.parametrize("kind", ["hex", "tet"])
def test_reference_block_identity(tb, kind):
    heart, torso = block_setup(tb, tb.Hexahedron if kind == "hex" else tb.Tetrahedron)
    hdh, tdh = tb.DofHandler(heart), tb.DofHandler(torso)
    phi = tb.dof_coordinates(hdh)[:, 0] ** 3
    el = np.array([[-2.0, 0, 0], [2.0, 0, 0], [0, -2.0, 0], [0, 2.0, 0], [0, 0, -2.0], [0, 0, 2.0]])
    # Plonsey on the heart
    xq, dO, _, _ = R.quadrature_geometry(heart.xyz, heart.conn)
    pl, _ = R.plonsey(R.fluxes(heart.xyz, heart.conn, hdh.cell_dofs, phi, 1.0), xq, dO, el)
    # the torso operators: κ = 1, κᵢ = 1 in the heart cells and 0 outside
    _, _, _, N = R.quadrature_geometry(torso.xyz, torso.conn)
    ki = np.einsum("qa,ca->cq", N, tb.cellset_coefficient(torso, "heart").data)[:, :, None, None] * np.eye(3)
    K = R.diffusion_matrix(torso.xyz, torso.conn, tdh.cell_dofs, tdh.ndofs, 1.0)
    Ki = R.diffusion_matrix(torso.xyz, torso.conn, tdh.cell_dofs, tdh.ndofs, ki)
    assert abs(Ki.sum()) <= 1e-12 and np.abs(Ki @ np.ones(tdh.ndofs)).max() <= 1e-13      # constants are in the kernel: the source sums to zero
    n2d = tb.vertex_dofs(tdh)
    ground = n2d[tb.get_closest_vertex([0.0, 0.0, 0.0], torso)]
    dofs, nodes = tb.intergrid_dofs(tdh, "heart")
    cells, xi = TR.locate(heart, nodes, 1e-10)
    assert (cells >= 0).all()
    phi_t = np.zeros(tdh.ndofs)
    phi_t[dofs] = TR.evaluate(hdh, phi, cells, xi)[:, 0]
    pe = R.poisson(K, Ki, phi_t, ground)
    ev = [n2d[tb.get_closest_vertex(e, torso)] for e in el]
    lam = -R.lead_fields(K, [[ev[0], ev[1]], [ev[2], ev[3]], [ev[4], ev[5]]], ground) @ (Ki @ phi_t)
    diff = np.array([pe[ev[1]] - pe[ev[0]], pe[ev[3]] - pe[ev[2]], pe[ev[5]] - pe[ev[4]]])
    print(kind, "Poisson differences", diff, "leads", lam, "Plonsey", pl)
    assert np.abs(lam - diff).max() <= 1e-14                     # the identity, to rounding (4e-16 computed on the hexahedra)
    assert pe[ground] == 0.0
    if kind == "hex":
        assert abs(diff[0] + 0.731061) <= 1e-6
        assert np.abs(diff[1:]).max() <= 1e-14                   # below 3e-16 computed
        assert abs(pl[1] - 0.161711) <= 1e-6 and abs(pl[0] + 0.161711) <= 1e-6
        assert np.abs(pl[2:]).max() <= 1e-15
    else:                                                        # the diagonal cut of the tetrahedra breaks the mirror symmetry slightly
        assert abs(diff[0] + 0.74) <= 1e-2 and np.abs(diff[1:]).max() <= 1e-4
        assert pl[1] > 0.04 and pl[0] < -0.04 and np.abs(pl[2:]).max() <= 1e-4


# ---- entry points
def test_entry_points_are_named_everywhere(tb):
    header = open(os.path.join(ROOT, "include", "tbhip.h"), encoding="utf-8").read()
    julia = open(os.path.join(ROOT, "julia", "ThunderboltHIPBackend.jl"), encoding="utf-8").read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md"), encoding="utf-8").read()
    for name in ENTRIES:
        assert name + "(" in header and name in tb._lib.SIGNATURES and ":" + name in julia, name
        assert hasattr(tb.lib(), name)
    assert "tb_ecg_*" in integration and "tb_scrub_scale" in integration
    for name in ("Plonsey1964ECGGaussCache", "PoissonECGReconstructionCache", "Geselowitz1989ECGLeadCache", "update_ecg", "evaluate_ecg", "get_closest_vertex",
                 "cellset_coefficient"):
        assert hasattr(tb, name), name
