"""Host checks of the Newmark elastodynamics pieces: the NumPy reference of the vector mass (tests/newmark_reference.py) against properties it must
have, the Hermite weights, the ABI entries, and the refusals of the host mirror that need no device."""
import numpy as np
import pytest

import newmark_reference as nref
import tet_reference as tref

KINDS = ["hex8", "hex27", "tet4", "tet10"]


def _mesh(tb, kind):
    if kind.startswith("hex"):
        g = tb.generate_mesh(tb.Hexahedron, (3, 2, 2), (0.0, 0.0, 0.0), (1.0, 0.7, 0.5), perturb=0.2)
    else:
        g = tref.perturbed_renumbered_box(tb, (2, 2, 2), (0.0, 0.0, 0.0), (1.0, 0.8, 0.6))
    dh = tb.DofHandler(g, tb.LagrangeCollection(2 if kind in ("hex27", "tet10") else 1) ** 3)
    return g, dh, tb.allocate_matrix(dh)


def _volume_and_lumped(kind, g, dh, rho):
    """cell volumes and ∫ ρ Nᵢ dΩ per dof, by quadrature one order above the one the mass uses (hexahedra) / from the closed form (tetrahedra)"""
    lumped = np.zeros(dh.ndofs)
    vol = 0.0
    for cell in range(g.n_cells):
        X = g.xyz[g.conn[cell]]
        if kind.startswith("hex"):
            pts, wts = nref.hex_rule(3)
            for xi, w in zip(pts, wts):
                dO = np.linalg.det(X.T @ nref.hex8_dshape(xi)) * w
                vol += dO
                N = nref.hex8_shape(xi) if kind == "hex8" else nref.hex27_shape(xi)
                for c in range(3):
                    lumped[dh.cell_dofs[cell, c::3]] += rho * dO * N
        else:
            V = tref.volumes(g.xyz, g.conn[cell:cell + 1])[0]
            vol += V
            # ∫ λᵥ = V/4;  P2: ∫ λᵥ(2λᵥ − 1) = −V/20, ∫ 4λᵢλⱼ = V/5
            N = np.full(4, V / 4.0) if kind == "tet4" else np.concatenate([np.full(4, -V / 20.0), np.full(6, V / 5.0)])
            for c in range(3):
                lumped[dh.cell_dofs[cell, c::3]] += rho * N
    return vol, lumped


@pytest.mark.parametrize("kind", KINDS)
def test_reference_mass_sums_to_the_mass_and_lumps_per_component(tb, kind):
    g, dh, sp = _mesh(tb, kind)
    rho = 1.7
    nz = nref.assemble_vector_mass(kind, g.xyz, g.conn, dh.cell_dofs, sp.rowptr, sp.colidx, rho)
    vol, lumped = _volume_and_lumped(kind, g, dh, rho)
    assert abs(nz.sum() - 3.0 * rho * vol) <= 1e-12 * 3.0 * rho * vol
    scale = np.abs(lumped).max()
    for c in range(3):
        e = np.zeros(dh.ndofs)
        comp = np.unique(dh.cell_dofs[:, c::3])
        e[comp] = 1.0
        y = nref.csr_matvec(sp.rowptr, sp.colidx, nz, e)
        want = np.zeros(dh.ndofs)
        want[comp] = lumped[comp]
        assert np.abs(y - want).max() <= 1e-12 * scale, (kind, c)
    # entries that couple different components are exactly zero
    assert np.all(nz[~nref.same_component_mask(dh.cell_dofs, sp.rowptr, sp.colidx)] == 0.0)


def test_tetrahedron_mass_rule_is_exact_to_degree_four():
    from math import factorial
    pts, w = nref.tet_mass_rule(2)
    assert len(w) == 11 and abs(w.sum() - 1.0 / 6.0) < 1e-16
    for d in range(5):
        for i in range(d + 1):
            for j in range(d + 1 - i):
                k = d - i - j
                exact = factorial(i) * factorial(j) * factorial(k) / factorial(i + j + k + 3)
                assert abs((w * pts[:, 1] ** i * pts[:, 2] ** j * pts[:, 3] ** k).sum() - exact) <= 1e-14 * exact


def test_hermite_weights_reproduce_the_end_points_and_differentiate():
    dt = 0.37
    for D, at0, at1 in ((0, (1, 0, 0, 0), (0, 0, 1, 0)), (1, (0, 1, 0, 0), (0, 0, 0, 1))):
        assert nref.hermite_weights(0.0, dt, D) == at0
        assert nref.hermite_weights(1.0, dt, D) == at1
    rng = np.random.default_rng(3)
    u0, v0, u1, v1 = rng.standard_normal((4, 5))
    assert np.array_equal(nref.hermite(0.0, dt, 0, u0, v0, u1, v1), u0) and np.array_equal(nref.hermite(1.0, dt, 0, u0, v0, u1, v1), u1)
    assert np.array_equal(nref.hermite(0.0, dt, 1, u0, v0, u1, v1), v0) and np.array_equal(nref.hermite(1.0, dt, 1, u0, v0, u1, v1), v1)
    h = 1e-6                                                    # in t; θ moves by h/Δt
    for theta in (0.0, 0.3, 0.5, 0.81, 1.0):
        for D in (0, 1):
            num = (np.array(nref.hermite_weights(theta + h / dt, dt, D)) - np.array(nref.hermite_weights(theta - h / dt, dt, D))) / (2 * h)
            want = np.array(nref.hermite_weights(theta, dt, D + 1))
            assert np.abs(num - want).max() <= 1e-8 * max(1.0, np.abs(want).max()), (theta, D)


def test_predictor_and_corrector_are_inverse_on_a_constant_acceleration():
    """with aₙ₊₁ = aₙ the corrected (u, v) are the exact constant-acceleration motion for any β, γ"""
    rng = np.random.default_rng(4)
    u, v, a = rng.standard_normal((3, 7))
    for beta, gamma in ((0.25, 0.5), (0.36, 0.7)):
        dt = 0.2
        ut, vt = nref.predict(u, v, a, dt, beta, gamma)
        u1 = u + dt * v + 0.5 * dt * dt * a
        a1, v1 = nref.correct(u1, ut, vt, dt, beta, gamma)
        assert np.allclose(a1, a, rtol=1e-12, atol=1e-12) and np.allclose(v1, v + dt * a, rtol=1e-12, atol=1e-12)


def test_newmark_symbols_are_declared_and_exported(tb):
    from thunderbolt_jl_amd import _lib
    lib = tb.lib()
    for name, nargs in (("tb_newmark_predict", 10), ("tb_newmark_stage", 7), ("tb_newmark_correct", 10), ("tb_hermite_interpolate", 10)):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs
        assert getattr(lib, name).argtypes is not None
    assert lib.tb_abi_revision() == 10
    # argument checks that need no device
    assert lib.tb_newmark_stage(None, None, 1.0, None, None, None, None) == _lib.TB_ERR_BAD_ARG
    assert lib.tb_hermite_interpolate(None, 0, 0.5, 1.0, 0, None, None, None, None, None) == _lib.TB_ERR_BAD_ARG


def test_model_forms_and_refusals_without_a_device(tb):
    ms = tb.ConstantCoefficient(tb.OrthotropicMicrostructure([1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0]))
    mat = tb.PK1Model(tb.Guccione1991PassiveModel(), ms)
    m4 = tb.ElastodynamicsModel("d", "v", mat, tb.ConstantCoefficient(1e3))
    m5 = tb.ElastodynamicsModel("d", "v", mat, (tb.RobinBC(1e8, "right"),), tb.ConstantCoefficient(1e3))
    assert m4.facet_models == () and len(m5.facet_models) == 1 and m5.quasi_static().facet_models == m5.facet_models
    s = tb.NewmarkSolver()
    assert (s.beta, s.gamma) == (0.25, 0.5)
    g = tb.generate_mesh(tb.Hexahedron, (2, 1, 1), (0.0, 0.0, 0.0), (1.0, 0.2, 0.2))
    dh = tb.DofHandler(g, tb.LagrangeCollection(1) ** 3)
    sp = tb.allocate_matrix(dh)
    with pytest.raises(NotImplementedError, match="adaptive"):
        tb.NewmarkIntegrator(m4, dh, sp, None, None, dt=0.1, adaptive=True)
    with pytest.raises(ValueError, match="velocity"):
        tb.NewmarkIntegrator(m4, dh, sp, [tb.Dirichlet("v", [0, 1, 2])], None, dt=0.1)
    with pytest.raises(NotImplementedError):
        tb.NewmarkIntegrator(tb.ElastodynamicsModel("d", "v", tb.LinearMaxwellMaterial(), 1e3), dh, sp, None, None, dt=0.1)
    active = tb.ActiveStressModel(tb.Guccione1991PassiveModel(), tb.SimpleActiveStress(220e3),
                                  tb.CaDrivenInternalSarcomereModel(tb.RDQ20MFModel(), tb.ConstantCoefficient(1.0)), ms)
    with pytest.raises(NotImplementedError, match="internal"):
        tb.NewmarkIntegrator(tb.ElastodynamicsModel("d", "v", active, 1e3), dh, sp, None, None, dt=0.1)
