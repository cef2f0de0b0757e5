"""Device point location and nodal inter-grid interpolation (tb_locator_*, thunderbolt.jl_amd/transfer.py) against the NumPy brute-force reference of
tests/transfer_reference.py.  Tolerances: 1e-12 relative to max |u| is the project's parity tolerance; a linear field is reproduced at 1e-13 and a
transfer between matching grids at 1e-14 (the located ξ of a vertex is ±1 to a few ulp, so N is 1 and 0 to a few ulp)."""
import ctypes as C
import json
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest

import transfer_reference as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-10


def linear(x):
    return 0.3 * x[:, 0] - 1.1 * x[:, 1] + 0.7 * x[:, 2] + 0.25


def collection(tb, order, ncomp):
    return tb.LagrangeCollection(order) ** ncomp if ncomp > 1 else tb.LagrangeCollection(order)


@pytest.fixture(scope="module")
def hexes(tb):
    return tb.generate_mesh(tb.Hexahedron, (5, 4, 3), (0, 0, 0), (1, 1, 1), perturb=0.2)


@pytest.fixture(scope="module")
def tets(tb):
    return tb.generate_mesh(tb.Tetrahedron, (3, 3, 2), (0.1, 0.1, 0.1), (0.9, 0.9, 0.9))


def run_transfer(tb, device, dh_from, dh_to, u_from, subdomains_to=None, fill=777.0, expect_missing=False):
    """device transfer and the reference's, both into vectors pre-filled with `fill`"""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore" if expect_missing else "error")
        op = tb.NodalIntergridInterpolation(device, dh_from, dh_to, subdomains_to)
    u_to = device.to_device(np.full(dh_to.ndofs, fill))
    tb.transfer(u_to, op, device.to_device(u_from))
    cells_to = None if subdomains_to is None else (dh_to.grid.getcellset(subdomains_to) if isinstance(subdomains_to, str) else subdomains_to)
    ref, ref_cells = R.transfer(np.full(dh_to.ndofs, fill), dh_from, dh_to, u_from, tb.dof_coordinates(dh_to), cells_to, TOL)
    return op, u_to.to_host(), ref, ref_cells


def check_against_reference(tb, device, dh_from, dh_to):
    rng = np.random.default_rng(7)
    u = rng.uniform(-1.0, 1.0, dh_from.ndofs)
    op, got, ref, _ = run_transfer(tb, device, dh_from, dh_to, u)
    assert op.n_missing == 0 and not np.isnan(ref).any()
    err = np.abs(got - ref).max() / np.abs(u).max()
    print("random nodal data: max error relative to max|u| %.3e" % err)
    assert err <= 1e-12
    ulin = linear(tb.dof_coordinates(dh_from))
    _, got, _, _ = run_transfer(tb, device, dh_from, dh_to, ulin)
    err = np.abs(got - linear(tb.dof_coordinates(dh_to))).max()
    print("linear field: max error %.3e" % err)
    assert err <= 1e-13


# ---- 1. perturbed hexahedra → tetrahedra, and back
@pytest.mark.parametrize("order,ncomp", [(1, 1), (2, 1), (1, 3), (2, 3)])
def test_hex_fields_to_tetrahedra(tb, device, hexes, tets, order, ncomp):
    check_against_reference(tb, device, tb.DofHandler(hexes, collection(tb, order, ncomp)), tb.DofHandler(tets, collection(tb, 1, ncomp)))


@pytest.mark.parametrize("order,ncomp", [(1, 1), (1, 3), (2, 3)])
def test_tet_fields_to_hexahedra(tb, device, order, ncomp):
    # source and target swapped: the tetrahedra now cover the unit cube and the perturbed hexahedra lie strictly inside
    src = tb.generate_mesh(tb.Tetrahedron, (3, 3, 2), (0, 0, 0), (1, 1, 1))
    dst = tb.generate_mesh(tb.Hexahedron, (5, 4, 3), (0.1, 0.1, 0.1), (0.9, 0.9, 0.9), perturb=0.2)
    check_against_reference(tb, device, tb.DofHandler(src, collection(tb, order, ncomp)), tb.DofHandler(dst, collection(tb, 1, ncomp)))


# ---- 2. cell ids and round trip
@pytest.mark.parametrize("n", [257, 1, 63, 65, 0])
def test_cell_ids_and_round_trip(tb, device, hexes, n):
    pts = np.random.default_rng(0).uniform(0.1, 0.9, (257, 3))[:n]
    ref_cells, ref_xi = R.locate(hexes, pts, TOL)
    # seed 0 keeps every point at least 1e-6 (reference coordinates) from a cell face, where rounding could not change the answer (checked here on the host)
    assert (ref_cells >= 0).all() and (n == 0 or R.face_distance(hexes.cell_kind, ref_xi).min() > 1e-6)
    ph = tb.PointEvalHandler(device, hexes, pts, TOL)
    assert ph.n_points == n and ph.n_missing == 0
    cells, xi = ph.cells, ph.xi
    assert cells.dtype == np.int32 and (cells == ref_cells).all()
    if n:
        diag = np.linalg.norm(hexes.xyz.max(axis=0) - hexes.xyz.min(axis=0))
        assert np.linalg.norm(R.position(hexes, cells, xi) - pts, axis=1).max() <= 1e-12 * diag
        assert (np.abs(xi) <= 1.0 + TOL).all()


def test_single_cell_source(tb, device):
    one = tb.generate_mesh(tb.Hexahedron, (1, 1, 1), (0, 0, 0), (1, 2, 3))
    pts = np.array([[0.5, 1.0, 1.5], [0.0, 0.0, 0.0], [1.0, 2.0, 3.0], [0.25, 1.9, 0.1], [1.5, 1.0, 1.0]])
    ph = tb.PointEvalHandler(device, one, pts, TOL)
    ref_cells, ref_xi = R.locate(one, pts, TOL)
    assert (ph.cells == ref_cells).all() and list(ref_cells) == [0, 0, 0, 0, -1] and ph.n_missing == 1
    assert np.abs(ph.xi[:4] - ref_xi[:4]).max() <= 1e-14


# ---- 3. matching grids: every point is a vertex shared by up to eight cells
def test_matching_grids(tb, device):
    g = tb.generate_mesh(tb.Hexahedron, (4, 3, 2), (0, 0, 0), (1, 1, 1))
    dh = tb.DofHandler(g)
    u = np.random.default_rng(3).uniform(-1.0, 1.0, dh.ndofs)
    op, got, ref, ref_cells = run_transfer(tb, device, dh, dh, u)
    assert op.n_missing == 0                                         # box-boundary points are found
    assert (op.ph.cells == ref_cells).all()                          # the lowest-numbered of the cells that share the vertex
    lowest = np.full(g.n_nodes, g.n_cells)
    np.minimum.at(lowest, dh.cell_dofs.ravel(), np.repeat(np.arange(g.n_cells), 8))
    assert (op.ph.cells == lowest[op.node_to_dof_map]).all()
    err = np.abs(got - u).max() / np.abs(u).max()
    print("matching grids: max error %.3e" % err)
    assert err <= 1e-14


# ---- 4. points outside the source
def test_points_outside(tb, device, hexes):
    tgt = tb.generate_mesh(tb.Tetrahedron, (4, 4, 3), (-0.2, -0.2, -0.2), (1.2, 1.2, 1.2))
    dh_from, dh_to = tb.DofHandler(hexes), tb.DofHandler(tgt)
    u = np.random.default_rng(4).uniform(-1.0, 1.0, dh_from.ndofs)
    op, got, ref, ref_cells = run_transfer(tb, device, dh_from, dh_to, u, expect_missing=True)
    assert (ref_cells < 0).any() and (ref_cells >= 0).any()
    assert op.n_missing == int((ref_cells < 0).sum()) and (op.ph.cells == ref_cells).all()
    assert (np.isnan(got) == np.isnan(ref)).all() and np.isnan(got[op.node_to_dof_map[ref_cells < 0]]).all()
    ok = ~np.isnan(ref)
    assert np.abs(got[ok] - ref[ok]).max() <= 1e-12 * np.abs(u).max()
    with pytest.warns(UserWarning, match="%d \\(out of %d\\) points not found" % (op.n_missing, len(op.nodes))):
        tb.NodalIntergridInterpolation(device, dh_from, dh_to)
    # half of the target's cells: only their dofs are written (test/test_transfer.jl:38-54), the rest keeps its 777
    half = np.arange(tgt.n_cells // 2, dtype=np.int32)
    tgt.addcellset("half", half)
    for sub in (half, "half"):
        op, got, ref, ref_cells = run_transfer(tb, device, dh_from, dh_to, u, subdomains_to=sub, expect_missing=True)
        touched = np.zeros(dh_to.ndofs, dtype=bool)
        touched[np.unique(dh_to.cell_dofs[half])] = True
        assert 0 < touched.sum() < dh_to.ndofs and (op.node_to_dof_map == np.flatnonzero(touched)).all()
        assert (got[~touched] == 777.0).all() and not (got[touched] == 777.0).any()
        assert (np.isnan(got) == np.isnan(ref)).all() and op.n_missing == int((ref_cells < 0).sum())
        ok = ~np.isnan(ref)
        assert np.abs(got[ok] - ref[ok]).max() <= 1e-12 * np.abs(u).max()


# ---- 5. thin curved wall: many empty bins, several cells per bin
def test_ring_coarse_nodes_coincide_with_fine_nodes(tb, device):
    fine, coarse = tb.generate_ring_mesh(16, 2, 4), tb.generate_ring_mesh(8, 1, 2)
    dh_from, dh_to = tb.DofHandler(fine), tb.DofHandler(coarse)
    X_to = tb.dof_coordinates(dh_to)
    ref_cells, _ = R.locate(fine, X_to, TOL)
    assert (ref_cells >= 0).all()                                    # established on the host before the device result is relied on
    u = np.random.default_rng(5).uniform(-1.0, 1.0, dh_from.ndofs)
    op, got, ref, _ = run_transfer(tb, device, dh_from, dh_to, u)
    assert op.n_missing == 0 and (op.ph.cells == ref_cells).all()
    # each coarse node is a fine node: its value is that node's
    X_from = tb.dof_coordinates(dh_from)
    d = np.linalg.norm(X_to[:, None, :] - X_from[None, :, :], axis=2)
    same = d.argmin(axis=1)
    assert d.min(axis=1).max() <= 1e-14
    err = np.abs(got - u[same]).max() / np.abs(u).max()
    print("ring: max error against the coinciding fine nodes %.3e" % err)
    assert err <= 1e-12
    assert np.abs(got - ref).max() <= 1e-12 * np.abs(u).max()


# ---- 6. two dimensions
def test_quadrilaterals(tb, device):
    src, dst = tb.generate_mesh(tb.Quadrilateral, (7, 5)), tb.generate_mesh(tb.Quadrilateral, (3, 2))
    check_against_reference(tb, device, tb.DofHandler(src), tb.DofHandler(dst))
    pts = np.random.default_rng(6).uniform(-0.95, 0.95, (100, 2))
    pts3 = np.hstack([pts, np.full((100, 1), 5.0)])                   # z is ignored on two-dimensional meshes
    ph = tb.PointEvalHandler(device, src, pts3, TOL)
    ref_cells, ref_xi = R.locate(src, np.hstack([pts, np.zeros((100, 1))]), TOL)
    assert R.face_distance(src.cell_kind, ref_xi).min() > 1e-6
    assert ph.n_missing == 0 and (ph.cells == ref_cells).all() and np.abs(ph.xi - ref_xi).max() <= 1e-13


# ---- 7. relocate, graph replay, reproducibility
def test_relocate_graph_and_bit_reproducibility(tb, device, hexes, tets):
    dh_from, dh_to = tb.DofHandler(hexes, tb.LagrangeCollection(2)), tb.DofHandler(tets)
    u = device.to_device(np.random.default_rng(8).uniform(-1.0, 1.0, dh_from.ndofs))
    pts = np.random.default_rng(9).uniform(0.1, 0.8, (130, 3))
    ph = tb.PointEvalHandler(device, hexes, pts, TOL)
    for shifted in (pts[:77] + 0.05, np.vstack([pts, pts + 0.07])):  # fewer points, then more than the locator was created with
        ph.relocate(shifted)
        fresh = tb.PointEvalHandler(device, hexes, shifted, TOL)
        assert ph.n_points == len(shifted) and ph.n_missing == fresh.n_missing == 0
        assert (ph.cells == fresh.cells).all() and (ph.xi == fresh.xi).all()
        a, b = tb.evaluate_at_points(ph, dh_from, u).to_host(), tb.evaluate_at_points(fresh, dh_from, u).to_host()
        assert (a == b).all()
    op = tb.NodalIntergridInterpolation(device, dh_from, dh_to)
    eager1, eager2, replay = (device.to_device(np.full(dh_to.ndofs, 777.0)) for _ in range(3))
    tb.transfer(eager1, op, u)
    tb.transfer(eager2, op, u)
    e1 = eager1.to_host()
    assert (e1 == eager2.to_host()).all() and not (e1 == 777.0).any()
    dpts, refused, h = device.to_device(pts.ravel()), [], C.c_void_p()

    def body():
        # create / relocate read the number of missing points back: refused inside a capture, which stays open and valid
        refused.append(tb.lib().tb_locator_relocate(ph.h, len(pts), dpts.ptr))
        refused.append(tb.lib().tb_locator_create(dh_from.device_mesh(device).h, len(pts), dpts.ptr, TOL, C.byref(h)))
        tb.transfer(replay, op, u)

    n_before = ph.n_points
    graph = device.capture(body)
    assert refused == [tb._lib.TB_ERR_BAD_ARG] * 2 and not h and ph.n_points == n_before
    assert graph.nodes == 1
    for _ in range(2):
        replay.copy_from_host(np.full(dh_to.ndofs, 777.0))
        graph.launch()
        assert (replay.to_host() == e1).all()
    graph.close()


def test_field_mesh_must_match_the_located_grid(tb, device, hexes, tets):
    ph = tb.PointEvalHandler(device, hexes, np.array([[0.5, 0.5, 0.5]]), TOL)
    dh = tb.DofHandler(tets)
    out = device.zeros(1)
    with pytest.raises(tb.TBError) as e:
        tb._lib.check(tb.lib().tb_locator_evaluate(ph.h, dh.device_mesh(device).h, device.zeros(dh.ndofs).ptr, out.ptr, None))
    assert e.value.code == tb._lib.TB_ERR_BAD_ARG


# ---- 8. the example
def test_example_runs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "intergrid_transfer.py"), "--n", "12", "--m", "5", "--steps", "3"],
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads(out.stdout.strip().splitlines()[-1])
    assert d["n_missing"] == 0 and d["transferred_range"][0] >= d["source_range"][0] - 1e-12 and d["transferred_range"][1] <= d["source_range"][1] + 1e-12
    assert d["locate_ms"] > 0 and d["transfer_ms"] > 0
