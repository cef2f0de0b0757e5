"""The host side of the geometric multigrid without a GPU: the grid hierarchy (nested nodes, parent lists, transferred sets), the transfer and
Galerkin planners (tests/multigrid_planner_driver.cpp, a stand-alone program linked with tb_mg_planners.cpp and the host generators, built plainly
and with ASan + UBSan, checked against dense PᵀAP from numpy), and the refusals and ABI additions that need no device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import multigrid_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "thunderbolt.jl_amd", "csrc")
MG_SYMBOLS = ["tb_mg_create", "tb_mg_set_level", "tb_mg_set_transfer", "tb_mg_set_prescribed", "tb_mg_setup", "tb_mg_apply", "tb_mg_level_matrix",
              "tb_mg_level_lambda_max", "tb_mg_prolong", "tb_mg_restrict", "tb_mg_destroy", "tb_pcg_solve_mg"]


def box(tb, nel, perturb=0.0):
    return tb.generate_mesh(tb.Hexahedron, nel, (0, 0, 0), (1, 1, 1), perturb=perturb)


# ------------------------------------------------------------------------------------------------ hierarchy
@pytest.fixture(scope="module")
def gh2(tb):
    return tb.GridHierarchy(box(tb, (2, 2, 2), perturb=0.2), 2)


def test_coarse_nodes_are_a_prefix_and_parents_interpolate_the_coordinates(tb, gh2):
    assert [g.n_cells for g in gh2.grids] == [8, 64, 512]
    for r in range(2):
        gc, gf = gh2.grids[r], gh2.grids[r + 1]
        assert np.array_equal(gf.xyz[:gc.n_nodes], gc.xyz)
        pptr, pidx = gh2.parents[r]
        counts = np.diff(pptr)
        assert set(counts.tolist()) == {1, 2, 4, 8} and np.array_equal(pidx[pptr[:gc.n_nodes]], np.arange(gc.n_nodes))
        P = ref.nodal_P(gh2.parents[r], gc.n_nodes)
        assert set(np.unique(P[P != 0]).tolist()) <= {1.0, 0.5, 0.25, 0.125}
        err = np.abs(P @ gc.xyz - gf.xyz).max()
        print("refinement %d: max |P xyz_c - xyz_f| = %.3e" % (r, err))
        assert err <= 1e-15


def _reference_coordinates(X, x):
    """ξ with Σ N_a(ξ) X_a = x for one trilinear hexahedron (Newton from the centre)"""
    s = np.array([(-1, -1, -1), (1, -1, -1), (1, 1, -1), (-1, 1, -1), (-1, -1, 1), (1, -1, 1), (1, 1, 1), (-1, 1, 1)], dtype=float)
    xi = np.zeros(3)
    for _ in range(30):
        N = 0.125 * np.prod(1 + s * xi, axis=1)
        dN = np.stack([0.125 * s[:, d] * np.prod(np.delete(1 + s * xi, d, axis=1), axis=1) for d in range(3)], axis=1)   # (8, 3)
        res = N @ X - x
        if np.abs(res).max() < 1e-14:
            break
        xi = xi - np.linalg.solve((X.T @ dN), res)
    return xi


def test_every_child_lies_in_its_parent(tb, gh2):
    for r in range(2):
        gc, gf = gh2.grids[r], gh2.grids[r + 1]
        f2c = gh2.fine2coarse[r]
        assert f2c.shape == (gf.n_cells,)
        cent = gf.xyz[gf.conn].mean(axis=1)
        for c in range(gf.n_cells):
            xi = _reference_coordinates(gc.xyz[gc.conn[f2c[c]]], cent[c])
            assert np.abs(xi).max() <= 1 + 1e-10, (r, c, xi)


def test_facet_sets_follow_the_refinement(tb):
    g = box(tb, (3, 2, 2))
    gh = tb.GridHierarchy(g, 2)
    fine = gh.grids[-1]
    geo = tb.Grid(tb.Hexahedron, fine.xyz, fine.conn)
    preds = {"left": lambda x: x[0] == 0.0, "right": lambda x: x[0] == 1.0, "front": lambda x: x[1] == 0.0, "back": lambda x: x[1] == 1.0,
             "bottom": lambda x: x[2] == 0.0, "top": lambda x: x[2] == 1.0}
    for name, pred in preds.items():
        want = {tuple(p) for p in geo.addfacetset(name, pred).tolist()}
        got = {tuple(p) for p in fine.facetset(name).tolist()}
        assert len(got) == len(fine.facetset(name)) and got == want, name
        assert len(got) == 16 * len(g.facetset(name))


def test_cell_and_node_sets_follow_the_refinement(tb):
    g = box(tb, (4, 2, 2))
    g.addcellset("soft", lambda x: x[0] <= 0.5)
    g.addcellset("stiff", lambda x: x[0] >= 0.5)
    g.nodesets = {"leftnodes": np.flatnonzero(g.xyz[:, 0] == 0.0), "corner": np.array([0])}
    fine = tb.GridHierarchy(g, 1).grids[1]
    cent = fine.xyz[fine.conn].mean(axis=1)
    assert np.array_equal(np.sort(fine.getcellset("soft")), np.flatnonzero(cent[:, 0] < 0.5))
    assert np.array_equal(np.sort(fine.getcellset("stiff")), np.flatnonzero(cent[:, 0] > 0.5))
    assert np.array_equal(np.sort(fine.getnodeset("leftnodes")), np.flatnonzero(fine.xyz[:, 0] == 0.0))
    assert fine.getnodeset("corner").tolist() == [0]


def test_uniform_refinement_keeps_its_return_value(tb):
    g = box(tb, (2, 1, 1), perturb=0.1)
    a, (b, _, _) = tb.uniform_refinement(g), tb.uniform_refinement_with_maps(g)
    assert isinstance(a, tb.Grid) and np.array_equal(a.conn, b.conn) and np.array_equal(a.xyz, b.xyz)


# ------------------------------------------------------------------------------------------------ planners
def build_driver(exe, extra=()):
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fopenmp", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
                           "-I", CSRC, *extra, os.path.join(ROOT, "tests", "multigrid_planner_driver.cpp"), os.path.join(CSRC, "tb_mg_planners.cpp"),
                           os.path.join(CSRC, "tb_hostgen.cpp"), "-o", exe])


def planner_cases(tb):
    """name → (grid hierarchy, ncomp, renumber, prescribed-face predicate or None)"""
    return {"box_scalar": (tb.GridHierarchy(box(tb, (2, 2, 2), perturb=0.2), 1), 1, False, None),
            "box_vector_renumbered": (tb.GridHierarchy(box(tb, (3, 2, 1), perturb=0.2), 1), 3, True, None),
            "box_vector_prescribed": (tb.GridHierarchy(box(tb, (3, 2, 1), perturb=0.2), 1), 3, True, "face"),
            "ring": (tb.GridHierarchy(tb.generate_ring_mesh(8, 1, 2), 1), 1, False, None),
            "ideal_lv": (tb.GridHierarchy(tb.generate_ideal_lv_mesh_hex(4, 1, 1), 1), 3, False, None)}


def level_handlers(tb, gh, ncomp, renumber, seed):
    rng = np.random.default_rng(seed)
    dhs = []
    for g in gh.grids:
        dh = tb.DofHandler(g, tb.LagrangeCollection(1, ncomp))
        if renumber:
            dh = tb.renumber_dofs(dh, rng.permutation(dh.ndofs).astype(np.int32))
        dhs.append(dh)
    return dhs


@pytest.fixture(scope="module")
def planner(tb, tmp_path_factory):
    d = str(tmp_path_factory.mktemp("mgplanners"))
    want = {}
    for k, (name, (gh, ncomp, renumber, face)) in enumerate(planner_cases(tb).items()):
        dhc, dhf = level_handlers(tb, gh, ncomp, renumber, 100 + k)
        sp = tb.allocate_matrix(dhf)
        rng = np.random.default_rng(7 + k)
        A = rng.uniform(-1.0, 1.0, sp.nnz)
        presc = None
        if face:
            presc = np.zeros(dhf.ndofs, dtype=np.uint8)
            presc[ref.node_dofs(dhf)[gh.grids[1].xyz[:, 0] == 0.0].ravel()] = 1
        base = os.path.join(d, name)
        with open(base + ".meta", "w") as f:
            f.write("%d %d %d %d %d %d %d %d\n" % (gh.grids[1].n_nodes, gh.grids[1].n_cells, dhf.ndofs, gh.grids[0].n_nodes, gh.grids[0].n_cells, dhc.ndofs, ncomp,
                                                    0 if presc is None else 1))
        for ext, a, dt in ((".fconn", gh.grids[1].conn, "<i4"), (".fdofs", dhf.cell_dofs, "<i4"), (".cconn", gh.grids[0].conn, "<i4"), (".cdofs", dhc.cell_dofs, "<i4"),
                           (".pptr", gh.parents[0][0], "<i8"), (".pidx", gh.parents[0][1], "<i4"), (".A", A, "<f8")):
            np.ascontiguousarray(a, dtype=dt).tofile(base + ext)
        if presc is not None:
            presc.tofile(base + ".presc")
        P, cpre = ref.dense_P(gh.parents[0], dhf, dhc, presc)
        want[name] = ref.dense_to_csr(tb.allocate_matrix(dhc), ref.galerkin(P, ref.csr_to_dense(sp, A), cpre))
    exe, exe_san = os.path.join(d, "mg_driver"), os.path.join(d, "mg_driver_san")
    build_driver(exe)
    build_driver(exe_san, ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"))
    return d, exe, exe_san, want


def run_driver(exe, d, case, threads):
    r = subprocess.run([exe, d, case], capture_output=True, text=True, timeout=300, env=dict(os.environ, OMP_NUM_THREADS=str(threads)))
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])     # the driver's own invariant checks
    return r.stdout


@pytest.mark.parametrize("case", ["box_scalar", "box_vector_renumbered", "box_vector_prescribed", "ring", "ideal_lv"])
def test_galerkin_plan_gives_the_dense_product(planner, case):
    d, exe, exe_san, want = planner
    out1, out4 = run_driver(exe, d, case, 1), run_driver(exe, d, case, 4)
    assert out1 == out4                                               # one recorded order, whatever the team size
    lines = out1.splitlines()
    got = np.array([float(v) for v in lines[1:]])
    w = want[case]
    err = np.abs(got - w).max() / np.abs(w).max()
    print("%s: %s; max |A_c - PtAP| / max |PtAP| = %.3e" % (case, lines[0], err))
    assert got.shape == w.shape and err <= 1e-14
    assert run_driver(exe_san, d, case, 4) == out1                    # ASan + UBSan: clean, and the same digits


def test_the_multigrid_planners_need_no_hip_header(tmp_path):
    subprocess.check_call(["g++", "-std=c++17", "-fopenmp", "-Wall", "-Werror", "-c", os.path.join(CSRC, "tb_mg_planners.cpp"), "-o", str(tmp_path / "tb_mg_planners.o")])


# ------------------------------------------------------------------------------------------------ refusals and ABI without a device
def test_refusals(tb):
    g = box(tb, (2, 2, 2))
    gh = tb.GridHierarchy(g, 1)
    tets = tb.generate_mesh(tb.Tetrahedron, (2, 2, 2), (0, 0, 0), (1, 1, 1))
    with pytest.raises(NotImplementedError, match="hexahedral"):
        tb.GridHierarchy(tets, 1)
    mg = tb.GMGPrecon(gh)
    mg.check(tb.DofHandler(gh.grids[-1]))                                                  # the supported case passes
    with pytest.raises(NotImplementedError, match="hexahedral"):
        mg.check(tb.DofHandler(tets))
    with pytest.raises(NotImplementedError, match="first-order"):
        mg.check(tb.DofHandler(gh.grids[-1], tb.LagrangeCollection(2)))
    with pytest.raises(ValueError, match="finest grid"):
        mg.check(tb.DofHandler(g))                                                         # the coarse grid is not the finest of the hierarchy
    with pytest.raises(NotImplementedError, match="GMRES"):
        tb.KrylovMGSolver("gmres", mg)
    for refused in (tb.PMGPrecon, tb.ChainedMGPrecon):
        with pytest.raises(NotImplementedError, match="p-levels"):
            refused(gh)
    with pytest.raises(NotImplementedError, match="V-cycles"):
        tb.GMGPrecon(gh, cycle="W")
    assert tb.KrylovMGSolver("cg", mg).mg is mg


def test_abi_additions(tb):
    L = tb._lib
    lib = tb.lib()
    assert lib.tb_abi_revision() == 10
    for name in MG_SYMBOLS:
        assert name in L.SIGNATURES and hasattr(lib, name), name
    h, p, v = C.c_void_p(), C.c_void_p(), C.c_double()
    it = C.c_int()
    ptr = np.zeros(2, dtype=np.int64).ctypes.data_as(L.c_i64p)
    idx = np.zeros(1, dtype=np.int32).ctypes.data_as(L.c_i32p)
    calls = [lib.tb_mg_create(None, 2, C.byref(h)), lib.tb_mg_set_level(None, 0, None), lib.tb_mg_set_transfer(None, 1, 1, ptr, idx),
             lib.tb_mg_set_prescribed(None, None), lib.tb_mg_setup(None, None, 2, 4.0), lib.tb_mg_apply(None, None, None),
             lib.tb_mg_level_matrix(None, 0, C.byref(p)), lib.tb_mg_level_lambda_max(None, 1, C.byref(v)), lib.tb_mg_prolong(None, 1, None, None),
             lib.tb_mg_restrict(None, 1, None, None), lib.tb_pcg_solve_mg(None, None, None, None, 1e-8, 0.0, 10, None, C.byref(it), C.byref(v))]
    assert calls == [L.TB_ERR_BAD_ARG] * len(calls), calls
    assert b"NULL" in lib.tb_last_error_string()
    assert lib.tb_mg_destroy(None) == L.TB_OK
