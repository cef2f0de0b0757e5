"""The host side of the p-level of the multigrid without a GPU: the Q2←Q1 prolongation from the two cell-dof tables, the transfer and the per-dof
and blocked Galerkin planners (tests/pmultigrid_planner_driver.cpp, a stand-alone program linked with tb_mg_planners.cpp and the host generators,
built plainly and with ASan + UBSan, checked against dense PᵀAP from numpy), and the refusals and ABI additions that need no device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pmultigrid_reference as pref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "thunderbolt.jl_amd", "csrc")
CASES = ["scalar", "vector", "vector_renumbered", "vector_clamped", "vector_x_only"]


def box(tb, nel, perturb=0.0):
    return tb.generate_mesh(tb.Hexahedron, nel, (0, 0, 0), (1, 1, 1), perturb=perturb)


def handlers(tb, grid, ncomp, renumber=False, seed=0):
    """the second-order and the first-order handler of one grid"""
    rng = np.random.default_rng(seed)
    out = []
    for order in (2, 1):
        dh = tb.DofHandler(grid, tb.LagrangeCollection(order, ncomp))
        if renumber:
            dh = tb.renumber_dofs(dh, rng.permutation(dh.ndofs).astype(np.int32))
        out.append(dh)
    return out


def component_of(dh):
    comp = np.empty(dh.ndofs, dtype=np.int64)
    nc = dh.ip.ncomp
    for k in range(nc):
        comp[dh.cell_dofs[:, k::nc].ravel()] = k
    return comp


# ------------------------------------------------------------------------------------------------ the prolongation
def test_p_prolongation_interpolates_the_dof_coordinates(tb):
    g = box(tb, (2, 2, 2), perturb=0.2)
    dhf, dhc = handlers(tb, g, 1)
    P, _ = pref.dense_p_level(tb, dhf, dhc)
    assert set(np.unique(P[P != 0]).tolist()) <= {1.0, 0.5, 0.25, 0.125}
    assert sorted(set((P != 0).sum(axis=1).tolist())) == [1, 2, 4, 8] and (P != 0).sum(axis=0).max() <= 27
    err = np.abs(P @ tb.dof_coordinates(dhc) - tb.dof_coordinates(dhf)).max()
    print("max |P x_Q1 - x_Q2| = %.3e" % err)
    assert err <= 1e-15


# ------------------------------------------------------------------------------------------------ planners
def build_driver(exe, extra=()):
    """starts the compiler; the caller waits"""
    return subprocess.Popen(["g++", "-O2", "-std=c++17", "-fopenmp", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
                           "-I", CSRC, *extra, os.path.join(ROOT, "tests", "pmultigrid_planner_driver.cpp"), os.path.join(CSRC, "tb_mg_planners.cpp"),
                           os.path.join(CSRC, "tb_hostgen.cpp"), "-o", exe])


@pytest.fixture(scope="module")
def planner(tb, tmp_path_factory):
    d = str(tmp_path_factory.mktemp("pmgplanners"))
    g = box(tb, (3, 2, 2), perturb=0.2)
    want = {}
    for k, name in enumerate(CASES):
        ncomp = 1 if name == "scalar" else 3
        dhf, dhc = handlers(tb, g, ncomp, renumber=name == "vector_renumbered", seed=100 + k)
        sp = tb.allocate_matrix(dhf)
        A = np.random.default_rng(7 + k).uniform(-1.0, 1.0, sp.nnz)
        presc = None
        if name in ("vector_clamped", "vector_x_only"):
            on_face = tb.dof_coordinates(dhf)[:, 0] == 0.0
            presc = (on_face if name == "vector_clamped" else on_face & (component_of(dhf) == 0)).astype(np.uint8)
            assert presc.any()
        base = os.path.join(d, name)
        with open(base + ".meta", "w") as f:
            f.write("%d %d %d %d %d %d\n" % (g.n_nodes, g.n_cells, dhf.ndofs, dhc.ndofs, ncomp, 0 if presc is None else 1))
        for ext, a, dt in ((".conn", g.conn, "<i4"), (".fdofs", dhf.cell_dofs, "<i4"), (".cdofs", dhc.cell_dofs, "<i4"), (".A", A, "<f8")):
            np.ascontiguousarray(a, dtype=dt).tofile(base + ext)
        if presc is not None:
            presc.tofile(base + ".presc")
        P, cpre = pref.dense_p_level(tb, dhf, dhc, presc)
        want[name] = (P, pref.dense_to_csr(tb.allocate_matrix(dhc), pref.galerkin(P, pref.csr_to_dense(sp, A), cpre)))
    exe, exe_san = os.path.join(d, "pmg_driver"), os.path.join(d, "pmg_driver_san")
    builds = [build_driver(exe), build_driver(exe_san, ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"))]   # side by side
    assert [b.wait() for b in builds] == [0, 0]
    return d, exe, exe_san, want


def run_driver(exe, d, case, threads, *more):
    r = subprocess.run([exe, d, case, *more], capture_output=True, text=True, timeout=300, env=dict(os.environ, OMP_NUM_THREADS=str(threads)))
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])     # the driver's own invariant checks
    return r.stdout


def parse(out):
    lines = out.splitlines()
    head = lines[0].split()
    info = {head[k]: int(head[k + 1]) for k in range(0, len(head), 2)}
    np_ = info["p_entries"]
    trip = np.array([[int(v) for v in l.split()] for l in lines[1:1 + np_]]).reshape(-1, 3)
    return info, trip, np.array([float(v) for v in lines[1 + np_:]])


@pytest.mark.parametrize("case", CASES)
def test_p_transfer_and_galerkin_plan_give_the_dense_product(planner, case):
    d, exe, exe_san, want = planner
    out1, out4 = run_driver(exe, d, case, 1), run_driver(exe, d, case, 4)
    assert out1 == out4                                               # one recorded order, whatever the team size
    info, trip, got = parse(out1)
    P, w = want[case]
    Pd = np.zeros_like(P)
    Pd[trip[:, 0], trip[:, 1]] = 0.5 ** trip[:, 2]
    assert np.array_equal(Pd, P)                                      # powers of two: exact
    err = np.abs(got - w).max() / np.abs(w).max()
    print("%s: %s; max |A_c - PtAP| / max |PtAP| = %.3e" % (case, out1.splitlines()[0], err))
    assert got.shape == w.shape and err <= 1e-14
    assert info["terms"] > 0
    assert info["blocked"] == (1 if case in ("vector", "vector_clamped", "vector_x_only") else 0)
    if case == "vector":
        assert 9 * info["terms"] == info["dof_terms"]                 # one term per node pair
    if info["blocked"]:                                               # the per-dof plan of the same system gives the same product
        _, _, dof = parse(run_driver(exe, d, case, 4, "dof"))
        assert np.abs(dof - w).max() / np.abs(w).max() <= 1e-14
    assert run_driver(exe_san, d, case, 4) == out1                    # ASan + UBSan: clean, and the same digits


def test_a_blocked_plan_does_not_let_a_dropped_non_finite_value_in(planner, tb):
    """the x-only face: the entries of the prescribed rows and columns are not read into the sums, whatever they hold"""
    d, exe, _, want = planner
    base = os.path.join(d, "vector_x_only")
    A = np.fromfile(base + ".A")
    presc = np.fromfile(base + ".presc", dtype=np.uint8).astype(bool)
    dhf, _ = handlers(tb, box(tb, (3, 2, 2), perturb=0.2), 3)
    sp = tb.allocate_matrix(dhf)
    rows = np.repeat(np.arange(dhf.ndofs), np.diff(sp.rowptr))
    A2 = A.copy()
    A2[presc[rows] | presc[sp.colidx]] = np.nan
    for ext in (".meta", ".conn", ".fdofs", ".cdofs", ".presc"):
        with open(base + ext, "rb") as src, open(os.path.join(d, "vector_nan" + ext), "wb") as dst:
            dst.write(src.read())
    A2.tofile(os.path.join(d, "vector_nan.A"))
    info, _, got = parse(run_driver(exe, d, "vector_nan", 4))
    assert info["blocked"] == 1 and np.array_equal(got, parse(run_driver(exe, d, "vector_x_only", 4))[2])


# ------------------------------------------------------------------------------------------------ refusals and ABI without a device
def test_refusals(tb):
    g = box(tb, (2, 2, 2))
    gh = tb.GridHierarchy(g, 1)
    for misuse in (tb.PMGPrecon, tb.ChainedMGPrecon):                 # the signatures of before p-levels existed
        with pytest.raises(NotImplementedError, match="p-levels"):
            misuse(gh)
    q2, q1 = tb.DofHandler(gh.grids[-1], tb.LagrangeCollection(2)), tb.DofHandler(gh.grids[-1])
    pmg = tb.PMGPrecon()
    pmg.check(q2)
    with pytest.raises(NotImplementedError, match="order"):
        pmg.check(q1)
    with pytest.raises(NotImplementedError, match="hexahedral"):
        pmg.check(tb.DofHandler(tb.generate_mesh(tb.Tetrahedron, (2, 2, 2), (0, 0, 0), (1, 1, 1)), tb.LagrangeCollection(2) ** 3))
    chained = tb.ChainedMGPrecon(tb.PMGPrecon(), tb.GMGPrecon(gh))
    chained.check(q2)
    with pytest.raises(NotImplementedError, match="order"):
        chained.check(q1)
    with pytest.raises(ValueError, match="finest grid"):
        chained.check(tb.DofHandler(g, tb.LagrangeCollection(2)))      # the coarse grid is not the finest of the hierarchy
    with pytest.raises(ValueError, match="degree"):
        tb.ChainedMGPrecon(tb.PMGPrecon(degree=3), tb.GMGPrecon(gh, degree=2))
    with pytest.raises(ValueError, match="interval_ratio"):
        tb.ChainedMGPrecon(tb.PMGPrecon(interval_ratio=8.0), tb.GMGPrecon(gh))
    with pytest.raises(TypeError):
        tb.ChainedMGPrecon(tb.GMGPrecon(gh), tb.PMGPrecon())
    with pytest.raises(NotImplementedError, match="V-cycles"):
        tb.PMGPrecon(cycle="W")
    with pytest.raises(NotImplementedError, match="Chebyshev"):
        tb.PMGPrecon(smoother="gauss-seidel")
    with pytest.raises(NotImplementedError, match="ChainedMGPrecon"):  # GMGPrecon alone keeps refusing second-order fields and says what serves them
        tb.GMGPrecon(gh).check(q2)
    assert tb.KrylovMGSolver("cg", chained).mg is chained and tb.KrylovMGSolver("cg", pmg).mg is pmg
    with pytest.raises(NotImplementedError, match="GMRES"):
        tb.KrylovMGSolver("gmres", chained)


def test_abi_additions(tb):
    L = tb._lib
    lib = tb.lib()
    assert lib.tb_abi_revision() == 10
    for name in ("tb_mg_set_p_transfer", "tb_mg_level_plan", "tb_mg_galerkin"):
        assert name in L.SIGNATURES and hasattr(lib, name), name
    blocked, terms = C.c_int(), C.c_int64()
    calls = [lib.tb_mg_set_p_transfer(None, 1), lib.tb_mg_level_plan(None, 1, C.byref(blocked), C.byref(terms)), lib.tb_mg_galerkin(None, 1)]
    assert calls == [L.TB_ERR_BAD_ARG] * 3, calls
    assert b"NULL" in lib.tb_last_error_string()
