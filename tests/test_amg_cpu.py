"""The algebraic multigrid without a GPU: the host planner (csrc/tb_amg_planners.cpp) through a stand-alone driver (tests/amg_planner_driver.cpp)
against the SciPy restatement of tests/amg_reference.py — aggregates, the patterns of P, R, A·P and A_c, the R permutation — the two properties of the
restatement the GPU tests lean on (level-independent iteration counts, no strength ties), and the refusals the Python layer decides on the host."""
import os
import subprocess

import numpy as np
import pytest

import amg_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "thunderbolt.jl_amd", "csrc")
THETA = 0.25


def face_x0(n_nodes):
    return np.flatnonzero(np.arange(n_nodes ** 3) % n_nodes == 0)


def tet_box(tb):
    g = tb.generate_mesh(tb.Tetrahedron, (4, 4, 4), (0, 0, 0), (1, 1, 1))
    return ref.p1_stiffness(np.asarray(g.xyz, dtype=np.float64), np.asarray(g.conn)), g


def three_components(K):
    """a 3-component system on the nodes of K, dofs 3v + c, the components coupled weakly → (A, labels)"""
    B = np.array([[1.0, 0.3, 0.1], [0.3, 1.5, 0.2], [0.1, 0.2, 2.0]])
    return ref.canonical(ref.sp.kron(K, B)), np.tile(np.arange(3, dtype=np.int8), K.shape[0])


def systems(tb):
    iso = ref.q1_box(9, mass=0.1)
    tet, _ = tet_box(tb)
    A3, comp = three_components(ref.q1_box(5, mass=0.1))
    return {
        "q1_9": (iso, None),
        "q1_9_aniso": (ref.q1_box(9, tensor=(9.0, 1.0, 1.0), mass=0.1), None),
        "tet_4x4x4": (ref.canonical(tet + 0.05 * ref.sp.diags(tet.diagonal())), None),
        "three_components": (A3, comp),
        "eliminated": (ref.eliminate(ref.q1_box(9), face_x0(9)), None),
    }


def run_driver(exe, d, name, A, comp, S):
    A = ref.canonical(A)
    open(os.path.join(d, name + ".meta"), "w").write("%d %d %d\n" % (A.shape[0], A.nnz, 0 if comp is None else 1))
    A.indptr.astype(np.int64).tofile(os.path.join(d, name + ".ptr"))
    A.indices.astype(np.int32).tofile(os.path.join(d, name + ".col"))
    np.asarray(S, dtype=np.uint8).tofile(os.path.join(d, name + ".str"))
    if comp is not None:
        np.asarray(comp, dtype=np.int8).tofile(os.path.join(d, name + ".comp"))
    r = subprocess.run([exe, d, name], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return r.stdout


def load(d, name, what, dtype):
    return np.fromfile(os.path.join(d, name + "." + what), dtype=dtype)


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("amgplanner"))
    exe = os.path.join(d, "amg_planner_driver")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-I", CSRC, os.path.join(ROOT, "tests", "amg_planner_driver.cpp"),
                           os.path.join(CSRC, "tb_amg_planners.cpp"), "-o", exe])
    return exe, d


@pytest.fixture(scope="module")
def cases(tb):
    return systems(tb)


@pytest.mark.parametrize("name", ["q1_9", "q1_9_aniso", "tet_4x4x4", "three_components", "eliminated"])
def test_planner_equals_the_restatement(driver, cases, name):
    exe, d = driver
    A, comp = cases[name]
    S = ref.strength(A, comp, THETA)
    want = ref.plan(A, comp, S)
    out = run_driver(exe, d, name, A, comp, S)
    assert out.split()[:4] == ["rc", "0", "nc", str(want["na"])], out
    agg = load(d, name, "agg", np.int32)
    assert np.array_equal(agg, want["agg"])
    # every dof with a strong neighbour sits in exactly one aggregate, every other dof in none; no aggregate is empty
    has_nbr = np.zeros(A.shape[0], dtype=bool)
    has_nbr[ref.rows_of(A)[S != 0]] = True
    assert np.array_equal(agg >= 0, has_nbr) and agg.max() == want["na"] - 1
    assert np.array_equal(load(d, name, "size", np.int32), np.bincount(agg[agg >= 0], minlength=want["na"])) and load(d, name, "size", np.int32).min() >= 1
    if name == "eliminated":
        assert (agg[face_x0(9)] == -1).all() and (agg >= 0).sum() == A.shape[0] - 81
    if comp is not None:                                     # aggregates never mix components
        assert np.array_equal(load(d, name, "ccomp", np.int8), want["ccomp"])
        assert np.array_equal(want["ccomp"][agg[agg >= 0]], comp[agg >= 0])
    for key, pre in (("P", "p"), ("R", "r"), ("AP", "ap"), ("Ac", "c")):
        assert np.array_equal(load(d, name, pre + "_ptr", np.int64), want[key][0]), key
        assert np.array_equal(load(d, name, pre + "_col", np.int32), want[key][1]), key
    assert np.array_equal(load(d, name, "r_perm", np.int64), want["r_perm"])
    assert np.array_equal(load(d, name, "p_row", np.int32), np.repeat(np.arange(A.shape[0]), np.diff(want["P"][0])))
    cptr, ccol = want["Ac"]
    diag = load(d, name, "c_diag", np.int64)
    assert (diag >= 0).all() and np.array_equal(ccol[diag], np.arange(want["na"]))
    print("%s: %d dofs -> %d aggregates, P %d, A.P %d, A_c %d non-zeros" % (name, A.shape[0], want["na"], len(want["P"][1]), len(want["AP"][1]), len(ccol)))


def test_planner_driver_under_sanitizers(tmp_path, cases):
    """the planner and its driver built with ASan + UBSan: a stand-alone host program, run on the 3-component system and on refused patterns"""
    exe = str(tmp_path / "amg_planner_driver_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                           os.path.join(ROOT, "tests", "amg_planner_driver.cpp"), os.path.join(CSRC, "tb_amg_planners.cpp"), "-o", exe])
    A, comp = cases["three_components"]
    S = ref.strength(A, comp, THETA)
    out = run_driver(exe, str(tmp_path), "c", A, comp, S)
    assert out.startswith("rc 0"), out
    assert np.array_equal(load(str(tmp_path), "c", "agg", np.int32), ref.plan(A, comp, S)["agg"])
    # an unsymmetric pattern is refused with the row named; so is a column outside the matrix (refused, not read)
    B = ref.canonical(A).tolil()
    B[7, 200] = 1.0
    B = ref.canonical(B.tocsr())
    out = run_driver(exe, str(tmp_path), "u", B, None, np.zeros(B.nnz, dtype=np.uint8))
    assert out.startswith("rc -1") and "row 7" in out and "symmetric" in out, out
    bad = ref.canonical(A).copy()
    bad.indices[-1] = A.shape[0]
    open(str(tmp_path / "b.meta"), "w").write("%d %d 0\n" % (A.shape[0], A.nnz))
    bad.indptr.astype(np.int64).tofile(str(tmp_path / "b.ptr"))
    bad.indices.astype(np.int32).tofile(str(tmp_path / "b.col"))
    np.zeros(A.nnz, dtype=np.uint8).tofile(str(tmp_path / "b.str"))
    r = subprocess.run([exe, str(tmp_path), "b"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith("rc -1") and "outside" in r.stdout, r.stdout + r.stderr


def reference_count(n_nodes, tensor=(1.0, 1.0, 1.0)):
    A = ref.eliminate(ref.q1_box(n_nodes, tensor=tensor), face_x0(n_nodes))
    levels = ref.hierarchy(A, None, None, THETA, max_coarse=32)
    b = np.random.default_rng(11).normal(size=A.shape[0])
    b[face_x0(n_nodes)] = 0.0
    _, it, _ = ref.pcg(A, b, lambda r: ref.vcycle(levels, r, 2, 4.0), rtol=1e-8)
    _, itj, _ = ref.pcg(A, b, ref.jacobi(A), rtol=1e-8)
    return it, itj, len(levels)


def test_reference_counts_do_not_grow_with_the_grid():
    """what the GPU tests lean on: the restatement is a multigrid — its isotropic count at 17³ nodes is at most its count at 9³ plus 2"""
    it9, j9, nl9 = reference_count(9)
    it17, j17, nl17 = reference_count(17)
    print("AMG-PCG iterations 9^3: %d (%d levels, Jacobi %d)   17^3: %d (%d levels, Jacobi %d)" % (it9, nl9, j9, it17, nl17, j17))
    assert nl9 >= 2 and nl17 >= 3
    assert it17 <= it9 + 2
    assert it9 < j9 and it17 < j17


def test_test_matrices_have_no_strength_ties(cases):
    """no |a_ij| of the test matrices lies within 1e-9 relative of θ·m_i on any level: the device and the restatement decide strength identically"""
    for name, (A, comp) in cases.items():
        levels = ref.hierarchy(A, comp, None, THETA, max_coarse=32)
        margins = [ref.strength_margin(lev["A"], lev["comp"], THETA) for lev in levels[:-1]]
        print("%s: %d levels, smallest relative distance from the threshold %.3e" % (name, len(levels), min(margins)))
        assert min(margins) > 1e-9


def test_recipes_refuse_what_is_out_of_scope(tb):
    with pytest.raises(NotImplementedError, match="V-cycles"):
        tb.AMGPrecon(cycle="W")
    with pytest.raises(NotImplementedError, match="V-cycles"):
        tb.AMGPrecon(cycle="F")
    with pytest.raises(NotImplementedError, match="smoother"):
        tb.AMGPrecon(smoother="gauss-seidel")
    with pytest.raises(NotImplementedError, match="GMRES"):
        tb.KrylovMGSolver("gmres", tb.AMGPrecon())
    assert tb.KrylovMGSolver("cg", tb.AMGPrecon()).mg.theta == 0.25
    chained = tb.ChainedMGPrecon(tb.PMGPrecon(), tb.AMGPrecon(max_coarse=32))
    assert chained.gh is None and chained.coarse.max_coarse == 32
    with pytest.raises(ValueError, match="disagree"):
        tb.ChainedMGPrecon(tb.PMGPrecon(degree=3), tb.AMGPrecon())
    gh = tb.GridHierarchy(tb.generate_mesh(tb.Hexahedron, (2, 2, 2), (0, 0, 0), (1, 1, 1)), 1)
    assert tb.GMGPrecon(gh).coarse is None and tb.GMGPrecon(gh, coarse=tb.AMGPrecon()).coarse.theta == 0.25
    with pytest.raises(TypeError, match="AMGPrecon"):
        tb.GMGPrecon(gh, coarse="amg")
    whole = tb.DofHandler(gh.grids[-1])
    tb.AMGPrecon().check(whole)
    part = tb.DofHandler(gh.grids[-1], cell_dofs=whole.cell_dofs[:whole.cell_dofs.shape[0] // 2], ndofs=whole.ndofs)      # a handler over half of the cells
    with pytest.raises(NotImplementedError, match="subdomain dof handlers are out of scope"):
        tb.AMGPrecon().check(part)
    labels = tb.amg.component_labels(tb.DofHandler(gh.grids[-1], tb.LagrangeCollection(1) ** 3))
    assert labels.dtype == np.int8 and np.array_equal(np.bincount(labels), [whole.ndofs] * 3) and tb.amg.component_labels(whole) is None


def test_abi_paperwork():
    header = open(os.path.join(ROOT, "include", "tbhip.h"), encoding="utf-8").read()
    julia = open(os.path.join(ROOT, "julia", "ThunderboltHIPBackend.jl"), encoding="utf-8").read()
    integ = open(os.path.join(ROOT, "INTEGRATION.md"), encoding="utf-8").read()
    assert "multigrid.jl:27" in header
    for name in ("tb_amg_create", "tb_amg_setup", "tb_amg_replan", "tb_amg_apply", "tb_amg_destroy", "tb_pcg_solve_amg", "tb_amg_n_levels", "tb_amg_level_size",
                 "tb_amg_level_csr", "tb_amg_level_prolongator", "tb_amg_level_aggregates", "tb_amg_level_strength", "tb_amg_level_lambda_max",
                 "tb_mg_set_coarse_amg", "tb_mg_coarse_amg"):
        assert "int %s(" % name in header, name
        assert ":%s" % name in julia, name
        assert name in integ, name
