"""The smoothed-aggregation multigrid on the device (tb_amg.hip) against the SciPy restatement of tests/amg_reference.py: strength bytes, aggregates,
prolongators and level matrices, one V-cycle, the preconditioned solve — on heat matrices of hexahedral and tetrahedral boxes with one face fixed, an
anisotropic one and a 3-component elasticity tangent — and as the coarse solver of a p- and of a geometric hierarchy (tb_mg_set_coarse_amg).
max_coarse = 32 makes these small systems produce 2 – 3 levels."""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.sparse as sparse

import amg_reference as ref
import multigrid_reference as mref
import pmultigrid_reference as pref
from gmg_case import face_dofs, gmg_problem, heat_values

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "amg_parent_gmg_solution.npz")
MAX_COARSE, DEGREE, RATIO = 32, 2, 4.0
CASES = ["hex9", "hex17", "hex9_aniso", "tet", "elasticity"]


def csr_of(sp, vals):
    n = len(sp.rowptr) - 1
    return sparse.csr_matrix((np.asarray(vals, dtype=np.float64), sp.colidx.astype(np.int32), sp.rowptr.astype(np.int64)), shape=(n, n))


class Case:
    """one system: the eliminated matrix on the device, its AMG hierarchy after one setup, the restatement fed with the device's λ"""

    def __init__(self, tb, device, name):
        self.name = name
        if name == "elasticity":
            grid = tb.generate_mesh(tb.Hexahedron, (5, 5, 5), (0, 0, 0), (1, 1, 1), perturb=0.1)
            dh = tb.DofHandler(grid, tb.LagrangeCollection(1) ** 3)
            sp = tb.allocate_matrix(dh)
            ms = tb.ConstantCoefficient(tb.OrthotropicMicrostructure(*np.eye(3)))
            op = tb.setup_operator(tb.ElementAssemblyStrategy(device), tb.QuasiStaticModel("d", tb.PK1Model(tb.HolzapfelOgden2009Model(a=1.0, b=1.0, af=0.0, as_=0.0, afs=0.0, beta=1.0), ms), []), dh, sp)
            u = np.random.default_rng(5).uniform(-5e-3, 5e-3, dh.ndofs)
            u[face_dofs(tb, dh)] = 0.0
            tb.update_linearization(op, device.to_device(u), 0.0, residual=device.zeros(dh.ndofs))
            vals, pattern = op.J.to_host(), op.pattern
            self.keep = op
        else:
            if name == "tet":
                grid = tb.generate_mesh(tb.Tetrahedron, (4, 4, 4), (0, 0, 0), (1, 1, 1))
            else:
                nel = 16 if name == "hex17" else 8
                grid = tb.generate_mesh(tb.Hexahedron, (nel, nel, nel), (0, 0, 0), (1, 1, 1), perturb=0.1)
            dh = tb.DofHandler(grid)
            sp = tb.allocate_matrix(dh)
            if name == "hex9_aniso":
                D = tb.SpectralTensorCoefficient(tb.ConstantCoefficient(tb.TransverselyIsotropicMicrostructure([1.0, 0.0, 0.0])), tb.ConstantCoefficient([9.0, 1.0]))
            else:
                D = tb.ConstantCoefficient(np.eye(3))
            vals, pattern = heat_values(tb, device, dh, sp, D)
        self.dh, self.sp, self.pattern = dh, sp, pattern
        self.ch = tb.ConstraintHandler(dh, face_dofs(tb, dh))
        self.dA = device.to_device(vals)
        tb.apply_zero(self.dA, None, self.ch, pattern=pattern)
        self.A = ref.canonical(csr_of(sp, self.dA.to_host()))
        assert np.array_equal(self.A.indices, sp.colidx) and np.array_equal(self.A.indptr, sp.rowptr)          # sorted columns: the restatement sees the device's order
        self.comp = tb.amg.component_labels(dh)
        self.amg = tb.AMGPrecon(max_coarse=MAX_COARSE, degree=DEGREE, interval_ratio=RATIO).materialize(pattern, self.ch)
        self.amg.setup(self.dA)
        self.nl = self.amg.n_levels
        self.lam = [self.amg.lambda_max(l) for l in range(self.nl - 1)]
        self.levels = ref.hierarchy(self.A, self.comp, self.lam, 0.25, MAX_COARSE)
        rng = np.random.default_rng(17)
        self.b = rng.normal(size=dh.ndofs)
        self.b[self.ch.prescribed_dofs] = 0.0


_cases = {}


@pytest.fixture(params=CASES)
def case(request, tb, device):
    if request.param not in _cases:
        _cases[request.param] = Case(tb, device, request.param)
    return _cases[request.param]


def relmax(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


# ------------------------------------------------------------------------------------------------ setup
def test_strength_and_aggregates_equal_the_reference(case):
    amg, levels = case.amg, case.levels
    assert case.nl == len(levels) and case.nl >= 2
    sizes = [amg.level_size(l) for l in range(case.nl)]
    print("%s: levels (dofs, non-zeros, aggregates) %s" % (case.name, sizes))
    assert sizes[-1][0] <= MAX_COARSE
    for l in range(case.nl - 1):
        margin = ref.strength_margin(levels[l]["A"], levels[l]["comp"], 0.25)
        assert margin > 1e-9, "a strength tie on level %d: the comparison below would be of roundings" % l
        assert np.array_equal(amg.strength(l), levels[l]["S"]), l
        assert np.array_equal(amg.aggregates(l), levels[l]["agg"]), l
        assert sizes[l][2] == levels[l]["plan"]["na"] == sizes[l + 1][0]
    assert (amg.aggregates(0)[case.ch.prescribed_dofs] == -1).all()                            # eliminated rows stay outside every aggregate


def test_prolongators_and_level_matrices_agree(case):
    amg, levels = case.amg, case.levels
    for l in range(case.nl):
        A, want = amg.level_matrix(l), levels[l]["A"]
        assert np.array_equal(A.indptr, want.indptr) and np.array_equal(A.indices, want.indices), "pattern of A_%d" % l
        eA = relmax(A.data, want.data)
        msg = "%s level %d: A %.2e" % (case.name, l, eA)
        assert eA <= 1e-13, msg
        if l < case.nl - 1:
            P, wantP = amg.prolongator(l), levels[l]["P"]
            assert np.array_equal(P.indptr, wantP.indptr) and np.array_equal(P.indices, wantP.indices), "pattern of P_%d" % l
            eP = relmax(P.data, wantP.data)
            exact = ref.lambda_max_exact(want)
            print(msg + "  P %.2e  lambda_max %.6f (exact %.6f)" % (eP, case.lam[l], exact))
            assert eP <= 1e-13
            assert case.lam[l] >= exact
            assert np.diff(P.indptr)[amg.aggregates(l) < 0].max(initial=0) == 0                   # rows of outside dofs are empty


def test_two_setups_and_two_applies_give_the_same_bits(case, device):
    amg = case.amg
    before = [amg.level_matrix(l).data.copy() for l in range(case.nl)], [amg.prolongator(l).data.copy() for l in range(case.nl - 1)]
    r = device.to_device(case.b)
    z1 = amg.apply(r, device.zeros(len(case.b))).to_host()
    amg.setup(case.dA)
    for l in range(case.nl):
        assert np.array_equal(before[0][l], amg.level_matrix(l).data), l
    for l in range(case.nl - 1):
        assert np.array_equal(before[1][l], amg.prolongator(l).data), l
        assert amg.lambda_max(l) == case.lam[l]
    z2 = amg.apply(r, device.zeros(len(case.b))).to_host()
    assert np.array_equal(z1, z2)


def test_numeric_setup_of_the_doubled_matrix_doubles_every_level(case, device):
    """the plan stays: same aggregates and patterns; scaling by 2 is exact in every sum, D⁻¹A and with it λ and P keep their bits"""
    amg = case.amg
    As = [amg.level_matrix(l) for l in range(case.nl)]
    Ps = [amg.prolongator(l) for l in range(case.nl - 1)]
    aggs = [amg.aggregates(l) for l in range(case.nl - 1)]
    d2 = device.to_device(2.0 * case.dA.to_host())
    try:
        amg.setup(d2)
        for l in range(case.nl):
            B = amg.level_matrix(l)
            assert np.array_equal(B.indptr, As[l].indptr) and np.array_equal(B.indices, As[l].indices)
            assert np.array_equal(B.data, 2.0 * As[l].data), l
        for l in range(case.nl - 1):
            assert np.array_equal(amg.aggregates(l), aggs[l])
            assert np.array_equal(amg.prolongator(l).data, Ps[l].data) and amg.lambda_max(l) == case.lam[l]
    finally:
        amg.setup(case.dA)


# ------------------------------------------------------------------------------------------------ cycle
def test_cycle_is_symmetric_positive_and_zero_at_prescribed_dofs(case, device):
    n = len(case.b)
    rng = np.random.default_rng(7)
    u, v = rng.normal(size=n), rng.normal(size=n)
    u[case.ch.prescribed_dofs] = 0.0
    v[case.ch.prescribed_dofs] = 0.0
    mu = case.amg.apply(device.to_device(u), device.zeros(n)).to_host()
    mv = case.amg.apply(device.to_device(v), device.zeros(n)).to_host()
    asym = abs(mu @ v - u @ mv) / abs(mu @ v)
    print("%s: <Mu, v> %.15e  <u, Mv> %.15e  relative difference %.2e,  <Mu, u> %.3e" % (case.name, mu @ v, u @ mv, asym, mu @ u))
    assert asym <= 1e-12 and mu @ u > 0.0
    assert (mu[case.ch.prescribed_dofs] == 0.0).all()


def test_cycle_agrees_with_the_reference(case, device):
    z = case.amg.apply(device.to_device(case.b), device.zeros(len(case.b))).to_host()
    want = ref.vcycle(case.levels, case.b, DEGREE, RATIO)
    err = relmax(z, want)
    print("%s: one V-cycle, max |z - z_ref| / max |z_ref| = %.2e" % (case.name, err))
    assert err <= 1e-12


def test_cycle_replays_from_a_graph_with_the_same_bits(tb, device):
    case = _cases.get("hex9") or Case(tb, device, "hex9")
    n = len(case.b)
    r = device.to_device(case.b)
    z1, z2 = device.zeros(n), device.zeros(n)
    case.amg.apply(r, z1)
    graph = device.capture(lambda: case.amg.apply(r, z2))
    graph.launch()
    device.synchronize()
    assert np.array_equal(z1.to_host(), z2.to_host()) and np.abs(z1.to_host()).max() > 0.0
    graph.close()


# ------------------------------------------------------------------------------------------------ solve
def test_pcg_count_matches_the_reference_and_beats_jacobi(tb, case, device):
    n = len(case.b)
    b = device.to_device(case.b)
    x = device.zeros(n)
    it, res = tb.pcg_solve(case.pattern, case.dA, b, x, rtol=1e-8, atol=0.0, maxiter=500, precond=case.amg)
    xr, itr, resr = ref.pcg(case.A, case.b, lambda r: ref.vcycle(case.levels, r, DEGREE, RATIO), rtol=1e-8)
    xj = device.zeros(n)
    itj, _ = tb.pcg_solve(case.pattern, case.dA, b, xj, rtol=1e-8, atol=0.0, maxiter=5000, precond="jacobi")
    true_res = np.linalg.norm(case.b - case.A @ x.to_host())
    print("%s: AMG-PCG %d iterations (reference %d), Jacobi-PCG %d; residual %.3e (true %.3e, reference %.3e)" % (case.name, it, itr, itj, res, true_res, resr))
    assert abs(it - itr) <= 2
    assert it < itj
    assert true_res <= 1.01e-8 * np.linalg.norm(case.b) + 1e-14
    assert relmax(x.to_host(), xr) <= 1e-6


def test_protocol_callers_accept_the_recipe(tb, device):
    """pcg_solve, KrylovMGSolver and the Newton solver's materialize protocol take an AMGPrecon as they take a GMGPrecon"""
    case = _cases.get("tet") or Case(tb, device, "tet")
    n = len(case.b)
    recipe = tb.AMGPrecon(max_coarse=MAX_COARSE)
    x1, x2 = device.zeros(n), device.zeros(n)
    it1, _ = tb.pcg_solve(case.pattern, case.dA, device.to_device(case.b), x1, rtol=1e-8, atol=0.0, precond=recipe)
    it2, _ = tb.KrylovMGSolver("cg", recipe, rtol=1e-8, atol=0.0).solve(case.pattern, case.dA, device.to_device(case.b), x2, case.ch)
    assert it1 == it2 and 0 < it1 < 30 and np.array_equal(x1.to_host(), x2.to_host())
    mg = recipe.materialize(case.pattern, case.ch)
    assert mg is recipe.materialize(case.pattern) and mg.n_levels == case.nl
    mg.replan()
    assert mg.setup(case.dA).n_levels == case.nl and np.array_equal(mg.aggregates(0), case.amg.aggregates(0))


# ------------------------------------------------------------------------------------------------ AMG below a p- or h-hierarchy
def mg_cycle(As, Ps, pres, lmax, r, coarse, level=None):
    """multigrid_reference.vcycle with the coarsest solve handed in"""
    l = len(As) - 1 if level is None else level
    if l == 0:
        return coarse(r)
    dinv = np.where(pres[l], 0.0, 1.0 / np.diag(As[l]))
    x = mref.chebyshev(As[l], dinv, lmax[l], RATIO, DEGREE, r)
    x = x + Ps[l] @ mg_cycle(As, Ps, pres, lmax, Ps[l].T @ (r - As[l] @ x), coarse, l - 1)
    return mref.chebyshev(As[l], dinv, lmax[l], RATIO, DEGREE, r, x)


def check_hierarchy_over_amg(tb, device, mg, dh, pattern, dA, ch, As, Ps, pres):
    mg.setup(dA)
    inner = mg.coarse_hierarchy()
    assert inner is not None and inner.n_levels >= 2 and inner.level_size(0)[0] == mg.dhs[0].ndofs > MAX_COARSE
    lam_in = [inner.lambda_max(l) for l in range(inner.n_levels - 1)]
    A0 = ref.canonical(csr_of(mg.sps[0], mref.dense_to_csr(mg.sps[0], As[0])))
    levels = ref.hierarchy(A0, tb.amg.component_labels(mg.dhs[0]), lam_in, 0.25, MAX_COARSE)
    assert len(levels) == inner.n_levels
    assert relmax(inner.level_matrix(0).data, A0.data) <= 1e-12
    lmax = [None] + [mg.lambda_max(l) for l in range(1, mg.n_levels)]
    rng = np.random.default_rng(23)
    r = rng.normal(size=dh.ndofs)
    r[ch.prescribed_dofs] = 0.0
    z = mg.apply(device.to_device(r), device.zeros(dh.ndofs)).to_host()
    want = mg_cycle(As, Ps, pres, lmax, r, lambda rc: ref.vcycle(levels, rc, DEGREE, RATIO))
    err = relmax(z, want)
    x = device.zeros(dh.ndofs)
    it, res = mg.solve(dA, device.to_device(r), x, rtol=1e-8, atol=0.0, maxiter=200)
    Ah = csr_of(pattern.sp, dA.to_host())
    true_res = np.linalg.norm(r - Ah @ x.to_host())
    print("%d levels over %d AMG levels: cycle error %.2e, %d iterations, residual %.3e (true %.3e)" % (mg.n_levels, inner.n_levels, err, it, res, true_res))
    assert err <= 1e-12
    assert it < 40 and true_res <= 1.01e-8 * np.linalg.norm(r)
    assert (z[ch.prescribed_dofs] == 0.0).all()


def test_p_level_over_amg(tb, device):
    """ChainedMGPrecon(PMGPrecon(), AMGPrecon()): the reference's default pcoarse_solver; the first-order level (64 dofs) exceeds max_coarse"""
    dh = tb.DofHandler(tb.generate_mesh(tb.Hexahedron, (3, 3, 3), (0, 0, 0), (1, 1, 1), perturb=0.1), tb.LagrangeCollection(2))
    sp = tb.allocate_matrix(dh)
    st = tb.ElementAssemblyStrategy(device)
    K = tb.update_operator(tb.setup_operator(st, tb.BilinearDiffusionIntegrator(tb.ConstantCoefficient(np.eye(3))), dh, sp), 0.0)
    M = tb.update_operator(tb.setup_operator(st, tb.BilinearMassIntegrator(tb.ConstantCoefficient(1.0)), dh, sp), 0.0)
    ch = tb.ConstraintHandler(dh, face_dofs(tb, dh))
    dA = device.to_device(M.A.to_host() - 0.1 * K.A.to_host())
    tb.apply_zero(dA, None, ch, pattern=K.pattern)
    mg = tb.ChainedMGPrecon(tb.PMGPrecon(), tb.AMGPrecon(max_coarse=MAX_COARSE)).materialize(K.pattern, ch)
    assert mg.n_levels == 2
    flags = np.zeros(dh.ndofs, dtype=bool)
    flags[ch.prescribed_dofs] = True
    Ad = mref.csr_to_dense(sp, dA.to_host())
    P, cpre = pref.dense_p_level(tb, dh, mg.dhs[0], flags)
    check_hierarchy_over_amg(tb, device, mg, dh, K.pattern, dA, ch, [mref.galerkin(P, Ad, cpre), Ad], [None, P], [cpre, flags])


def gmg_solution(tb, device, vals=None):
    """what the stored arrays were recorded with on the parent commit: GMGPrecon(gh) through pcg_solve, one cycle, the coarsest operator and its λmax.
    vals: the eliminated matrix (None: assembled here — two assemblies may differ in their last bits, so the stored run keeps its own)"""
    gh, dh, sp, pattern, dA, ch, b = gmg_problem(tb, device)
    if vals is not None:
        dA = device.to_device(vals)
    mg = tb.GMGPrecon(gh).materialize(pattern, ch)
    x = device.zeros(dh.ndofs)
    it, res = tb.pcg_solve(pattern, dA, device.to_device(b), x, rtol=1e-10, atol=0.0, maxiter=100, precond=mg)
    z = mg.apply(device.to_device(b), device.zeros(dh.ndofs)).to_host()
    return dict(vals=dA.to_host(), x=x.to_host(), z=z, iterations=np.int64(it), resnorm=np.float64(res), A0=mg.level_matrix(0), lmax=np.float64(mg.lambda_max(1)))


def test_geometric_levels_over_amg(tb, device):
    gh, dh, sp, pattern, dA, ch, b = gmg_problem(tb, device)
    mg = tb.GMGPrecon(gh, coarse=tb.AMGPrecon(max_coarse=MAX_COARSE)).materialize(pattern, ch)
    flags = np.zeros(dh.ndofs, dtype=bool)
    flags[ch.prescribed_dofs] = True
    As, Ps, pres = mref.hierarchy(gh, mg.dhs, mref.csr_to_dense(sp, dA.to_host()), flags)
    check_hierarchy_over_amg(tb, device, mg, dh, pattern, dA, ch, As, Ps, pres)


def test_geometric_multigrid_without_amg_keeps_the_parents_bits(tb, device):
    """GMGPrecon(gh) on the same box, on the matrix values stored with the record: the coarsest operator, λmax, one cycle, the iteration count, the
    residual norm and the solution are, bit for bit, what the commit before the AMG returned (tests/golden/amg_parent_gmg_solution.npz)"""
    gold = np.load(GOLDEN)
    got = gmg_solution(tb, device, gold["vals"])
    assert relmax(gmg_problem(tb, device)[4].to_host(), gold["vals"]) <= 1e-13                    # the stored matrix is this problem's
    dx = relmax(got["x"], gold["x"])
    print("A0 %s  lmax %s  z %s  iterations %d / %d  x max difference %.2e  resnorm %.17e / %.17e" % (
        np.array_equal(got["A0"], gold["A0"]), got["lmax"] == gold["lmax"], np.array_equal(got["z"], gold["z"]), got["iterations"], gold["iterations"], dx,
        got["resnorm"], gold["resnorm"]))
    assert np.array_equal(got["A0"], gold["A0"]) and got["lmax"] == gold["lmax"]
    assert np.array_equal(got["z"], gold["z"])
    assert got["iterations"] == gold["iterations"] and got["resnorm"] == gold["resnorm"]
    assert np.array_equal(got["x"], gold["x"])


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(tb, device):
    L, lib = tb._lib, tb.lib()
    # a last level above 1 024 dofs: 33³ nodes aggregate to about 11³, and two levels are the most allowed
    grid = tb.generate_mesh(tb.Hexahedron, (32, 32, 32), (0, 0, 0), (1, 1, 1))
    dh = tb.DofHandler(grid)
    sp = tb.allocate_matrix(dh)
    vals, pattern = heat_values(tb, device, dh, sp, tb.ConstantCoefficient(np.eye(3)))
    dA = device.to_device(vals)
    big = tb.AMGPrecon(max_coarse=MAX_COARSE, max_levels=2).materialize(pattern)
    with pytest.raises(tb._lib.TBError, match="max_levels") as e:
        big.setup(dA)
    assert e.value.code == L.TB_ERR_UNSUPPORTED
    r, z = device.zeros(dh.ndofs), device.zeros(dh.ndofs)
    assert lib.tb_amg_apply(big.h, r.ptr, z.ptr) == L.TB_ERR_BAD_ARG                            # no numeric setup
    # setup inside an open capture refuses, and the capture survives
    ok = tb.AMGPrecon(max_coarse=MAX_COARSE).materialize(pattern)
    tb.check(lib.tb_graph_begin(device.h))
    rc = lib.tb_amg_setup(ok.h, dA.ptr, 2, 4.0)
    h = C.c_void_p()
    tb.check(lib.tb_graph_end(device.h, C.byref(h)))
    if h:
        lib.tb_graph_destroy(h)
    assert rc == L.TB_ERR_BAD_ARG
    assert ok.setup(dA).n_levels >= 3
    # an unsymmetric pattern: row 0 gains the last column, the last row does not gain column 0 — the row is named
    n = dh.ndofs
    rowptr2 = sp.rowptr.copy()
    rowptr2[1:] += 1
    sp2 = tb.api.SparsityPattern(rowptr2, np.insert(sp.colidx, sp.rowptr[1], n - 1).astype(np.int32))
    p2 = dh.device_mesh(device).pattern(sp2)
    out = C.c_void_p()
    rc = lib.tb_amg_create(p2.h, None, 0.25, 32, 16, C.byref(out))
    assert rc == L.TB_ERR_BAD_ARG and b"row 0 " in lib.tb_last_error_string() and b"symmetric" in lib.tb_last_error_string()
    # the bidomain block system takes GMGPrecon only
    D = tb.ConstantCoefficient(np.eye(3))
    with pytest.raises(NotImplementedError, match="out of scope"):
        tb.BidomainBackwardEulerStage(tb.BackwardEulerSolver(), tb.PerColorAssemblyStrategy(device), dh, D, D, [0], precond=tb.AMGPrecon())


def test_the_tetrahedral_example_runs():
    """examples/amg_tet_ecg.py: heat steps on a tetrahedral box at toy size — the AMG takes fewer iterations than Jacobi and both reach the same field"""
    import json, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "examples", "amg_tet_ecg.py")], capture_output=True, text=True, timeout=300, cwd=root)
    assert out.returncode == 0, out.stderr[-2000:]
    rec = json.loads(out.stdout.strip().splitlines()[-1])
    print(rec)
    assert len(rec["levels"]) >= 2 and rec["levels"][-1] <= 64
    assert max(rec["iterations_amg"]) < min(rec["iterations_jacobi"])
    assert rec["max_relative_difference"] <= 1e-7
