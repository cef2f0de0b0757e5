"""The smoothed aggregation with rigid-body modes on the device (tb_amg_block.hip) against the restatement of tests/amg_elasticity_reference.py, fed with
the device's λ per level: node map, strength bytes, aggregates, dead flags, candidates, tentative and smoothed prolongators, level matrices, one V-cycle,
the preconditioned solve — on device tangents of the isotropic Holzapfel–Ogden model at a small random displacement — through the protocol callers,
below a p- and a geometric hierarchy, the refusals, and the scalar method's bits against those recorded on the commit before the near-null-space
(tests/golden/amg_scalar_parent_bits.npz, tests/amg_parent_bits.py).  max_coarse = 32, V(2, 2), θ = 0.25 unless the case says otherwise.

TOL is the bound of tests/test_amg_gpu.py, 1e-13 of the largest entry: the distances to the restatement measured on an MI355X — B 1.8e-16, T 1.0e-15,
P 1.4e-15, A_l 1.2e-15, TᵀT 3.4e-15, T B_{l+1} = B_l 2.2e-16, P B_{l+1} = (I − ω D⁻¹ A) B_l 6.7e-16, the largest over all cases and levels — stay under
a tenth of it.  Every test prints the distances it measures before it asserts."""
import ctypes as C
import os

import numpy as np
import pytest
import scipy.sparse as sparse

import amg_elasticity_reference as eref
import amg_parent_bits as parent_bits
import amg_reference as ref
from gmg_case import face_dofs

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "amg_scalar_parent_bits.npz")
MAX_COARSE, DEGREE, RATIO = 32, 2, 4.0
TOL = 1e-13
THETA = {"cube": 0.25, "beam": 0.25, "roller": 0.25, "tet": 0.25, "small_aggregates": 0.7}


def csr_of(sp, vals):
    n = len(sp.rowptr) - 1
    return sparse.csr_matrix((np.asarray(vals, dtype=np.float64), sp.colidx.astype(np.int32), sp.rowptr.astype(np.int64)), shape=(n, n))


def relmax(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def material(tb):
    ms = tb.ConstantCoefficient(tb.OrthotropicMicrostructure(*np.eye(3)))
    return tb.QuasiStaticModel("d", tb.PK1Model(tb.HolzapfelOgden2009Model(a=1.0, b=1.0, af=0.0, as_=0.0, afs=0.0, beta=1.0), ms), [])


def tangent(tb, device, dh, sp, pres, seed=5):
    """the Holzapfel–Ogden tangent at a small random displacement that vanishes at the prescribed dofs → (operator, pattern)"""
    op = tb.setup_operator(tb.ElementAssemblyStrategy(device), material(tb), dh, sp)
    u = np.random.default_rng(seed).uniform(-5e-3, 5e-3, dh.ndofs)
    u[pres] = 0.0
    tb.update_linearization(op, device.to_device(u), 0.0, residual=device.zeros(dh.ndofs))
    return op


class Case:
    def __init__(self, tb, device, name):
        self.name, self.theta = name, THETA[name]
        if name == "tet":
            grid = tb.generate_mesh(tb.Tetrahedron, (4, 4, 4), (0, 0, 0), (1, 1, 1))
        elif name == "beam":
            grid = tb.generate_mesh(tb.Hexahedron, (16, 4, 4), (0, 0, 0), (4, 1, 1), perturb=0.1)
        else:
            grid = tb.generate_mesh(tb.Hexahedron, (4, 4, 4), (0, 0, 0), (1, 1, 1), perturb=0.1)
        dh = tb.DofHandler(grid, tb.LagrangeCollection(1) ** 3)
        sp = tb.allocate_matrix(dh)
        comp = tb.amg.component_labels(dh)
        if name == "roller":
            pres = np.concatenate([d[comp[d] == a] for a, d in ((a, face_dofs(tb, dh, axis=a)) for a in range(3))])
        else:
            pres = face_dofs(tb, dh)
        self.keep = tangent(tb, device, dh, sp, pres)
        self.dh, self.sp, self.pattern = dh, sp, self.keep.pattern
        self.ch = tb.ConstraintHandler(dh, pres)
        self.dA = device.to_device(self.keep.J.to_host())
        tb.apply_zero(self.dA, None, self.ch, pattern=self.pattern)
        self.A = ref.canonical(csr_of(sp, self.dA.to_host()))
        assert np.array_equal(self.A.indices, sp.colidx) and np.array_equal(self.A.indptr, sp.rowptr)
        self.node, self.n_nodes, self.B = tb.amg.dof_nodes(dh), len(grid.xyz), tb.amg.rigid_body_modes(dh)
        self.recipe = tb.AMGPrecon(theta=self.theta, max_coarse=MAX_COARSE, degree=DEGREE, interval_ratio=RATIO, near_nullspace="rigid_body")
        self.amg = self.recipe.materialize(self.pattern, self.ch)
        self.amg.setup(self.dA)
        self.nl = self.amg.n_levels
        self.lam = [self.amg.lambda_max(l) for l in range(self.nl - 1)]
        self.levels = eref.hierarchy(self.A, self.node, self.n_nodes, self.B, self.lam, self.theta, MAX_COARSE)
        self.b = np.random.default_rng(17).normal(size=dh.ndofs)
        self.b[self.ch.prescribed_dofs] = 0.0


_cases = {}


def get_case(tb, device, name):
    if name not in _cases:
        _cases[name] = Case(tb, device, name)
    return _cases[name]


@pytest.fixture(params=list(THETA))
def case(request, tb, device):
    return get_case(tb, device, request.param)


# ------------------------------------------------------------------------------------------------ 1. structure
def test_structure_equals_the_restatement(case):
    amg, levels = case.amg, case.levels
    assert case.nl == len(levels) and case.nl >= 2
    sizes = [amg.level_size(l) for l in range(case.nl)]
    print("%s: levels (dofs, non-zeros, coarse dofs) %s, operator complexity %.3f" % (case.name, sizes, sum(s[1] for s in sizes) / sizes[0][1]))
    assert sizes[-1][0] <= MAX_COARSE
    ratios = np.concatenate([lev["ratios"] for lev in levels[:-1]])
    print("%s: dead columns %d, norm ratios: smallest live %.3g, largest dead %.3g" % (case.name, int(sum(lev["dead"].sum() for lev in levels[:-1])),
                                                                                      ratios[ratios > 1e-8].min(), ratios[ratios <= 1e-8].max(initial=0.0)))
    assert not ((ratios > 1e-12) & (ratios < 1e-4)).any(), "a column near the dead threshold: the flags below would compare roundings"
    for l in range(case.nl - 1):
        lev = levels[l]
        margin = ref.strength_margin(lev["G"], None, case.theta)
        assert margin > 1e-9, "a node-strength tie on level %d" % l
        assert np.array_equal(amg.nodes(l), lev["node"]), l
        assert np.array_equal(amg.strength(l), lev["S"]), l
        assert np.array_equal(amg.aggregates(l), lev["agg"]), l
        assert np.array_equal(amg.dead(l), lev["dead"]), l
        assert sizes[l][2] == lev["plan"]["nc"] == sizes[l + 1][0] == 6 * lev["plan"]["na"]
    assert np.array_equal(amg.nodes(case.nl - 1), levels[-1]["node"])
    pres, agg0, B0 = case.ch.prescribed_dofs, amg.aggregates(0), amg.near_nullspace(0)
    held = np.bincount(case.node[pres], minlength=case.n_nodes)[case.node[pres]]
    assert (agg0[pres][held == 3] == -1).all()                                       # all three dofs of a clamped node lie outside every aggregate
    assert not B0[pres].any()
    if case.name == "roller":
        assert (held < 3).sum() > 0 and (agg0[pres][held < 3] >= 0).all()            # a roller node lies inside one, with a zero row of B
    if case.name == "small_aggregates":
        assert sum(int(lev["dead"].sum()) for lev in levels[:-1]) >= 1


# ------------------------------------------------------------------------------------------------ 2. tentative prolongator
def test_tentative_prolongator(case):
    amg, levels = case.amg, case.levels
    worst = {}
    for l in range(case.nl - 1):
        lev = levels[l]
        B, T, Bn, dead = amg.near_nullspace(l), amg.tentative(l), amg.near_nullspace(l + 1), amg.dead(l).astype(bool)
        assert not Bn[dead].any()                                                    # R's row of a dead column is zero
        assert np.array_equal(T.indptr, lev["T"].indptr) and np.array_equal(T.indices, lev["T"].indices)
        e = dict(B=relmax(B, lev["B"]), T=relmax(T.data, lev["T"].data), Bn=relmax(Bn, levels[l + 1]["B"]))
        TtT = (T.T @ T).toarray()
        e["TtT"] = float(np.abs(TtT - np.diag((~dead).astype(float))).max())
        e["TB"] = relmax(T @ Bn, B)
        print("%s level %d: %s" % (case.name, l, "  ".join("%s %.2e" % kv for kv in e.items())))
        for k, v in e.items():
            worst[k] = max(worst.get(k, 0.0), v)
        assert not T[amg.aggregates(l) < 0].nnz or not T[amg.aggregates(l) < 0].data.any()
    assert max(worst.values()) <= TOL, worst


# ------------------------------------------------------------------------------------------------ 3. prolongator and level matrices
def test_prolongators_and_level_matrices(case):
    amg, levels = case.amg, case.levels
    for l in range(case.nl):
        A, want = amg.level_matrix(l), levels[l]["A"]
        assert np.array_equal(A.indptr, want.indptr) and np.array_equal(A.indices, want.indices), "pattern of A_%d" % l
        eA = relmax(A.data, want.data)
        msg = "%s level %d: A %.2e" % (case.name, l, eA)
        assert eA <= TOL, msg
        if l < case.nl - 1:
            P, wantP = amg.prolongator(l), levels[l]["P"]
            assert np.array_equal(P.indptr, wantP.indptr) and np.array_equal(P.indices, wantP.indices), "pattern of P_%d" % l
            eP = relmax(P.data, wantP.data)
            B, Bn, agg = amg.near_nullspace(l), amg.near_nullspace(l + 1), amg.aggregates(l)
            omega = 4.0 / (3.0 * case.lam[l])
            rhs = B - omega * (ref.inverse_diagonal(A)[:, None] * (A @ B))
            eI = float(np.abs((P @ Bn - rhs)[agg >= 0]).max() / np.abs(B).max())
            print(msg + "  P %.2e  P B_c = (I - w D^-1 A) B %.2e  lambda_max %.6f" % (eP, eI, case.lam[l]))
            assert eP <= TOL and eI <= TOL
            assert np.diff(P.indptr)[agg < 0].max(initial=0) == 0
            rows = ref.rows_of(amg.level_matrix(l + 1))
            Ac, dead = amg.level_matrix(l + 1), amg.dead(l).astype(bool)
            offdiag = (rows != Ac.indices) & (dead[rows] | dead[Ac.indices])
            assert not Ac.data[offdiag].any() and (Ac.diagonal()[dead] == 1.0).all()     # dead coarse dofs are decoupled, with a unit diagonal


# ------------------------------------------------------------------------------------------------ 5. reproducibility
def test_setups_replan_and_applies_give_the_same_bits(case, device):
    amg = case.amg
    snap = lambda: ([amg.level_matrix(l).data.copy() for l in range(case.nl)], [amg.prolongator(l).data.copy() for l in range(case.nl - 1)],
                    [amg.tentative(l).data.copy() for l in range(case.nl - 1)], [amg.near_nullspace(l).copy() for l in range(case.nl)])
    same = lambda a, b: all(np.array_equal(x, y) for u, v in zip(a, b) for x, y in zip(u, v))
    r = device.to_device(case.b)
    before, z1 = snap(), amg.apply(r, device.zeros(len(case.b))).to_host()
    amg.setup(case.dA)
    assert same(before, snap()) and [amg.lambda_max(l) for l in range(case.nl - 1)] == case.lam
    z2 = amg.apply(r, device.zeros(len(case.b))).to_host()
    amg.replan()
    amg.setup(case.dA)
    assert amg.n_levels == case.nl and same(before, snap())
    z3 = amg.apply(r, device.zeros(len(case.b))).to_host()
    assert np.array_equal(z1, z2) and np.array_equal(z1, z3)
    z4 = device.zeros(len(case.b))
    graph = device.capture(lambda: amg.apply(r, z4))
    graph.launch()
    device.synchronize()
    assert np.array_equal(z1, z4.to_host()) and np.abs(z1).max() > 0.0
    graph.close()


# ------------------------------------------------------------------------------------------------ 6. cycle
def test_cycle(case, device):
    n = len(case.b)
    rng = np.random.default_rng(7)
    u, v = rng.normal(size=n), rng.normal(size=n)
    u[case.ch.prescribed_dofs] = 0.0
    v[case.ch.prescribed_dofs] = 0.0
    mu = case.amg.apply(device.to_device(u), device.zeros(n)).to_host()
    mv = case.amg.apply(device.to_device(v), device.zeros(n)).to_host()
    asym = abs(mu @ v - u @ mv) / abs(mu @ v)
    z = case.amg.apply(device.to_device(case.b), device.zeros(n)).to_host()
    err = relmax(z, ref.vcycle(case.levels, case.b, DEGREE, RATIO))
    print("%s: asymmetry %.2e, <Mu, u> %.3e, one V-cycle against the restatement %.2e" % (case.name, asym, mu @ u, err))
    assert asym <= 1e-12 and mu @ u > 0.0 and mv @ v > 0.0
    assert (mu[case.ch.prescribed_dofs] == 0.0).all()
    assert err <= 1e-12


# ------------------------------------------------------------------------------------------------ 7. iteration counts
def test_pcg_count_matches_the_restatement(tb, case, device):
    n = len(case.b)
    b, x = device.to_device(case.b), device.zeros(n)
    it, res = tb.pcg_solve(case.pattern, case.dA, b, x, rtol=1e-8, atol=0.0, maxiter=500, precond=case.amg)
    xr, itr, resr = ref.pcg(case.A, case.b, lambda r: ref.vcycle(case.levels, r, DEGREE, RATIO), rtol=1e-8)
    true_res = np.linalg.norm(case.b - case.A @ x.to_host())
    line = "%s: rigid-body AMG-PCG %d iterations (restatement %d); residual %.3e (true %.3e)" % (case.name, it, itr, res, true_res)
    assert abs(it - itr) <= 2, line
    assert true_res <= 1.01e-8 * np.linalg.norm(case.b) + 1e-14 and relmax(x.to_host(), xr) <= 1e-6
    if case.name == "beam":
        xs = device.zeros(n)
        its, _ = tb.pcg_solve(case.pattern, case.dA, b, xs, rtol=1e-8, atol=0.0, maxiter=500, precond=tb.AMGPrecon(max_coarse=MAX_COARSE))
        line += "; AMGPrecon() on the same system %d" % its
        print(line)
        assert it < its
    else:
        print(line)


# ------------------------------------------------------------------------------------------------ 8. protocol callers
def test_protocol_callers(tb, device):
    case = get_case(tb, device, "cube")
    n = len(case.b)
    recipe = tb.AMGPrecon(max_coarse=MAX_COARSE, near_nullspace="rigid_body")
    x1, x2 = device.zeros(n), device.zeros(n)
    it1, _ = tb.pcg_solve(case.pattern, case.dA, device.to_device(case.b), x1, rtol=1e-8, atol=0.0, precond=recipe)
    it2, _ = tb.KrylovMGSolver("cg", recipe, rtol=1e-8, atol=0.0).solve(case.pattern, case.dA, device.to_device(case.b), x2, case.ch)
    assert it1 == it2 and 0 < it1 < 30 and np.array_equal(x1.to_host(), x2.to_host())
    mg = recipe.materialize(case.pattern, case.ch)
    assert mg is recipe.materialize(case.pattern) and mg.n_levels == case.nl and mg.k == 6
    # the user's own candidates on the same node blocks: the translations alone
    own = tb.AMGPrecon(max_coarse=MAX_COARSE, near_nullspace=case.B[:, :3].copy()).materialize(case.pattern, case.ch)
    own.setup(case.dA)
    assert own.near_nullspace(0).shape == (n, 3) and own.level_size(0)[2] == 3 * (case.amg.level_size(0)[2] // 6)
    x3 = device.zeros(n)
    it3, _ = tb.pcg_solve(case.pattern, case.dA, device.to_device(case.b), x3, rtol=1e-8, atol=0.0, precond=own)
    print("cube: rigid-body modes %d iterations, translations on node blocks %d" % (it1, it3))
    assert relmax(x3.to_host(), x1.to_host()) <= 1e-6


def bent_beam(tb, device, precond):
    grid = tb.generate_mesh(tb.Hexahedron, (8, 2, 2), (0, 0, 0), (4, 1, 1))
    dh = tb.DofHandler(grid, tb.LagrangeCollection(1) ** 3)
    sp = tb.allocate_matrix(dh)
    X, comp = tb.dof_coordinates(dh), tb.amg.component_labels(dh)
    pres = {int(d): 0.0 for d in np.flatnonzero(np.abs(X[:, 0]) < 1e-12)}
    pres.update({int(d): 0.05 for d in np.flatnonzero((np.abs(X[:, 0] - 4.0) < 1e-12) & (comp == 2))})          # the free end is pushed sideways
    dofs = np.array(sorted(pres))
    ch = tb.ConstraintHandler(dh, dofs, np.array([pres[d] for d in dofs]))
    op = tb.setup_operator(tb.ElementAssemblyStrategy(device), material(tb), dh, sp)
    u = device.zeros(dh.ndofs)
    tb.apply(u, ch)
    solver = tb.NewtonRaphsonSolver(max_iter=20, tol=1e-9, inner_rtol=1e-8, inner_solver="cg", inner_precond=precond, inner_maxiter=5000)
    ok = tb.nlsolve(u, op, ch, solver)
    return ok, u.to_host(), solver


def test_newton_on_the_bent_beam_reaches_the_jacobi_solution(tb, device):
    ok1, u1, s1 = bent_beam(tb, device, tb.AMGPrecon(max_coarse=MAX_COARSE, near_nullspace="rigid_body"))
    ok2, u2, s2 = bent_beam(tb, device, None)
    print("bent beam: Newton %d / %d iterations, linear iterations rigid-body AMG %s, Jacobi %s, difference %.2e" % (
        s1.iter, s2.iter, list(s1.linear_iters), list(s2.linear_iters), np.abs(u1 - u2).max()))
    assert ok1 and ok2
    assert np.abs(u1 - u2).max() <= 1e-6 * np.abs(u2).max()        # Newton tolerance 1e-9 on the residual, inner rtol 1e-8: the iterates agree far below 1e-6
    assert sum(s1.linear_iters) < sum(s2.linear_iters)


def solve_against_direct(tb, device, mg, dh, pattern, dA, ch):
    mg.setup(dA)
    inner = mg.coarse_hierarchy()
    k = C.c_int()
    tb.check(tb.lib().tb_amg_level_near_nullspace(inner.h, 0, C.byref(k), None))
    assert inner is not None and inner.n_levels >= 2 and k.value == 6 and inner.k == 6
    r = np.random.default_rng(23).normal(size=dh.ndofs)
    r[ch.prescribed_dofs] = 0.0
    x = device.zeros(dh.ndofs)
    it, res = mg.solve(dA, device.to_device(r), x, rtol=1e-10, atol=0.0, maxiter=200)
    A = csr_of(pattern.sp, dA.to_host())
    want = np.linalg.solve(A.toarray(), r)
    print("%d levels over %d AMG levels with rigid-body modes: %d iterations, against the direct solve %.2e" % (mg.n_levels, inner.n_levels, it, relmax(x.to_host(), want)))
    assert it < 60 and relmax(x.to_host(), want) <= 1e-7
    return inner


def test_p_level_over_rigid_body_amg(tb, device):
    """ChainedMGPrecon(PMGPrecon(), AMGPrecon(near_nullspace="rigid_body")) on a 4³-cell second-order box: the AMG sits on the Q1 level"""
    dh = tb.DofHandler(tb.generate_mesh(tb.Hexahedron, (4, 4, 4), (0, 0, 0), (1, 1, 1), perturb=0.1), tb.LagrangeCollection(2) ** 3)
    sp = tb.allocate_matrix(dh)
    pres = face_dofs(tb, dh)
    op = tangent(tb, device, dh, sp, pres)
    ch = tb.ConstraintHandler(dh, pres)
    dA = device.to_device(op.J.to_host())
    tb.apply_zero(dA, None, ch, pattern=op.pattern)
    mg = tb.ChainedMGPrecon(tb.PMGPrecon(), tb.AMGPrecon(max_coarse=MAX_COARSE, near_nullspace="rigid_body")).materialize(op.pattern, ch)
    inner = solve_against_direct(tb, device, mg, dh, op.pattern, dA, ch)
    assert inner.level_size(0)[0] == 375


def test_geometric_levels_over_rigid_body_amg(tb, device):
    gh = tb.GridHierarchy(tb.generate_mesh(tb.Hexahedron, (4, 4, 4), (0, 0, 0), (1, 1, 1)), 1)
    dh = tb.DofHandler(gh.grids[-1], tb.LagrangeCollection(1) ** 3)
    sp = tb.allocate_matrix(dh)
    pres = face_dofs(tb, dh)
    op = tangent(tb, device, dh, sp, pres)
    ch = tb.ConstraintHandler(dh, pres)
    dA = device.to_device(op.J.to_host())
    tb.apply_zero(dA, None, ch, pattern=op.pattern)
    mg = tb.GMGPrecon(gh, coarse=tb.AMGPrecon(max_coarse=MAX_COARSE, near_nullspace="rigid_body")).materialize(op.pattern, ch)
    inner = solve_against_direct(tb, device, mg, dh, op.pattern, dA, ch)
    assert inner.level_size(0)[0] == 375


# ------------------------------------------------------------------------------------------------ 9. refusals
def test_refusals(tb, device):
    L, lib = tb._lib, tb.lib()
    case = get_case(tb, device, "cube")
    n, nn = case.dh.ndofs, case.n_nodes
    fresh = lambda: tb.AMGPrecon(max_coarse=MAX_COARSE).materialize(case.pattern)
    i32, dp = lambda a: a.ctypes.data_as(L.c_i32p), lambda a: a.ctypes.data_as(L.c_dp)

    def refused(node, k, B, text):
        h = fresh()
        rc = lib.tb_amg_set_near_nullspace(h.h, nn, i32(node), k, dp(B))
        msg = lib.tb_last_error_string()
        assert rc == L.TB_ERR_BAD_ARG and text in msg, (rc, msg)
        h.close()

    B7 = np.ones((n, 7))
    refused(case.node, 7, B7, b"1 to 6")
    refused(case.node, 0, B7, b"1 to 6")
    two = case.node.copy()
    two[0] = case.node[3]
    refused(two, 6, case.B, b"dofs, not 3")
    far = case.node.copy()
    far[5] = nn
    refused(far, 6, case.B, b"outside")
    nan = case.B.copy()
    nan[7, 4] = np.inf
    refused(case.node, 6, nan, b"non-finite")
    # a change after a set-up needs replan()
    with pytest.raises(L.TBError, match="replan"):
        case.amg.set_near_nullspace(nn, case.node, case.B[:, :3].copy())
    # inspectors of the near-null-space on a scalar hierarchy
    plain = fresh()
    plain.setup(case.dA)
    with pytest.raises(L.TBError, match="near-null-space"):
        plain.tentative(0)
    plain.close()
    # the recipes
    scalar_dh = tb.DofHandler(case.dh.grid)
    with pytest.raises(ValueError, match="3-component"):
        tb.AMGPrecon(near_nullspace="rigid_body").materialize(scalar_dh.device_mesh(device).pattern(tb.allocate_matrix(scalar_dh)))
    q2 = tb.DofHandler(case.dh.grid, tb.LagrangeCollection(2) ** 3)
    with pytest.raises(ValueError, match="PMGPrecon"):
        tb.AMGPrecon(near_nullspace="rigid_body").materialize(q2.device_mesh(device).pattern(tb.allocate_matrix(q2)))
    with pytest.raises(NotImplementedError, match="near_nullspace"):
        tb.BidomainAMGPrecon(near_nullspace="rigid_body")
    D = tb.ConstantCoefficient(np.eye(3))
    gh = tb.GridHierarchy(tb.generate_mesh(tb.Hexahedron, (2, 2, 2), (0, 0, 0), (1, 1, 1)), 1)
    with pytest.raises(NotImplementedError, match="near_nullspace"):
        tb.BidomainBackwardEulerStage(tb.BackwardEulerSolver(), tb.PerColorAssemblyStrategy(device), tb.DofHandler(gh.grids[-1]), D, D, [0],
                                      precond=tb.GMGPrecon(gh, coarse=tb.AMGPrecon(near_nullspace="rigid_body")))
    mg = C.c_void_p()
    tb.check(lib.tb_mg_create(device.h, 2, C.byref(mg)))
    assert lib.tb_mg_set_coarse_amg_near_nullspace(mg, nn, i32(case.node), 6, dp(case.B)) == L.TB_ERR_BAD_ARG and b"tb_mg_set_coarse_amg" in lib.tb_last_error_string()
    lib.tb_mg_destroy(mg)


# ------------------------------------------------------------------------------------------------ 10. unchanged default
@pytest.mark.parametrize("name", parent_bits.SYSTEMS)
def test_the_scalar_method_keeps_the_parents_bits(tb, device, name):
    gold = dict(np.load(GOLDEN))
    got = parent_bits.scalar_bits(tb, device, name)
    want = {k: v for k, v in gold.items() if k.startswith(name + ".")}
    assert np.array_equal(got[name + ".input.sha256"], want[name + ".input.sha256"]), "the rounded input differs: the comparison below would be of two matrices"
    differ = [k for k in sorted(set(got) | set(want)) if k not in got or k not in want or got[k].dtype != want[k].dtype or not np.array_equal(got[k], want[k])]
    print("%s: %d arrays, differing: %s" % (name, len(want), differ or "none"))
    assert len(want) > 0 and not differ
