"""Multigrid-preconditioned GMRES on the device (tb_gmres_solve_mg, tb_gmres_solve_amg; general mode of the hierarchies) against the extended-precision
recurrence of tests/gmres_mg_reference.py, whose M⁻¹ is the hierarchy's own `apply` on the double-rounded vector.

Matrices: the assembled M + K of the mesh (scalar: mass plus the diffusion form; three components: vector mass plus a Holzapfel–Ogden tangent at a small
displacement), Dirichlet rows eliminated, plus the seeded skew term A_ij += 0.1·σ_ij·√(A_ii A_jj) on the stored pattern (σ antisymmetric in [−1, 1],
eliminated rows untouched); the diagonal is checked positive on the host.

Largest ratio deviation / tolerance of an iterate per hierarchy kind over k ∈ {1, 2, 3, 5} and restart ∈ {3, 30}, tolerance 16·max(ε_ref, 2⁻⁵⁰) with
ε_ref from the two float64 orders of the reference, measured on an MI355X (two runs, the larger figure; the test prints every ratio):
    gmg2    2-level GMGPrecon,  125 dofs                              0.03
    gmg3    3-level GMGPrecon,  729 dofs                              0.06
    gmg3v   3-level GMGPrecon, 3 components, 2 187 dofs               0.03
    amg     AMGPrecon(max_coarse=32), tetrahedra, 216 dofs, 2 levels  0.04
    amg_rb  rigid-body AMGPrecon, tetrahedra, 375 dofs, 3 levels      0.04
The deviations themselves are 1e-16 … 1e-15 of the iterate: ε_ref stays under its floor 2⁻⁵⁰ in all but three cells, so the tolerance is 1.42e-14
almost everywhere.  restart = 1, k = 3: 0.01.  The two-level cycle against its restatement: 0.01 in either mode.  Pivoted inverse: error 3.3e-16
against numpy.linalg.solve's 4.3e-16 (ratio 0.77 of the allowed 16); the unpivoted default mode on that matrix: 0.48."""
import ctypes as C

import numpy as np
import pytest

import amg_reference as aref
import gmres_mg_reference as gref
import krylov_reference as kr
from gmg_case import face_dofs, heat_values

pytestmark = pytest.mark.gpu
LD = np.longdouble
KS, RESTARTS = (1, 2, 3, 5), (3, 30)
KINDS = ("gmg2", "gmg3", "gmg3v", "amg", "amg_rb")
MAX_COARSE = 32
S = 0.1


def box(tb, kind, nel):
    return tb.generate_mesh(kind, nel, (0, 0, 0), (1, 1, 1))


def ho_model(tb, facets=()):
    ms = tb.ConstantCoefficient(tb.OrthotropicMicrostructure(*np.eye(3)))
    return tb.QuasiStaticModel("d", tb.PK1Model(tb.HolzapfelOgden2009Model(a=1.0, b=1.0, af=0.0, as_=0.0, afs=0.0, beta=1.0), ms), list(facets))


def assembled(tb, device, dh, sp, pres):
    """M + K on the host and the pattern: scalar M − K_diffusion (the diffusion form is negative semidefinite); 3 components: vector mass + the tangent
    of the Holzapfel–Ogden energy at a small random displacement that vanishes at the prescribed dofs"""
    if dh.ip.ncomp == 1:
        vals, pattern = heat_values(tb, device, dh, sp, tb.ConstantCoefficient(np.diag([9.0, 4.0, 4.0])), dt=1.0)
        return vals, pattern, None
    op = tb.setup_operator(tb.ElementAssemblyStrategy(device), ho_model(tb), dh, sp)
    u = np.random.default_rng(5).uniform(-5e-3, 5e-3, dh.ndofs)
    u[pres] = 0.0
    tb.update_linearization(op, device.to_device(u), 0.0, residual=device.zeros(dh.ndofs))
    M = tb.update_operator(tb.setup_operator(tb.PerColorAssemblyStrategy(device), tb.BilinearMassIntegrator(tb.ConstantCoefficient(1.0)), dh, sp), 0.0)
    return op.J.to_host() + M.A.to_host(), op.pattern, op


class Case:
    """one skewed system on the device and its hierarchy in general mode, set up once"""

    def __init__(self, tb, device, kind, skew=S):
        self.kind = kind
        ncomp = 3 if kind in ("gmg3v", "amg_rb") else 1
        if kind.startswith("gmg"):
            self.gh = tb.GridHierarchy(box(tb, tb.Hexahedron, (2, 2, 2)), 1 if kind == "gmg2" else 2)
            grid = self.gh.grids[-1]
        else:
            self.gh = None
            grid = box(tb, tb.Tetrahedron, (4, 4, 4) if kind == "amg_rb" else (5, 5, 5))
        dh = tb.DofHandler(grid, tb.LagrangeCollection(1, ncomp))
        sp = tb.allocate_matrix(dh)
        pres = face_dofs(tb, dh)
        vals, pattern, self.keep = assembled(tb, device, dh, sp, pres)
        self.dh, self.sp, self.pattern, self.n = dh, sp, pattern, dh.ndofs
        self.ch = tb.ConstraintHandler(dh, pres)
        dA = device.to_device(vals)
        tb.apply_zero(dA, None, self.ch, pattern=pattern)
        sym = dA.to_host()
        rows = np.repeat(np.arange(self.n), np.diff(sp.rowptr))
        assert (sym[rows == sp.colidx] > 0).all(), "the hierarchy needs a positive diagonal"
        self.sym = sym
        self.vals = gref.skewed(sp.rowptr, sp.colidx, sym, 100 + KINDS.index(kind) if kind in KINDS else 99, s=skew, untouched=pres) if skew else sym
        assert (self.vals[rows == sp.colidx] > 0).all()
        self.dA = device.to_device(self.vals)
        if kind.startswith("gmg"):
            self.recipe = tb.GMGPrecon(self.gh)
        elif kind == "amg":
            self.recipe = tb.AMGPrecon(max_coarse=MAX_COARSE)
        else:
            self.recipe = tb.AMGPrecon(max_coarse=MAX_COARSE, near_nullspace="rigid_body")
        self.mg = self.recipe.materialize(pattern, self.ch)
        self.mg.set_general(True)
        self.mg.setup(self.dA)
        rng = np.random.default_rng(17)
        self.b = rng.normal(size=self.n)
        self.b[pres] = 0.0
        self.xrand = rng.normal(size=self.n)
        self.xrand[pres] = 0.0
        self.device, self.z = device, device.zeros(self.n)
        self._refs = {}

    def apply_M(self, v):
        """the hierarchy's own cycle on the double-rounded vector"""
        return self.mg.apply(self.device.to_device(np.asarray(v, dtype=np.float64)), self.z).to_host()

    def x0(self, restart):
        return np.zeros(self.n) if restart == 3 else self.xrand

    def reference(self, restart, kmax=max(KS)):
        if (restart, kmax) not in self._refs:
            self._refs[restart, kmax] = gref.Reference(self.sp.rowptr, self.sp.colidx, self.vals, self.apply_M, self.b, self.x0(restart), kmax, restart)
        return self._refs[restart, kmax]

    def solve(self, x0, rtol, atol, maxiter, restart, b=None):
        x = self.device.to_device(x0)
        it, res = self.mg.solve_gmres(self.dA, self.device.to_device(self.b if b is None else b), x, rtol=rtol, atol=atol, maxiter=maxiter, restart=restart, setup=False)
        return x.to_host(), it, res

    def last_tolerance(self, tb):
        tol = C.c_double()
        tb.check(tb.lib().tb_solver_last_tolerance(self.pattern.h, C.byref(tol)))
        return tol.value

    def residual_bound(self, x, b=None):
        """4·(maxrow + 2)·2⁻⁵³·‖ |A||x| + |b| ‖₂: the rounding bound of a residual computed in double"""
        b = self.b if b is None else b
        absAx = kr.csr_matvec(self.sp.rowptr, self.sp.colidx, np.abs(self.vals), np.abs(x))
        return float(4 * (gref.max_row_entries(self.sp.rowptr) + 2) * 2.0 ** -53 * np.sqrt(np.sum((absAx + np.abs(b).astype(LD)) ** 2)))

    def true_residual(self, x, b=None):
        b = self.b if b is None else b
        r = b.astype(LD) - kr.csr_matvec(self.sp.rowptr, self.sp.colidx, self.vals, x)
        return float(np.sqrt(np.sum(r * r)))


_cases = {}


def get_case(tb, device, kind):
    if kind not in _cases:
        _cases[kind] = Case(tb, device, kind)
    return _cases[kind]


# ------------------------------------------------------------------------------------------------ 1. iterates
@pytest.mark.parametrize("restart", RESTARTS)
@pytest.mark.parametrize("kind", KINDS)
def test_iterates_follow_the_reference(tb, device, kind, restart):
    case = get_case(tb, device, kind)
    assert {"gmg2": 125, "gmg3": 729, "gmg3v": 2187}.get(kind, case.n) == case.n and case.mg.general
    ref = case.reference(restart)
    x0 = case.x0(restart)
    worst = 0.0
    for k in KS:
        x, it, res = case.solve(x0, 0.0, 0.0, k, restart)
        assert it == k
        dev, tol = kr.deviation(x - x0, ref.dx(k)), ref.tol_x(k)
        rdev, rtol = kr.relative(res, ref.ld["res"][k]), ref.tol_scalar("res", k)
        worst = max(worst, dev / tol)
        print("%s (%d dofs, %d levels) restart %d k %d: iterate deviates %.2e, tolerance %.2e, ratio %.2f; residual %.6e deviates %.2e (tolerance %.2e)"
              % (kind, case.n, case.mg.n_levels, restart, k, dev, tol, dev / tol, res, rdev, rtol))
        assert dev <= tol and rdev <= rtol
    print("%s restart %d: largest ratio %.2f" % (kind, restart, worst))


# ------------------------------------------------------------------------------------------------ 2. edges
def test_maxiter_zero_leaves_x_and_returns_the_initial_residual(tb, device):
    case = get_case(tb, device, "gmg2")
    x, it, res = case.solve(case.xrand, 1e-8, 0.0, 0, 30)
    want = case.true_residual(case.xrand)
    print("maxiter 0: residual %.17g, host %.17g" % (res, want))
    assert it == 0 and np.array_equal(x, case.xrand)
    assert abs(res - want) <= case.residual_bound(case.xrand)
    assert not tb.solve_converged(case.pattern, res)


def test_a_solved_system_takes_no_iteration(tb, device):
    case = get_case(tb, device, "gmg2")
    xs = case.xrand
    b = kr.csr_matvec(case.sp.rowptr, case.sp.colidx, case.vals, xs).astype(np.float64)
    atol = 1e-10 * float(np.linalg.norm(b))
    x, it, res = case.solve(xs, 0.0, atol, 50, 30, b=b)
    print("x0 = solution: %d iterations, residual %.3e (threshold %.3e)" % (it, res, atol))
    assert it == 0 and np.array_equal(x, xs) and res <= atol and tb.solve_converged(case.pattern, res)


def test_restart_one_runs_and_follows_the_reference(tb, device):
    case = get_case(tb, device, "gmg2")
    x0 = case.xrand
    ref = gref.Reference(case.sp.rowptr, case.sp.colidx, case.vals, case.apply_M, case.b, x0, 3, 1)
    x, it, res = case.solve(x0, 0.0, 0.0, 3, 1)
    dev, tol = kr.deviation(x - x0, ref.dx(3)), ref.tol_x(3)
    print("restart 1, k 3: iterate deviates %.2e, tolerance %.2e, ratio %.2f" % (dev, tol, dev / tol))
    assert it == 3 and dev <= tol


def test_iteration_count_and_last_tolerance(tb, device):
    """the solve stops at the first Arnoldi step whose estimate meets the threshold: rtol sits a factor ≥ 4 below the reference's estimate at step
    j − 1 and a factor ≥ 4 above the one at step j, so rounding cannot move the count"""
    case = get_case(tb, device, "gmg2")
    x0 = np.zeros(case.n)
    ref = gref.Reference(case.sp.rowptr, case.sp.colidx, case.vals, case.apply_M, case.b, x0, 10, 30)
    est = [float(e) for e in ref.ld["est"]]
    print("estimates of the reference: %s" % " ".join("%.3e" % e for e in est))
    j = max((i for i in range(2, 11) if est[i] > 1e-10 * est[0]), key=lambda i: est[i - 1] / est[i])    # (above the level where rounding takes over)
    thr = np.sqrt(est[j - 1] * est[j])
    rtol = thr / est[0]
    assert est[j - 1] >= 4 * thr and 4 * est[j] <= thr and all(e > thr for e in est[:j]), (j, est)
    x, it, res = case.solve(x0, rtol, 0.0, 50, 30)
    tol = case.last_tolerance(tb)
    _, _, res0 = case.solve(x0, rtol, 0.0, 0, 30)
    print("rtol %.3e: %d iterations (reference %d), residual %.3e, threshold %.17g" % (rtol, it, j, res, tol))
    assert it == j
    assert tol == 0.0 + rtol * res0                           # atol + rtol·‖r₀‖ with the solver's own ‖r₀‖
    assert abs(res - float(ref.ld["res"][j])) <= 1e-6 * float(ref.ld["res"][j]) and res <= tol and tb.solve_converged(case.pattern, res)
    # with an absolute part
    _, it2, res2 = case.solve(x0, 0.0, thr, 50, 30)
    assert it2 == j and case.last_tolerance(tb) == thr


def test_nan_in_b_returns_at_once_unconverged(tb, device):
    case = get_case(tb, device, "gmg2")
    b = case.b.copy()
    b[case.n // 2] = np.nan
    x, it, res = case.solve(case.xrand, 1e-8, 1e-12, 50, 30, b=b)
    assert it == 0 and np.isnan(res) and np.array_equal(x, case.xrand)
    assert np.isnan(case.last_tolerance(tb)) and not tb.solve_converged(case.pattern, res)


def test_solve_entries_check_the_hierarchy(tb, device):
    L, lib = tb._lib, tb.lib()
    case = get_case(tb, device, "gmg2")
    other = get_case(tb, device, "amg")
    it, v = C.c_int(), C.c_double()
    x, b = device.zeros(case.n), device.to_device(case.b)
    args = (1e-8, 0.0, 10)
    assert lib.tb_gmres_solve_mg(case.pattern.h, case.dA.ptr, b.ptr, x.ptr, *args, 0, case.mg.h, C.byref(it), C.byref(v)) == L.TB_ERR_BAD_ARG
    assert b"restart" in lib.tb_last_error_string()
    assert lib.tb_gmres_solve_mg(other.pattern.h, case.dA.ptr, b.ptr, x.ptr, *args, 5, case.mg.h, C.byref(it), C.byref(v)) == L.TB_ERR_BAD_ARG
    assert b"finest level" in lib.tb_last_error_string()
    copy = device.to_device(case.vals)
    assert lib.tb_gmres_solve_mg(case.pattern.h, copy.ptr, b.ptr, x.ptr, *args, 5, case.mg.h, C.byref(it), C.byref(v)) == L.TB_ERR_BAD_ARG
    assert b"another matrix array" in lib.tb_last_error_string()
    assert lib.tb_gmres_solve_amg(case.pattern.h, other.dA.ptr, b.ptr, x.ptr, *args, 5, other.mg.h, C.byref(it), C.byref(v)) == L.TB_ERR_BAD_ARG
    assert b"another pattern" in lib.tb_last_error_string()


# ------------------------------------------------------------------------------------------------ 3. convergence
def test_solve_converges_and_reports_the_true_residual(tb, device):
    case = get_case(tb, device, "gmg3")
    x, it, res = case.solve(np.zeros(case.n), 1e-8, 0.0, 200, 30)
    true, bound = case.true_residual(x), case.residual_bound(x)
    xj = device.zeros(case.n)
    itj, resj = tb.gmres_solve(case.pattern, case.dA, device.to_device(case.b), xj, rtol=1e-8, atol=0.0, maxiter=2000, restart=30)
    print("729 dofs: multigrid-GMRES(30) %d steps (Jacobi-GMRES(30) %d), residual %.6e, host %.6e, difference %.2e, bound %.2e" % (it, itj, res, true, abs(res - true), bound))
    assert tb.gmres_solve is not None and tb.solve_converged(case.pattern, resj)
    x2 = device.zeros(case.n)
    it2, res2 = tb.gmres_solve(case.pattern, case.dA, device.to_device(case.b), x2, rtol=1e-8, atol=0.0, maxiter=200, restart=30, precond=case.mg)
    assert tb.solve_converged(case.pattern, res2) and it2 == it and kr.deviation(x2.to_host(), x) <= 1e-9  # the public route is the same solve (sums of several workgroups: not the same bits)
    assert res <= 1e-8 * float(np.linalg.norm(case.b)) and abs(res - true) <= bound
    assert it < itj


# ------------------------------------------------------------------------------------------------ 4. pivoted inverse
def pivot_matrix(sp, zero=None):
    """non-symmetric on the pattern: diagonal 1, the first three diagonal entries 1e-12, off-diagonals N(0, 0.05²) — but O(1) couplings between the
    first three dofs and their neighbours, which keep the matrix well conditioned although its leading pivots are useless.  zero: a dof whose row and
    column are exactly zero"""
    n = len(sp.rowptr) - 1
    rows = np.repeat(np.arange(n), np.diff(sp.rowptr))
    cols = sp.colidx.astype(np.int64)
    rng = np.random.default_rng(41)
    v = 0.05 * rng.normal(size=len(cols))
    near = ((rows < 3) | (cols < 3)) & (rows != cols)
    v[near] = rng.uniform(0.5, 1.0, size=near.sum()) * rng.choice([-1.0, 1.0], size=near.sum())
    v[rows == cols] = np.where(np.arange(n) < 3, 1e-12, 1.0)
    if zero is not None:
        v[(rows == zero) | (cols == zero)] = 0.0
    return v


def single_level(tb, device):
    dh = tb.DofHandler(box(tb, tb.Hexahedron, (4, 4, 4)))
    sp = tb.allocate_matrix(dh)
    pattern = dh.device_mesh(device).pattern(sp)
    return dh, sp, pattern


def longdouble_solve(A, r):
    """A⁻¹ r to extended precision: the float64 LU solve refined with residuals in longdouble (cond₂ ≤ 1e4: every pass gains twelve digits)"""
    x = np.linalg.solve(A, r).astype(LD)
    for _ in range(4):
        x = x + np.linalg.solve(A, (r.astype(LD) - A.astype(LD) @ x).astype(np.float64)).astype(LD)
    return x


def test_pivoted_inverse(tb, device):
    dh, sp, pattern = single_level(tb, device)
    vals = pivot_matrix(sp)
    A = gref.dense(sp.rowptr, sp.colidx, vals)
    cond = np.linalg.cond(A)
    print("125 dofs, first three diagonal entries 1e-12: cond2 = %.3e, asymmetry %.2f" % (cond, np.abs(A - A.T).max() / np.abs(A).max()))
    assert dh.ndofs == 125 and cond <= 1e4 and np.abs(A - A.T).max() > 0.1
    dA = device.to_device(vals)
    amg = tb.AMGPrecon().materialize(pattern)
    amg.set_general(True).setup(dA)
    assert amg.n_levels == 1                                  # the cycle is the dense inverse
    r = np.random.default_rng(43).normal(size=125)
    z1 = amg.apply(device.to_device(r), device.zeros(125)).to_host()
    amg.setup(dA)
    z2 = amg.apply(device.to_device(r), device.zeros(125)).to_host()
    want = longdouble_solve(A, r)
    err = kr.deviation(z1, want)
    err_np = kr.deviation(np.linalg.solve(A, r), want)
    print("pivoted inverse: error %.3e, numpy.linalg.solve %.3e, ratio %.2f" % (err, err_np, err / err_np))
    assert np.array_equal(z1, z2), "two set-ups differ"
    assert err <= 16 * err_np
    # the unpivoted inverse of the default mode is of no use on this matrix: the flag is what makes the difference
    amg.set_general(False).setup(dA)
    z0 = amg.apply(device.to_device(r), device.zeros(125)).to_host()
    print("default mode on the same matrix: error %.3e" % kr.deviation(z0, want))
    assert not kr.deviation(z0, want) <= 16 * err_np


def test_zero_pivot_is_an_error_return(tb, device):
    dh, sp, pattern = single_level(tb, device)
    dA = device.to_device(pivot_matrix(sp, zero=60))
    amg = tb.AMGPrecon().materialize(pattern)
    amg.set_general(True)
    with pytest.raises(tb.TBError, match="tb_amg_setup.*level 0") as e:
        amg.setup(dA)
    print(str(e.value))
    assert e.value.code == tb._lib.TB_ERR_BAD_ARG
    assert tb.lib().tb_amg_apply(amg.h, device.zeros(125).ptr, device.zeros(125).ptr) == tb._lib.TB_ERR_BAD_ARG      # no numeric phase
    amg.setup(device.to_device(pivot_matrix(sp)))             # the hierarchy is usable again


# ------------------------------------------------------------------------------------------------ 5. the flag through a hierarchy
def two_level_cycle(A0, A1inv, P, lam, r, dtype, reverse):
    """V(2, 2) of a two-level hierarchy from the accessors' matrices, in `dtype`; reverse: every product summed from the last column to the first"""
    c = lambda a: np.asarray(a).astype(dtype)                 # noqa: E731

    class Mat:
        def __init__(self, M):
            self.M = c(M)[:, ::-1].copy() if reverse else c(M)

        def __matmul__(self, x):
            return self.M @ (x[::-1] if reverse else x)
    A, Pm, Pt, Ci = Mat(A0), Mat(P), Mat(P.T), Mat(A1inv)
    dinv = 1 / c(np.diag(A0))                                 # (the diagonal is positive)
    r = c(r)
    x = aref.chebyshev(A, dinv, dtype(lam), dtype(4.0), 2, r)
    x = x + Pm @ (Ci @ (Pt @ (r - A @ x)))
    return aref.chebyshev(A, dinv, dtype(lam), dtype(4.0), 2, r, x)


def refined_inverse(A):
    """A⁻¹ in longdouble: two Newton–Schulz steps on the float64 inverse"""
    X, Al = np.linalg.inv(A).astype(LD), A.astype(LD)
    for _ in range(2):
        X = X @ (2 * np.eye(len(A), dtype=LD) - Al @ X)
    return X


def test_flag_through_a_two_level_hierarchy(tb, device):
    case = get_case(tb, device, "amg")
    make = lambda: tb.AMGPrecon(max_coarse=MAX_COARSE, max_levels=2).materialize(case.pattern, case.ch)      # noqa: E731
    amg, untouched = make(), make()
    r = case.b
    dr = device.to_device(r)
    z_plain = untouched.setup(case.dA).apply(dr, device.zeros(case.n)).to_host()                              # never saw the new entry
    out = {}
    for general in (True, False):
        before = amg.n_setups
        amg.set_general(general)
        assert amg._A is None                                  # flipping drops the numeric phase …
        x = device.zeros(case.n)
        (amg.solve_gmres if general else amg.solve)(case.dA, dr, x, rtol=1e-8, atol=0.0, maxiter=5, setup=False)
        assert amg.n_setups == before + 1 and amg.general is general                                          # … and the solve sets up again
        assert amg.n_levels == 2
        A0, A1, P, lam = amg.level_matrix(0).toarray(), amg.level_matrix(1).toarray(), amg.prolongator(0).toarray(), amg.lambda_max(0)
        assert np.abs(A1 - A1.T).max() > 1e-3 * np.abs(A1).max()                                              # the coarse operator is not symmetric either
        inv = refined_inverse(A1)
        Ci = inv if general else (inv + inv.T) / 2
        z = amg.apply(dr, device.zeros(case.n)).to_host()
        ld = two_level_cycle(A0, Ci, P, lam, r, LD, False)
        eps = max(kr.deviation(two_level_cycle(A0, Ci.astype(np.float64), P, lam, r, np.float64, rev), ld) for rev in (False, True))
        dev, tol = kr.deviation(z, ld), kr.tolerance(eps)
        other = two_level_cycle(A0, (inv + inv.T) / 2 if general else inv, P, lam, r, LD, False)
        print("general %d: cycle deviates %.2e from its restatement (tolerance %.2e, ratio %.2f); from the other mode's restatement %.2e"
              % (general, dev, tol, dev / tol, kr.deviation(z, other)))
        assert dev <= tol and kr.deviation(z, other) > 16 * tol
        out[general] = z
    assert np.array_equal(out[False], z_plain), "general = 0 after general = 1 differs from a hierarchy that never saw the flag"
    # CG after GMRES on one hierarchy: the protocol callers flip the flag themselves
    before = amg.n_setups
    amg.reuse_setup = True
    tb.gmres_solve(case.pattern, case.dA, dr, device.zeros(case.n), rtol=1e-6, atol=0.0, precond=amg)
    tb.pcg_solve(case.pattern, case.dA, dr, device.zeros(case.n), rtol=1e-6, atol=0.0, maxiter=3, precond=amg)
    amg.reuse_setup = False
    assert amg.n_setups == before + 2 and not amg.general


def test_set_general_clears_the_numeric_phase_in_the_library(tb, device):
    """tb_*_set_general itself drops `ready` on a change (and only on a change): apply and the solves refuse until the next set-up"""
    L, lib = tb._lib, tb.lib()
    case = get_case(tb, device, "amg")
    it, v = C.c_int(), C.c_double()
    r, z, x = device.to_device(case.b), device.zeros(case.n), device.zeros(case.n)
    amg = tb.AMGPrecon(max_coarse=MAX_COARSE).materialize(case.pattern, case.ch).setup(case.dA)
    assert lib.tb_amg_set_general(amg.h, 0) == L.TB_OK and lib.tb_amg_apply(amg.h, r.ptr, z.ptr) == L.TB_OK           # no change: still set up
    assert lib.tb_amg_set_general(amg.h, 1) == L.TB_OK
    assert lib.tb_amg_apply(amg.h, r.ptr, z.ptr) == L.TB_ERR_BAD_ARG and b"no numeric setup" in lib.tb_last_error_string()
    assert lib.tb_gmres_solve_amg(case.pattern.h, case.dA.ptr, r.ptr, x.ptr, 1e-8, 0.0, 10, 5, amg.h, C.byref(it), C.byref(v)) == L.TB_ERR_BAD_ARG
    assert lib.tb_pcg_solve_amg(case.pattern.h, case.dA.ptr, r.ptr, x.ptr, 1e-8, 0.0, 10, amg.h, C.byref(it), C.byref(v)) == L.TB_ERR_BAD_ARG
    assert lib.tb_amg_setup(amg.h, case.dA.ptr, 2, 4.0) == L.TB_OK and lib.tb_amg_apply(amg.h, r.ptr, z.ptr) == L.TB_OK
    assert lib.tb_amg_set_general(amg.h, 7) == L.TB_OK and lib.tb_amg_apply(amg.h, r.ptr, z.ptr) == L.TB_OK           # any non-zero value is "on": no change
    g = get_case(tb, device, "gmg2")
    rg, zg, xg = device.to_device(g.b), device.zeros(g.n), device.zeros(g.n)
    mg = tb.GMGPrecon(g.gh, coarse=tb.AMGPrecon(max_coarse=8)).materialize(g.pattern, g.ch).setup(g.dA)
    assert not mg.coarse_hierarchy().general
    assert lib.tb_mg_set_general(mg.h, 1) == L.TB_OK
    assert lib.tb_mg_apply(mg.h, rg.ptr, zg.ptr) == L.TB_ERR_BAD_ARG and b"no numeric setup" in lib.tb_last_error_string()
    assert lib.tb_gmres_solve_mg(g.pattern.h, g.dA.ptr, rg.ptr, xg.ptr, 1e-8, 0.0, 10, 5, mg.h, C.byref(it), C.byref(v)) == L.TB_ERR_BAD_ARG
    assert lib.tb_mg_setup(mg.h, g.dA.ptr, 2, 4.0) == L.TB_OK and lib.tb_mg_apply(mg.h, rg.ptr, zg.ptr) == L.TB_OK
    # the Python object, flipped through its own method, hands its mode to the view of the AMG below level 0
    mg2 = tb.GMGPrecon(g.gh, coarse=tb.AMGPrecon(max_coarse=8)).materialize(g.pattern, g.ch)
    mg2.set_general(True).setup(g.dA)                         # the flag precedes the AMG's creation: it is created in general mode
    view = mg2.coarse_hierarchy()
    assert view.general and view.n_setups == 1
    with pytest.raises(RuntimeError, match="MultigridHierarchy"):
        view.set_general(False)
    z1 = mg2.apply(rg, device.zeros(g.n)).to_host()
    assert np.array_equal(z1, zg.to_host())                   # flag before or after the first set-up: the same hierarchy, the same bits


def test_flag_reaches_the_coarse_amg_of_a_geometric_hierarchy(tb, device):
    case = get_case(tb, device, "gmg3")
    mg = tb.GMGPrecon(case.gh, coarse=tb.AMGPrecon(max_coarse=8)).materialize(case.pattern, case.ch)
    x = device.zeros(case.n)
    it, res = tb.gmres_solve(case.pattern, case.dA, device.to_device(case.b), x, rtol=1e-8, atol=0.0, maxiter=200, restart=30, precond=mg)
    assert mg.general and mg.n_setups == 1 and tb.solve_converged(case.pattern, res)
    inner = mg.coarse_hierarchy()
    xg, itg, _ = case.solve(np.zeros(case.n), 1e-8, 0.0, 200, 30)
    print("729 dofs: GMG over AMG (%d AMG levels) %d steps, GMG with the dense inverse %d; solutions differ by %.2e" % (inner.n_levels, it, itg, kr.deviation(x.to_host(), xg)))
    assert inner.n_levels >= 2 and kr.deviation(x.to_host(), xg) <= 1e-6
    # the same through KrylovMGSolver(KrylovGMRES)
    x2 = device.zeros(case.n)
    it2, _ = tb.KrylovMGSolver(tb.KrylovGMRES(restart=30), mg, maxiters=200, rtol=1e-8, atol=0.0).solve(case.pattern, case.dA, device.to_device(case.b), x2, case.ch)
    assert it2 == it and kr.deviation(x2.to_host(), x.to_host()) <= 1e-9


# ------------------------------------------------------------------------------------------------ 6. Newton
def beam(tb, device, cell, inner, precond, pressure):
    """a 4 × 1 × 1 Holzapfel–Ogden beam clamped at x = 0: under a follower pressure on its bottom face (a non-symmetric tangent), or — pressure None —
    with its free end pushed sideways (a symmetric positive definite one)"""
    if cell == "hex":
        gh = tb.GridHierarchy(tb.generate_mesh(tb.Hexahedron, (4, 1, 1), (0, 0, 0), (4, 1, 1)), 1)
        grid = gh.grids[-1]
        precond = precond and tb.GMGPrecon(gh)
    else:
        grid = tb.generate_mesh(tb.Tetrahedron, (8, 2, 2), (0, 0, 0), (4, 1, 1))
        precond = precond and tb.AMGPrecon(max_coarse=MAX_COARSE, near_nullspace="rigid_body")
    dh = tb.DofHandler(grid, tb.LagrangeCollection(1) ** 3)
    sp = tb.allocate_matrix(dh)
    X, comp = tb.dof_coordinates(dh), tb.amg.component_labels(dh)
    pres = {int(d): 0.0 for d in np.flatnonzero(np.abs(X[:, 0]) < 1e-12)}
    if pressure is None:
        pres.update({int(d): 0.05 for d in np.flatnonzero((np.abs(X[:, 0] - 4.0) < 1e-12) & (comp == 2))})
    dofs = np.array(sorted(pres))
    ch = tb.ConstraintHandler(dh, dofs, np.array([pres[d] for d in dofs]))
    load = [] if pressure is None else [tb.PressureFieldBC(tb.ConstantCoefficient(pressure), "bottom")]
    op = tb.setup_operator(tb.ElementAssemblyStrategy(device), ho_model(tb, load), dh, sp)
    u = device.zeros(dh.ndofs)
    tb.apply(u, ch)
    solver = tb.NewtonRaphsonSolver(max_iter=20, tol=1e-9, inner_rtol=1e-8, inner_solver=inner, inner_precond=precond or None, inner_maxiter=5000, gmres_restart=250)
    ok = tb.nlsolve(u, op, ch, solver)
    assert ok, (cell, inner, solver.residual_norms, solver.linear_failure)
    return u.to_host(), solver, precond


@pytest.mark.parametrize("cell", ["tet", "hex"])
def test_newton_under_pressure_with_multigrid_gmres(tb, device, cell):
    u1, s1, recipe = beam(tb, device, cell, "gmres", True, 0.001)
    u2, s2, _ = beam(tb, device, cell, "gmres", False, 0.001)
    hier = next(iter(recipe._materialized.values()))[0]
    print("%s beam under pressure (%d dofs): Newton %d / %d iterations; Arnoldi steps multigrid-GMRES %s = %d, Jacobi-GMRES %s = %d; tip %.4f, difference %.2e"
          % (cell, len(u1), s1.iter, s2.iter, list(s1.linear_iters), sum(s1.linear_iters), list(s2.linear_iters), sum(s2.linear_iters), np.abs(u2).max(),
             np.abs(u1 - u2).max()))
    assert hier.general and hier.n_setups == s1.iter          # GMRES ran on the hierarchy (not CG), one set-up per tangent
    assert np.abs(u1 - u2).max() <= 1e-6 * np.abs(u2).max()   # Newton tolerance 1e-9 on the residual, inner rtol 1e-8: the iterates agree far below 1e-6
    assert sum(s1.linear_iters) < sum(s2.linear_iters)


@pytest.mark.parametrize("cell", ["tet", "hex"])
def test_gmres_and_cg_agree_on_a_symmetric_tangent(tb, device, cell):
    u1, s1, r1 = beam(tb, device, cell, "gmres", True, None)
    u2, s2, r2 = beam(tb, device, cell, "cg", True, None)
    h1, h2 = next(iter(r1._materialized.values()))[0], next(iter(r2._materialized.values()))[0]
    print("%s beam, end pushed: Newton %d / %d iterations; multigrid-GMRES %s, multigrid-CG %s; difference %.2e"
          % (cell, s1.iter, s2.iter, list(s1.linear_iters), list(s2.linear_iters), np.abs(u1 - u2).max()))
    assert h1.general and not h2.general
    assert np.abs(u1 - u2).max() <= 1e-6 * np.abs(u2).max()


def test_simplified_newton_keeps_the_setup(tb, device):
    gh = tb.GridHierarchy(tb.generate_mesh(tb.Hexahedron, (4, 1, 1), (0, 0, 0), (4, 1, 1)), 1)
    dh = tb.DofHandler(gh.grids[-1], tb.LagrangeCollection(1) ** 3)
    sp = tb.allocate_matrix(dh)
    ch = tb.ConstraintHandler(dh, face_dofs(tb, dh))
    op = tb.setup_operator(tb.ElementAssemblyStrategy(device), ho_model(tb, [tb.PressureFieldBC(tb.ConstantCoefficient(0.0005), "bottom")]), dh, sp)
    recipe = tb.GMGPrecon(gh)
    solver = tb.NewtonRaphsonSolver(max_iter=40, tol=1e-9, inner_rtol=1e-8, inner_solver="gmres", inner_precond=recipe, gmres_restart=50, simplified_newton=True)
    u = device.zeros(dh.ndofs)
    assert tb.nlsolve(u, op, ch, solver), (solver.residual_norms, solver.linear_failure)
    hier = next(iter(recipe._materialized.values()))[0]
    print("simplified Newton: %d iterations, %d set-up(s), Arnoldi steps %s" % (solver.iter, hier.n_setups, list(solver.linear_iters)))
    assert solver.iter >= 2 and hier.n_setups == 1 and hier.general
