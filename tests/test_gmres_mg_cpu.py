"""Multigrid-preconditioned GMRES without a GPU: the reference recurrence of tests/gmres_mg_reference.py against a dense least-squares solution over
the Krylov space, the error returns of the four new C entries on NULL arguments, and the Python surface (KrylovGMRES, KrylovMGSolver, gmres_solve)."""
import ctypes as C

import numpy as np
import pytest

import gmres_mg_reference as gref
import krylov_reference as kr

LD = np.longdouble


def seeded_system(seed, n=40):
    """a dense non-symmetric A = D(I + 0.3 G/√n) with a positive diagonal scale D over four octaves, and M⁻¹ = (D + a random tridiagonal part)⁻¹: a
    fixed, non-symmetric preconditioner that is neither Jacobi nor exact"""
    rng = np.random.default_rng(seed)
    D = 2.0 ** rng.uniform(-2, 2, n)
    A = D[:, None] * (np.eye(n) + 0.3 * rng.normal(size=(n, n)) / np.sqrt(n))
    T = np.diag(D) + np.diag(0.2 * D[:-1] * rng.normal(size=n - 1), 1) + np.diag(0.2 * D[1:] * rng.normal(size=n - 1), -1)
    Minv = np.linalg.inv(T)
    return A, Minv, rng.normal(size=n), rng.normal(size=n) / D


def least_squares_iterate(A, Minv, b, x0, k):
    """x0 + M⁻¹ K y with y minimising ‖r0 − A M⁻¹ K y‖₂ over the Krylov space K = span{r0, (A M⁻¹) r0, …} of dimension k, on an orthonormalised basis
    (float64 lstsq; the basis is orthonormalised twice so that the k ≤ 6 columns stay well conditioned)"""
    r0 = b - A @ x0
    B = A @ Minv
    K = [r0 / np.linalg.norm(r0)]
    for _ in range(k - 1):
        w = B @ K[-1]
        for _ in range(2):
            for v in K:
                w = w - (v @ w) * v
        K.append(w / np.linalg.norm(w))
    K = np.array(K).T
    y = np.linalg.lstsq(B @ K, r0, rcond=None)[0]
    return x0 + Minv @ (K @ y)


@pytest.mark.parametrize("seed", [11, 12])
def test_reference_minimises_the_residual_over_the_krylov_space(seed):
    A, Minv, b, x0 = seeded_system(seed)
    mv = lambda x: A.astype(LD) @ x                           # noqa: E731
    M = lambda v: Minv.astype(LD) @ v                         # noqa: E731
    # inside one cycle
    out = gref.right_gmres(mv, M, b, x0, 6, 30)
    for k in (1, 2, 3, 6):
        want = least_squares_iterate(A, Minv, b, x0, k)
        err = kr.deviation(out["x"][k - 1] - x0, want - x0)
        true = float(np.linalg.norm(b - A @ want))
        print("seed %d k %d: iterate against least squares %.2e; residual %.6e, estimate %.6e" % (seed, k, err, float(out["res"][k]), float(out["est"][k])))
        assert err <= 1e-10
        assert abs(float(out["res"][k]) - true) <= 1e-10 * true and abs(float(out["est"][k]) - true) <= 1e-10 * true
    assert all(float(a) >= float(c) for a, c in zip(out["res"], out["res"][1:]))       # the residual of a cycle does not grow
    # across a restart: three steps, then two more from the iterate of the third (the extra M⁻¹ of the cycle's end is part of x_3)
    out = gref.right_gmres(mv, M, b, x0, 5, 3)
    x3 = least_squares_iterate(A, Minv, b, x0, 3)
    x5 = least_squares_iterate(A, Minv, b, x3, 2)
    assert kr.deviation(out["x"][2] - x0, x3 - x0) <= 1e-10 and kr.deviation(out["x"][4] - x0, x5 - x0) <= 1e-10
    # the double runs in two summation orders stay near the extended one and differ from each other (the tolerance rule needs both)
    f = [gref.right_gmres(lambda x: A @ x, lambda v: Minv @ v, b, x0, 5, 3, np.float64, order) for order in ("natural", "reversed")]
    devs = [kr.deviation(r["x"][4] - x0, out["x"][4] - x0) for r in f]
    print("seed %d: float64 runs deviate by %.2e and %.2e" % (seed, devs[0], devs[1]))
    assert max(devs) <= 1e-12 and not np.array_equal(f[0]["x"][4], f[1]["x"][4])


def test_restart_one_is_a_minimal_residual_step_per_cycle():
    A, Minv, b, x0 = seeded_system(13)
    out = gref.right_gmres(lambda x: A.astype(LD) @ x, lambda v: Minv.astype(LD) @ v, b, x0, 3, 1)
    x = x0
    for k in range(3):
        x = least_squares_iterate(A, Minv, b, x, 1)
        assert kr.deviation(out["x"][k] - x0, x - x0) <= 1e-10


def test_skewed_matrix_is_what_the_issue_states(tb):
    dh = tb.DofHandler(tb.generate_mesh(tb.Hexahedron, (3, 2, 2), (0, 0, 0), (1, 1, 1)))
    sp = tb.allocate_matrix(dh)
    sysm = kr.spd_system("s", sp.rowptr, sp.colidx, 5)
    v = np.abs(sysm.vals)                                     # positive diagonal
    fixed = np.array([0, 7])
    w = gref.skewed(sp.rowptr, sp.colidx, v, 3, s=0.1, untouched=fixed)
    A, S = gref.dense(sp.rowptr, sp.colidx, v), gref.dense(sp.rowptr, sp.colidx, w)
    E = S - A
    d = np.sqrt(np.diag(A))
    sig = E / (0.1 * d[:, None] * d[None, :])
    assert np.abs(E + E.T).max() <= 1e-15 * np.abs(A).max() and np.abs(sig).max() <= 1.0 + 1e-12 and np.abs(sig).max() > 0.5
    assert np.array_equal(np.diag(S), np.diag(A)) and not E[fixed].any() and not E[:, fixed].any()
    assert np.array_equal(gref.skewed(sp.rowptr, sp.colidx, v, 3), gref.skewed(sp.rowptr, sp.colidx, v, 3))


def test_abi_additions(tb):
    L, lib = tb._lib, tb.lib()
    for name in ("tb_gmres_solve_mg", "tb_gmres_solve_amg", "tb_mg_set_general", "tb_amg_set_general"):
        assert name in L.SIGNATURES and hasattr(lib, name), name
    it, v = C.c_int(), C.c_double()
    calls = [lib.tb_gmres_solve_mg(None, None, None, None, 1e-8, 0.0, 10, 5, None, C.byref(it), C.byref(v)),
             lib.tb_gmres_solve_amg(None, None, None, None, 1e-8, 0.0, 10, 5, None, C.byref(it), C.byref(v)),
             lib.tb_mg_set_general(None, 1), lib.tb_amg_set_general(None, 1)]
    assert calls == [L.TB_ERR_BAD_ARG] * 4, calls
    assert b"NULL" in lib.tb_last_error_string()


def test_krylov_gmres_is_accepted_and_the_bare_string_points_at_it(tb):
    gh = tb.GridHierarchy(tb.generate_mesh(tb.Hexahedron, (2, 2, 2), (0, 0, 0), (1, 1, 1)), 1)
    assert tb.KrylovGMRES().restart == 50 and tb.KrylovGMRES(restart=400).restart == 400
    with pytest.raises(ValueError, match="restart"):
        tb.KrylovGMRES(0)
    for mg in (tb.GMGPrecon(gh), tb.PMGPrecon(), tb.ChainedMGPrecon(tb.PMGPrecon(), tb.AMGPrecon()), tb.AMGPrecon(near_nullspace="rigid_body"),
               tb.GMGPrecon(gh, coarse=tb.AMGPrecon())):
        s = tb.KrylovMGSolver(tb.KrylovGMRES(restart=30), mg, maxiters=77)
        assert s.mg is mg and s.krylov.restart == 30 and s.maxiters == 77
    with pytest.raises(TypeError, match="mg must be"):
        tb.KrylovMGSolver(tb.KrylovGMRES(), tb.ChebyshevPrecBuilder(4))
    with pytest.raises(TypeError, match="mg must be"):
        tb.KrylovMGSolver(tb.KrylovGMRES(), None)
    with pytest.raises(NotImplementedError, match="KrylovGMRES"):
        tb.KrylovMGSolver("gmres", tb.AMGPrecon())
    with pytest.raises(TypeError, match="precond"):
        tb.gmres_solve(None, None, None, None, precond=tb.ChebyshevPrecBuilder(4))
    assert tb.NewtonRaphsonSolver(inner_solver="gmres", inner_precond=tb.AMGPrecon(), gmres_restart=40).gmres_restart == 40
    for cls in (tb.MultigridHierarchy, tb.amg.AlgebraicHierarchy):
        assert cls.general is False and cls.n_setups == 0 and callable(cls.solve_gmres) and callable(cls.set_general)
