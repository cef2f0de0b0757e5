"""tests/krylov_reference.py checked without a device, so that tests/test_krylov_iterates_gpu.py can lean on it:

  * every recurrence against the same recurrence on 40-digit mpmath numbers (n = 120): the reference's own rounding lies 1 000× below the smallest
    tolerance the device comparison uses;
  * power: each of the six defects (`mutant=`) moves every iterate it can act on by at least 1 000 × that case's tolerance, at two or more checked k
    per solver — the float32 comparison by 1 000 ulp or more;
  * the inputs: no checked iterate at convergence, no residual within a factor 2 of a stopping tolerance of the count cases, no Lanczos β under
    10⁻⁶·|α|, no zero on a rotated Hessenberg diagonal, no float32 entry whose ulp the double tolerance could reach."""
import sys
import os

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import krylov_reference as kr  # noqa: E402

LD = kr.LD
SMALLEST_TOLERANCE = kr.tolerance(0.0)                    # 16 · 2⁻⁵⁰ ≈ 1.4e-14
MP_AGREEMENT = SMALLEST_TOLERANCE / 1000.0
SEPARATION = 1000.0
N_CU = 256                                                # MI355X: the large system is the 81³ cube of nodes


@pytest.fixture(scope="module")
def systems(tb):
    return kr.build_systems(kr.meshes(tb))


@pytest.fixture(scope="module")
def large(tb):
    return kr.build_systems({**kr.meshes(tb), "large": kr.large_mesh(tb, N_CU)})


def small_cases():
    return [c for c in kr.CASES if c.system != "large"]


def ids(cases):
    return [c.id for c in cases]


# ------------------------------------------------------------------------------------------------ the reference's own rounding
MP_CASES = [c for c in kr.CASES + kr.COUNT_CASES if c.system in ("n120", "n120g")]


# The one kind of quantity that cannot meet MP_AGREEMENT, named: a step or a norm formed by cancellation, whose error in ANY arithmetic is the unit
# roundoff times the cancellation factor.  (a) The true residual ‖b − A·x_k‖ of a late GMRES iterate: where ‖r_k‖ has fallen to 10⁻³…10⁻⁴·‖r₀‖, with
# entries of A·x_k spread over 2¹⁰ by the two-sided scaling, longdouble carries up to 1e-16 of it and double 7e-13 — the device tolerance of that
# norm is then 16·ε_ref ≈ 1e-11, five orders above.  (b) Unpreconditioned CG from a random x₀ on the two-sidedly scaled matrix: the first direction is
# r₀ = b − A·x₀ itself, a difference of vectors whose entries spread over 2¹⁰, and x₁ − x₀, x₂ − x₀ inherit its 2e-17 (Jacobi scales it away).
# Each entry: case id → the (quantity, k) excepted.  The bound of an exception is 1/1000 of the device tolerance of that very quantity and no more than
# MP_EXCEPTION_CEILING; anything not listed here is held to MP_AGREEMENT.  Measured: (a) 1.8e-17 … 9.6e-17 (1.2 … 6.8 × MP_AGREEMENT), (b) 2.2e-17 and
# 1.8e-17; the worst quantity that is no exception 1.4e-17 = 0.98 × MP_AGREEMENT (x₃ − x₀ of the case of (b)), then 0.86 (‖r₄‖ of (a)), 0.47.
MP_EXCEPTION_CEILING = 2e-16
MP_EXCEPTIONS = {"n120-gmres-jacobi1-restart30-k6-x0zero-kstar6-maxiter50": {("res", 5), ("res", 6)},
                 "n120-gmres-jacobi1-restart4-k6-x0zero-kstar6-maxiter50": {("res", 5), ("res", 6)},
                 "n120-none-x0rand": {("x", 1), ("x", 2)}}
assert set(MP_EXCEPTIONS) <= {c.id for c in MP_CASES}

WORST_MP = {}


@pytest.mark.parametrize("c", MP_CASES, ids=ids(MP_CASES))
def test_recurrence_agrees_with_mpmath_at_40_digits(systems, c):
    """every iterate and every scalar the device test compares, at every k (checked or not): the extended-precision run agrees with the 40-digit run
    to MP_AGREEMENT = 16·2⁻⁵⁰/1000 ≈ 1.4e-17, 1 000× under the smallest tolerance of the device comparison; the quantities named in MP_EXCEPTIONS,
    and only those, to 1/1000 of their own device tolerance"""
    import mpmath
    R = kr.reference(c, systems)
    listed = MP_EXCEPTIONS.get(c.id, set())
    over = {}
    with mpmath.workdps(40):
        mp = c.run(systems[c.system], dtype=object)
        x0 = kr.cast(R.x0, object)
        worst = 0.0
        for k in range(1, len(mp["x"]) + 1):
            dmp, dld = mp["x"][k - 1] - x0, kr.to_mp(R.ld["x"][k - 1]) - x0
            errs = {"x": (float(np.abs(dld - dmp).max() / np.abs(dmp).max()), R.tol_x(k))}
            for key in [a for a in ("res", "gamma", "delta", "rho") if a in mp]:
                errs[key] = (float(abs(kr.to_mp(R.ld[key][k]) - mp[key][k]) / abs(mp[key][k])), R.tol_scalar(key, k))
            for key, (err, tol) in errs.items():
                if (key, k) in listed:
                    print("%s: exception %s at k = %d: %.2e = %.2f x MP_AGREEMENT, its device tolerance %.2e" % (c.id, key, k, err, err / MP_AGREEMENT, tol))
                    assert err <= min(tol / 1000.0, MP_EXCEPTION_CEILING), (key, k, err, tol)
                else:
                    worst = max(worst, err)
                    if err > MP_AGREEMENT:
                        over[(key, k)] = err
    WORST_MP[c.id] = worst / MP_AGREEMENT
    print("%s: longdouble against 40 digits, worst error %.2e = %.3f x MP_AGREEMENT" % (c.id, worst, worst / MP_AGREEMENT))
    assert not over, "above MP_AGREEMENT = %.2e and not a named exception: %s" % (MP_AGREEMENT, over)


def test_lambda_max_agrees_with_mpmath_at_40_digits(systems):
    import mpmath
    with mpmath.workdps(40):
        mp = kr.lambda_max(systems["n120"].op(object))
        ld = kr.lambda_max(systems["n120"].op())
        errs = {key: float(abs(kr.to_mp(ld[key]) - mp[key]) / abs(mp[key])) for key in ("lmax", "gersh", "theta")}
    print("lambda_max, longdouble against 40 digits:", errs)
    assert max(errs.values()) <= MP_AGREEMENT
    assert len(ld["alpha"]) == kr.LANCZOS_STEPS


def test_csr_product_orders_and_dtypes(systems):
    s = systems["n120g"]
    x = np.random.default_rng(0).normal(size=s.n)
    dense = np.zeros((s.n, s.n), dtype=LD)
    rows = np.repeat(np.arange(s.n), np.diff(s.rowptr))
    dense[rows, s.colidx] = s.vals
    want = dense @ x.astype(LD)
    scale = np.abs(dense) @ np.abs(x).astype(LD)
    for dtype, eps in ((LD, np.finfo(LD).eps), (np.float64, np.finfo(np.float64).eps)):
        ys = [kr.csr_matvec(s.rowptr, s.colidx, s.vals, x, dtype, order) for order in ("natural", "reversed")]
        for y in ys:
            assert y.dtype == dtype and np.all(np.abs(y.astype(LD) - want) <= 28 * float(eps) * scale)    # 27 entries per row at the most
        assert dtype is LD or not np.array_equal(ys[0], ys[1])          # the two orders do round differently


# ------------------------------------------------------------------------------------------------ power
def ulps32(x, ref):
    """|x − ref| in units of the float32 spacing at ref, both rounded once to float32"""
    a, r = np.asarray(x, dtype=LD).astype(np.float32), np.asarray(ref, dtype=LD).astype(np.float32)
    return np.abs(a.astype(np.float64) - r.astype(np.float64)) / np.spacing(np.abs(r)).astype(np.float64)


def separated(R, c, sysm, mutant):
    """the checked k at which the mutant lies at least SEPARATION × tolerance from the reference"""
    run = c.run(sysm, mutant=mutant)
    good = []
    for k in c.ks:
        dev, tol = kr.deviation(R.dx(k, run), R.dx(k)), R.tol_x(k)
        ok = dev >= SEPARATION * tol
        if c.solver == "f32":
            u = float(ulps32(run["x"][k - 1], R.ld["x"][k - 1]).max())
            ok = ok and u >= 1000.0
        if ok:
            good.append(k)
    return good


def test_every_mutant_is_separated_from_the_reference(systems):
    per_solver = {}
    for c in small_cases():
        R = kr.reference(c, systems)
        for m in c.mutants():
            good = separated(R, c, systems[c.system], m)
            # a defect may go unseen at k = 1, 2 (most first act at k = 3); every checked k ≥ 3 separates it
            assert set(k for k in c.ks if k >= 3) <= set(good), (c.id, m, good)
            per_solver.setdefault((c.solver, m), set()).update(good)
    for (solver, m), ks in sorted(per_solver.items()):
        print("%-14s %-22s separated at k = %s" % (solver, m, sorted(ks)))
        assert len(ks) >= 2, (solver, m, ks)
    seen = {m for (_, m) in per_solver}
    assert seen == set(kr.MUTANTS)


def test_large_system_inputs_and_power(large):
    """the 81³ system of the device test (Jacobi-CG, k ≤ 3 and one count): its mutants, its distance from convergence and its count margin"""
    c = kr.case("large", "jacobi")
    R = kr.reference(c, large)
    res = [float(r) for r in R.ld["res"]]
    assert res[3] / res[0] >= 1e-7
    for m in c.mutants():
        good = separated(R, c, large["large"], m)
        assert 3 in good, (m, good)
    cc = [q for q in kr.COUNT_CASES if q.system == "large"][0]
    check_count_margins(cc, res)


# ------------------------------------------------------------------------------------------------ input conditions
@pytest.mark.parametrize("c", small_cases(), ids=ids(small_cases()))
def test_no_checked_iterate_sits_at_convergence(systems, c):
    R = kr.reference(c, systems)
    res = [float(r) for r in R.ld["res"]]
    print("%s: |r_k| / |r_0| = %s" % (c.id, " ".join("%.1e" % (r / res[0]) for r in res[1:])))
    assert res[max(c.ks)] / res[0] >= 1e-7
    assert len(R.ld["x"]) == max(c.ks) == len(res) - 1
    if c.solver == "gmres":
        assert all(float(h) != 0.0 for h in R.ld["hdiag"]) and len(R.ld["hdiag"]) == max(c.ks)
        assert min(float(abs(h)) for h in R.ld["hdiag"]) >= 1e-6 * max(float(abs(h)) for h in R.ld["hdiag"])
    if c.solver == "f32":       # a double iterate within 16·ε_ref lies less than one float32 spacing from the reference in every entry, the smallest
        for k in c.ks:          # included: the two then round to the same or to neighbouring float32 numbers (no floor here: this guards against a
            x = np.abs(R.ld["x"][k - 1]).astype(np.float64)    # needless failure of the one-ulp check, not against a wrong pass)
            assert kr.FACTOR * R.eps_x(k) * float(np.abs(R.dx(k)).max()) <= float(np.spacing(x.astype(np.float32)).min())


def check_count_margins(c, res):
    rtol = kr.rtol_for(res, c.kstar)
    tol = rtol * res[0]
    assert c.kstar <= 32 and all(res[k] >= 2.0 * tol for k in range(c.kstar)), (c.id, [r / tol for r in res])
    assert all(res[k] <= tol / 2.0 for k in range(c.kstar, c.returned + 1)), (c.id, [r / tol for r in res])
    return rtol


SMALL_COUNTS = [c for c in kr.COUNT_CASES if c.system != "large"]


@pytest.mark.parametrize("c", SMALL_COUNTS, ids=ids(SMALL_COUNTS))
def test_count_cases_keep_a_factor_two_from_the_stopping_tolerance(systems, c):
    R = kr.reference(c, systems)
    res = [float(r) for r in R.ld["res"]]
    rtol = check_count_margins(c, res)
    print("%s: rtol %.3e, |r_k| / tol = %s" % (c.id, rtol, " ".join("%.2f" % (r / (rtol * res[0])) for r in res)))
    if c.solver == "gmres":                               # the rotated right-hand side the solver stops on is the true residual to rounding
        assert all(kr.relative(e, r) <= 1e-12 for e, r in zip(R.ld["est"], R.ld["res"]))
    if c.solver in ("jacobi", "from_residual", "f32"):
        assert c.kstar % 4 != 0                           # (a multiple of 4 would not tell a look every fourth iteration from one every iteration)


@pytest.mark.parametrize("name", ["n120", "n1716", "mg175", "mg1573"])
def test_lanczos_inputs(systems, name):
    s = systems[name]
    lm = kr.lambda_max(s.op())
    al, be = [float(a) for a in lm["alpha"]], [float(b) for b in lm["beta"]]
    assert len(al) == kr.LANCZOS_STEPS and all(be[k + 1] >= 1e-6 * abs(al[k]) for k in range(len(al)))
    dense = np.zeros((s.n, s.n))
    dense[np.repeat(np.arange(s.n), np.diff(s.rowptr)), s.colidx] = s.vals
    d = 1.0 / np.sqrt(np.diag(dense))
    true = float(np.linalg.eigvalsh(dense * d[:, None] * d[None, :])[-1])
    print("%s: gersh %.4f, 1.05·theta %.6f, true %.6f" % (name, float(lm["gersh"]), 1.05 * float(lm["theta"]), true))
    assert 0.9 * true <= float(lm["lmax"]) <= float(lm["gersh"])
    # in double, in either summation order, the 24-step value moves by what the device comparison allows for
    eps = max(kr.relative(kr.lambda_max(s.op(np.float64, o))["lmax"], lm["lmax"]) for o in ("natural", "reversed"))
    print("%s: eps_ref of lambda_max %.2e" % (name, eps))
    assert eps <= 1e-9


def test_exact_edge_inputs(systems):
    """the diagonal system of the exact-convergence checks: b / diag is exact, and the textbook recurrence converges in one step"""
    s = systems["n120"]
    d = kr.diagonal_system("diag", s.rowptr, s.colidx, 5000)
    rows = np.repeat(np.arange(d.n), np.diff(d.rowptr))
    diag = d.vals[rows == d.colidx]
    assert np.all(np.log2(diag) == np.round(np.log2(diag))) and np.count_nonzero(d.vals) == d.n
    out = kr.pcg(d.op(np.float64), d.b, d.x0[False], 1, kr.jacobi(d.op(np.float64)))
    assert np.array_equal(out["x"][0], d.b / diag) and float(out["res"][1]) == 0.0
