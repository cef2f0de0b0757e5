"""TT06 reaction kernels with the parameter-only FP64 work formed on the host (CellDerived<TB_CELL_TT06>, tb_reaction.hip), rsqrt_b and the
lower-degree exp_b (tb_math.hpp).

GPU cases: every kernel form that reads the derived block against the CPU oracle at the suite's per-step tolerance (1e-12 of the largest
reference entry, tests/test_gpu_parity.py: TOL / rel_err), on point counts at the wave and workgroup edges of the grid-stride loop.
Host case: exp_b and rsqrt_b compiled for the host and measured against long double next to the forms they replace.
Device math: exp_b, rcp_b, rsqrt_b, log_b and expm1_b evaluated by a kernel each (tests/tb_math_device.hip, built with the library's flags) against the host
build and long double: the hardware seeds of rcp_b and rsqrt_b exist on the device only, the host build stands in for them."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

TOL = 1e-12
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KO, CAO, NAO, VC, BUFC = 12, 13, 14, 15, 18        # parameter slots (CellModel<TB_CELL_TT06>::rhs_rates)
COUNTS = [1, 63, 65, 257]                          # below / above one wave, above one 256-thread workgroup
DT = 0.001


def rel_err(a, r):
    return float(np.abs(np.asarray(a, dtype=np.float64) - r).max() / np.abs(r).max())


def tt06_points(model, n, seed=11):
    """V from rest to plateau (both sides of the −40 mV branch of the h and j gates once n > 1), gates perturbed, concentrations near rest"""
    rng = np.random.default_rng(seed)
    pts = np.tile(model.default_initial_state(), (n, 1))
    pts[:, 0] += rng.uniform(0.0, 110.0, size=n)
    pts[:, 6:] = np.clip(pts[:, 6:] + rng.uniform(-0.2, 0.2, size=(n, 13)), 0.0, 1.0)
    pts[:, 1:6] *= rng.uniform(0.9, 1.1, size=(n, 5))
    return pts


def flat(pts, layout):
    return (np.ascontiguousarray(pts.T) if layout == "SOA" else pts).ravel().copy()


def par(model):
    return model.params.ctypes.data_as(C.POINTER(C.c_double))


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["SOA", "AOS"])
@pytest.mark.parametrize("n", COUNTS)
def test_forward_euler_forms_against_oracle(tb, oracle, device, n, layout):
    """k_reaction<TT06, layout, WRITE_DU, double>: one forward-Euler step and one call of four sub-steps (threshold 0: every point sub-steps), with and
    without du.  The figures are printed before they are asserted."""
    lib, check = tb.lib(), tb._lib.check
    model = tb.TT06()
    host = flat(tt06_points(model, n), layout)
    code = getattr(oracle, "LAYOUT_" + layout)
    for substeps, thr in ((1, 0.0), (4, 0.0)):
        ref = host.copy()
        du_ref = oracle.reaction_step(oracle.CELL_TT06, model.params, ref, n, code, t=0.0, dt=DT, substeps=substeps, threshold=thr)
        got = []
        for with_du in (True, False):
            u = device.to_device(host.copy())
            du = device.zeros(n * 19) if with_du else None
            check(lib.tb_reaction_step(device.h, model.model_id, par(model), len(model.params), u.ptr, du.ptr if with_du else None, n, 19,
                                       0 if layout == "SOA" else 1, 0.0, DT, substeps, thr))
            got.append(u.to_host())
            eu = rel_err(got[-1], ref)
            print("n %d %s substeps %d du %s: u %.3e" % (n, layout, substeps, with_du, eu), end="")
            if with_du:
                edu = rel_err(du.to_host(), du_ref)
                print("  du %.3e" % edu, end="")
            print()
            assert eu < TOL
            if with_du:
                assert edu < 1e-10                      # the suite's bound for the materialised rates (test_reaction_forward_euler_parity)
        np.testing.assert_array_equal(got[0], got[1])   # WRITE_DU changes what is stored, not what is computed


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["SOA", "AOS"])
@pytest.mark.parametrize("n", COUNTS)
def test_float32_storage_against_oracle(tb, oracle, device, n, layout):
    """k_reaction<TT06, layout, ·, float>: states read from and rounded to Float32 once per call, arithmetic in Float64.  Against the oracle's Float64 step
    from the same Float32 inputs the result may differ by the one rounding to Float32 (half a unit in the last place, 2⁻²⁴ relative per entry) plus the
    suite's 1e-12 of the largest entry."""
    lib, check = tb.lib(), tb._lib.check
    model = tb.TT06()
    host32 = flat(tt06_points(model, n), layout).astype(np.float32)
    code = getattr(oracle, "LAYOUT_" + layout)
    for substeps in (1, 4):
        ref = host32.astype(np.float64)
        du_ref = oracle.reaction_step(oracle.CELL_TT06, model.params, ref, n, code, t=0.0, dt=DT, substeps=substeps, threshold=0.0)
        u32, du32 = device.to_device(host32.copy()), tb.DeviceVector(device, n * 19, dtype=np.float32)
        check(lib.tb_reaction_step_f32(device.h, model.model_id, par(model), len(model.params), u32.ptr, du32.ptr, n, 19, 0 if layout == "SOA" else 1,
                                       None, 0, 0.0, DT, substeps, 0.0))
        for name, got, r, tol in (("u", u32.to_host(), ref, TOL), ("du", du32.to_host(), du_ref, 1e-10)):
            excess = np.abs(got.astype(np.float64) - r) - 2.0 ** -24 * np.abs(r)
            print("n %d %s substeps %d f32 %s: beyond the rounding %.3e (bound %.3e)" % (n, layout, substeps, name, excess.max(), tol * np.abs(r).max()))
            assert excess.max() <= tol * np.abs(r).max()


@pytest.mark.gpu
def test_both_sodium_gate_branches_in_one_wave(tb, oracle, device):
    """64 points = one wave whose V straddles −40 mV point by point: the lanes of the wave take both sides of the h / j branch in the same pass"""
    model = tb.TT06()
    n = 64
    pts = tt06_points(model, n)
    pts[:, 0] = -40.0 + np.where(np.arange(n) % 2 == 0, -1.0, 1.0) * np.linspace(0.0, 8.0, n)    # −40 itself (the ≥ side), then alternating sides
    assert (pts[:, 0] < -40.0).sum() >= 16 and (pts[:, 0] >= -40.0).sum() >= 16
    host = flat(pts, "SOA")
    f = tb.PointwiseODEFunction(n, model)
    cache = tb.setup_solver_cache(f, tb.ForwardEulerCellSolver(device), u=device.to_device(host.copy()))
    ref = host.copy()
    du_ref = oracle.reaction_step(oracle.CELL_TT06, model.params, ref, n, oracle.LAYOUT_SOA, t=0.0, dt=DT)
    tb.perform_step(f, cache, 0.0, DT)
    eu, edu = rel_err(cache.un.to_host(), ref), rel_err(cache.du.to_host(), du_ref)
    print("divergent branch: u %.3e du %.3e" % (eu, edu))
    assert eu < TOL and edu < 1e-10
    # per state as well: the h and j gates (states 7, 8) are O(1) beside V = O(100) and would hide in the norm above
    g, r = cache.un.to_host().reshape(19, n), ref.reshape(19, n)
    for k in (7, 8):
        assert rel_err(g[k], r[k]) < TOL


@pytest.mark.gpu
def test_parameter_changed_between_two_calls_is_seen(tb, oracle, device):
    """The derived block is formed from the parameters of every launch: two calls on the same solver cache with Ko, Nao, Cao, Vc and Bufc off their defaults
    and Ko changed again in between — the second call must be the oracle's step with the NEW value (a block kept from the first call would not be)."""
    model = tb.TT06()
    n = 65
    for slot, factor in ((KO, 0.8), (NAO, 1.05), (CAO, 1.3), (VC, 1.2), (BUFC, 0.7)):
        model.params[slot] *= factor
    host = flat(tt06_points(model, n), "SOA")
    f = tb.PointwiseODEFunction(n, model)
    cache = tb.setup_solver_cache(f, tb.ForwardEulerCellSolver(device), u=device.to_device(host.copy()), keep_du=False)
    ref = host.copy()
    tb.perform_step(f, cache, 0.0, DT)
    oracle.reaction_step(oracle.CELL_TT06, model.params, ref, n, oracle.LAYOUT_SOA, t=0.0, dt=DT)
    e1 = rel_err(cache.un.to_host(), ref)
    old = model.params.copy()
    model.params[KO] *= 1.5
    stale = ref.copy()
    tb.perform_step(f, cache, DT, DT)
    oracle.reaction_step(oracle.CELL_TT06, model.params, ref, n, oracle.LAYOUT_SOA, t=DT, dt=DT)
    oracle.reaction_step(oracle.CELL_TT06, old, stale, n, oracle.LAYOUT_SOA, t=DT, dt=DT)
    e2, gap = rel_err(cache.un.to_host(), ref), rel_err(stale, ref)
    print("off-default parameters: call 1 %.3e, call 2 %.3e (stale values would be off by %.3e)" % (e1, e2, gap))
    assert gap > 1e3 * TOL                              # the trap can spring
    assert e1 < TOL and e2 < TOL
    # the Rush–Larsen kernel forms its block per launch too
    rl = tb.setup_solver_cache(f, tb.RushLarsenCellSolver(device), u=device.to_device(host.copy()), keep_du=False)
    ref = host.copy()
    model.params[KO] = old[KO]
    tb.perform_step(f, rl, 0.0, 0.02)
    oracle.reaction_step_rl(oracle.CELL_TT06, model.params, ref, n, oracle.LAYOUT_SOA, t=0.0, dt=0.02)
    model.params[KO] *= 1.5
    tb.perform_step(f, rl, 0.02, 0.02)
    oracle.reaction_step_rl(oracle.CELL_TT06, model.params, ref, n, oracle.LAYOUT_SOA, t=0.02, dt=0.02)
    e3 = rel_err(rl.un.to_host(), ref)
    print("off-default parameters, Rush–Larsen, call 2: %.3e" % e3)
    assert e3 < TOL


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["SOA", "AOS"])
def test_rush_larsen_and_reaction_tangent_against_oracle(tb, oracle, device, layout):
    """k_reaction_rl<TT06> and the tangent-reducing launch of k_reaction (tb_reaction_step_rtc) share rhs_rates with the forward-Euler kernel: 65 points"""
    model = tb.TT06()
    n = 65
    host = flat(tt06_points(model, n), layout)
    code = getattr(oracle, "LAYOUT_" + layout)
    f = tb.PointwiseODEFunction(n, model, layout=tb.StateBlockedLayout() if layout == "SOA" else tb.PointBlockedLayout())
    rl = tb.setup_solver_cache(f, tb.RushLarsenCellSolver(device), u=device.to_device(host.copy()), keep_du=False)
    ref = host.copy()
    tb.perform_step(f, rl, 0.0, 0.02)
    oracle.reaction_step_rl(oracle.CELL_TT06, model.params, ref, n, code, t=0.0, dt=0.02)
    e_rl = rel_err(rl.un.to_host(), ref)
    fe = tb.setup_solver_cache(f, tb.ForwardEulerCellSolver(device), u=device.to_device(host.copy()), keep_du=False)
    ref = host.copy()
    du_ref = oracle.reaction_step(oracle.CELL_TT06, model.params, ref, n, code, t=0.0, dt=DT)
    ok, R = tb.perform_step_with_reaction_tangent(f, fe, 0.0, DT)
    sl = du_ref.reshape(19, n)[0] if layout == "SOA" else du_ref.reshape(n, 19)[:, 0]
    e_fe = rel_err(fe.un.to_host(), ref)
    print("%s: Rush–Larsen %.3e, tangent step %.3e, R %.17g against %.17g" % (layout, e_rl, e_fe, R, sl.max()))
    assert ok is True and e_rl < TOL and e_fe < TOL
    np.testing.assert_allclose(R, sl.max(), rtol=1e-10)  # a rate: the suite's bound for du


def test_exp_b_and_rsqrt_b_are_no_less_accurate_than_what_they_replace(tmp_path):
    """tb_math.hpp compiled for the host (tests/tb_math_host.cpp): largest error in units of the last place against long double of exp_b over
    [−700, 700] — 1.7·10⁶ arguments, 8·10⁵ of them from a few ulp to 10⁻³·ln2 around the reduction boundaries (k + ½)·ln2 — and of rsqrt_b over
    [1, 4] and 10⁻⁶ … 10⁶, each next to the same figure of the form it replaces (the degree-13 Taylor exp_b kept there as a copy; 1/sqrt), measured
    in the same run on the same arguments.  The new figures must not be larger."""
    rocm = os.environ.get("ROCM", os.environ.get("ROCM_PATH", "/opt/rocm"))
    so = str(tmp_path / "libtbmathhost.so")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-ffp-contract=off", "-std=c++17", "-fPIC", "-shared", "-D__HIP_PLATFORM_AMD__",
                           "-I" + os.path.join(rocm, "include"), "-I" + os.path.join(ROOT, "thunderbolt.jl_amd", "csrc"),
                           os.path.join(ROOT, "tests", "tb_math_host.cpp"), "-o", so])
    L = C.CDLL(so)
    fns = {}
    for name in ("max_ulps_exp_b", "max_ulps_exp_b_before", "max_ulps_rsqrt_b", "max_ulps_rsqrt_before"):
        fn = getattr(L, name)
        fn.restype, fn.argtypes = C.c_double, [C.c_void_p, C.c_long]
        fns[name] = lambda a, fn=fn: fn(a.ctypes.data, len(a))
    rng = np.random.default_rng(1)
    ln2 = float(np.log(2.0))
    k = rng.integers(-1009, 1010, 400000)
    x = np.concatenate([rng.uniform(-700, 700, 600000), rng.uniform(-100, 100, 300000),
                        (k + 0.5) * ln2 + rng.uniform(-1e-3, 1e-3, 400000) * ln2,
                        (k + 0.5) * ln2 * (1 + rng.integers(-4, 5, 400000) * 2.2e-16)])
    x = np.ascontiguousarray(x[(x >= -700) & (x <= 700)])
    assert len(x) >= 10 ** 6
    new, old = fns["max_ulps_exp_b"](x), fns["max_ulps_exp_b_before"](x)
    print("exp_b: %.4f ulp, degree-13 Taylor form %.4f ulp (%d arguments)" % (new, old, len(x)))
    assert new <= old
    y = np.concatenate([rng.uniform(1, 4, 1000000), 10 ** rng.uniform(-6, 6, 500000)])
    new, old = fns["max_ulps_rsqrt_b"](y), fns["max_ulps_rsqrt_before"](y)
    print("rsqrt_b: %.4f ulp, 1/sqrt %.4f ulp (%d arguments)" % (new, old, len(y)))
    assert new <= old and new <= 2.0


# ------------------------------------------------------------------------------------------- the math functions on the device
LD = np.longdouble
NARG = 2 ** 18
HALF_SQRT2 = 0.70710678118654752                    # the cut of log_b's mantissa range [√½, √2)
FUNCTIONS = ("exp_b", "rcp_b", "rsqrt_b", "log_b", "expm1_b")      # in the order of the enum of tests/tb_math_device.hip


def _spread_ulps(rng, centre, count, width):
    """`centre` moved by a whole number of units in the last place, −width … width"""
    return centre * (1.0 + rng.integers(-width, width + 1, count) * 2.0 ** -52)


@pytest.fixture(scope="module")
def math_args():
    """2¹⁸ arguments per function, fixed seed, only where the function is defined (tb_math.hpp)"""
    rng = np.random.default_rng(20261)
    ln2 = float(np.log(2.0))
    sign = lambda m: np.where(rng.integers(0, 2, m) == 1, 1.0, -1.0)      # noqa: E731
    a = {}
    # the set of the host test below, scaled to 2¹⁸: uniform in ±700 and ±100, and the reduction boundaries (k + ½)·ln2 from a few ulp to 10⁻³·ln2 away
    k1, k2 = rng.integers(-1009, 1010, 57344), rng.integers(-1009, 1010, 57344)
    a["exp_b"] = np.concatenate([rng.uniform(-700, 700, 98304), rng.uniform(-100, 100, 49152), (k1 + 0.5) * ln2 + rng.uniform(-1e-3, 1e-3, 57344) * ln2,
                                 (k2 + 0.5) * ln2 * (1 + rng.integers(-4, 5, 57344) * 2.2e-16)])
    a["rcp_b"] = np.concatenate([sign(2 ** 17) * 10.0 ** rng.uniform(-12, 12, 2 ** 17), rng.uniform(1, 2, 2 ** 17 - 4), [1.0, np.nextafter(1.0, 2.0), np.nextafter(2.0, 1.0), 2.0]])
    a["rsqrt_b"] = np.concatenate([rng.uniform(1, 4, 2 ** 17), 10.0 ** rng.uniform(-6, 6, 2 ** 17)])
    cuts = HALF_SQRT2 * 2.0 ** rng.integers(-22, 11, 2 ** 15)                        # √½·2ᵉ inside 10⁻⁷ … 10³: where frexp's mantissa crosses the cut
    a["log_b"] = np.concatenate([10.0 ** rng.uniform(-7, 3, 2 ** 17), rng.uniform(0.7, 1.3, 2 ** 16 + 2 ** 15), _spread_ulps(rng, cuts, 2 ** 15, 64)])
    edge = np.concatenate([_spread_ulps(rng, s * np.full(32, 0.3), 32, 8) for s in (1.0, -1.0)])      # both sides of the switch between series and exp_b − 1
    a["expm1_b"] = np.concatenate([rng.uniform(-0.3, 0.3, 2 ** 16), sign(2 ** 16) * 10.0 ** rng.uniform(-12, -3, 2 ** 16),
                                   sign(2 ** 17 - 64) * rng.uniform(0.3, 50.0, 2 ** 17 - 64), edge])
    for name, x in a.items():
        assert len(x) == NARG and np.isfinite(x).all(), name
        a[name] = np.ascontiguousarray(x, dtype=np.float64)
    assert np.abs(a["exp_b"]).max() <= 700.0
    assert 1e-12 <= np.abs(a["rcp_b"]).min() and np.abs(a["rcp_b"]).max() <= 1e12
    assert 1e-6 <= a["rsqrt_b"].min() and a["rsqrt_b"].max() <= 1e6
    assert 1e-7 <= a["log_b"].min() and a["log_b"].max() <= 1e3 and (a["log_b"] < HALF_SQRT2).any()
    assert np.abs(a["expm1_b"]).max() <= 50.0 and (np.abs(edge) < 0.3).any() and (np.abs(edge) >= 0.3).any()
    return a


@pytest.fixture(scope="module")
def math_truth(math_args):
    """the exact values to 2⁻¹¹ of a double's last place: numpy.longdouble where it has a 64-bit significand (x87), skipped elsewhere"""
    if np.finfo(LD).nmant < 63:
        pytest.skip("numpy.longdouble has no 64-bit significand here")
    x = {k: v.astype(LD) for k, v in math_args.items()}
    return {"exp_b": np.exp(x["exp_b"]), "rcp_b": LD(1) / x["rcp_b"], "rsqrt_b": LD(1) / np.sqrt(x["rsqrt_b"]), "log_b": np.log(x["log_b"]),
            "expm1_b": np.expm1(x["expm1_b"])}


def max_ulps(got, truth):
    """largest |got − truth| in units of the last place of a double at the truth's magnitude (2^(ilogb(truth) − 52), as tests/tb_math_host.cpp counts)"""
    _, e = np.frexp(truth)                                         # |truth| = m·2ᵉ, m in [½, 1): ilogb = e − 1
    err = np.abs(got.astype(LD) - truth) / np.ldexp(LD(1), e - 53)
    return float(err.max()) if np.isfinite(got).all() else float("nan")


@pytest.fixture(scope="module")
def host_math(tmp_path_factory, math_args):
    """the five functions of the host build of tb_math.hpp (tests/tb_math_host.cpp) on math_args"""
    rocm = os.environ.get("ROCM", os.environ.get("ROCM_PATH", "/opt/rocm"))
    so = str(tmp_path_factory.mktemp("tbmathhost") / "libtbmathhost.so")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-ffp-contract=off", "-std=c++17", "-fPIC", "-shared", "-D__HIP_PLATFORM_AMD__",
                           "-I" + os.path.join(rocm, "include"), "-I" + os.path.join(ROOT, "thunderbolt.jl_amd", "csrc"),
                           os.path.join(ROOT, "tests", "tb_math_host.cpp"), "-o", so])
    L = C.CDLL(so)
    out = {}
    for name in FUNCTIONS:
        fn = getattr(L, "eval_" + name)
        fn.restype, fn.argtypes = None, [C.c_void_p, C.c_long, C.c_void_p]
        y = np.full(NARG, np.nan)
        fn(math_args[name].ctypes.data, NARG, y.ctypes.data)
        out[name] = y
    return out


def test_log_b_and_expm1_b_of_the_host_build_against_long_double(math_args, math_truth, host_math):
    """The two functions tb_math.hpp gave no figure for.  Measured on 3·10⁶ arguments each of the same ranges: log_b 2.38 ulp on 10⁻⁷ … 10³ and 2.42 ulp on
    [0.7, 1.3], expm1_b 1.48 ulp for |z| < 0.3 and 3.31 ulp for 0.3 ≤ |z| ≤ 50 (libm: log 0.52 ulp, exp(z) − 1 2.01 ulp).  The bounds are those figures
    rounded up to the next integer: a later change of coefficients cannot slide past them."""
    e_log, e_expm1 = max_ulps(host_math["log_b"], math_truth["log_b"]), max_ulps(host_math["expm1_b"], math_truth["expm1_b"])
    z = math_args["expm1_b"]
    small = np.abs(z) < 0.3
    e_small = max_ulps(host_math["expm1_b"][small], math_truth["expm1_b"][small])
    print("host build: log_b %.4f ulp; expm1_b %.4f ulp (|z| < 0.3: %.4f ulp); %d arguments each" % (e_log, e_expm1, e_small, NARG))
    assert e_log <= 3.0
    assert e_expm1 <= 4.0


@pytest.mark.gpu
def test_math_functions_on_the_device(tmp_path, math_args, math_truth, host_math):
    """exp_b, rcp_b, rsqrt_b, log_b and expm1_b as the kernels get them: tests/tb_math_device.hip built with the library's flags (-O3 -ffp-contract=fast for
    gfx950), one kernel per function, on math_args.
      exp_b, expm1_b  no hardware seed and every fused multiply-add written out: bit for bit the host build's values, which pins the device to the host
                      measurement against long double (0.862 ulp for exp_b);
      rcp_b           ≤ 2 ulp (the header's claim for v_rcp_f64 and two Newton steps);
      rsqrt_b         ≤ 2 ulp, and no more than 1.0 / sqrt(y) evaluated in the same kernel (the host assertion above, on the device);
      log_b           ≤ the host build's error on the same arguments + 3 ulp: the one seed dependence is rcp_b(m + 1), allowed 2 ulp on the device against
                      the stand-in's 0.5; log m = 2f(1 + …) carries f's relative error one to one, and a relative error is worth up to twice as many units in
                      the last place on the far side of a binade.
    Every figure is printed before it is asserted."""
    import shutil
    hipcc = shutil.which("hipcc") or os.path.join(os.environ.get("ROCM", os.environ.get("ROCM_PATH", "/opt/rocm")), "bin", "hipcc")
    so = str(tmp_path / "libtbmathdevice.so")
    b = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=fast", "-shared", "-fPIC",
                        "-I" + os.path.join(ROOT, "thunderbolt.jl_amd", "csrc"), os.path.join(ROOT, "tests", "tb_math_device.hip"), "-o", so],
                       capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-2000:]
    fn = C.CDLL(so).tb_math_device_eval
    fn.restype, fn.argtypes = C.c_int, [C.c_int, C.c_void_p, C.c_long, C.c_void_p, C.c_void_p]
    dev, plain_rsqrt = {}, np.full(NARG, np.nan)
    for which, name in enumerate(FUNCTIONS):
        y = np.full(NARG, np.nan)
        rc = fn(which, math_args[name].ctypes.data, NARG, y.ctypes.data, plain_rsqrt.ctypes.data if name == "rsqrt_b" else None)
        assert rc == 0, "%s: HIP status %d" % (name, rc)
        dev[name] = y
    e_dev = {name: max_ulps(dev[name], math_truth[name]) for name in FUNCTIONS}
    e_host = {name: max_ulps(host_math[name], math_truth[name]) for name in FUNCTIONS}
    e_plain = max_ulps(plain_rsqrt, math_truth["rsqrt_b"])
    for name in FUNCTIONS:
        differ = np.flatnonzero(dev[name].view(np.uint64) != host_math[name].view(np.uint64))
        print("%-8s device %.4f ulp, host build %.4f ulp, %d of %d values differ from the host build%s" % (
            name, e_dev[name], e_host[name], len(differ), NARG, "".join(" [x = %r: device %r, host %r]" % (
                float(math_args[name][i]), float(dev[name][i]), float(host_math[name][i])) for i in differ[:3]) if name in ("exp_b", "expm1_b") else ""))
    print("1.0 / sqrt(y) in the rsqrt_b kernel: %.4f ulp" % e_plain)
    np.testing.assert_array_equal(dev["exp_b"].view(np.uint64), host_math["exp_b"].view(np.uint64))
    np.testing.assert_array_equal(dev["expm1_b"].view(np.uint64), host_math["expm1_b"].view(np.uint64))
    assert e_dev["rcp_b"] <= 2.0
    assert e_dev["rsqrt_b"] <= 2.0 and e_dev["rsqrt_b"] <= e_plain
    assert e_dev["log_b"] <= e_host["log_b"] + 3.0
