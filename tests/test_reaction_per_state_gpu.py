"""Every form of the reaction kernels against the CPU oracle, state by state: helpers.per_state_err, the suite's thresholds (1e-12 for states, 1e-10 for
rates) applied to each state relative to that state's own largest reference entry.  The global norm of the other reaction tests divides by the largest
entry of the whole array (K_i, V) and lets a calcium flux that is off by a thousandth pass: tests/test_reaction_per_state_cpu.py shows it on the oracle,
and that the oracle's own spread under 1-ulp perturbations is below 1/50 of these thresholds in every form below.

Point counts: 65 (one lane past a wave) and 1037 (four workgroups and a ragged tail) — the smallest at which the index arithmetic of both layouts can go
wrong.  Start values: initial_points of tests/test_gpu_parity.py.  Every figure is printed before it is asserted."""
import numpy as np
import pytest

from helpers import ADAPTIVE_DT, ADAPTIVE_THRESHOLD, FE_DT, RL_DT, per_state_ratio, phi_rates
from test_gpu_parity import MODELS, initial_points

pytestmark = pytest.mark.gpu

TOL_U, TOL_DU = 1e-12, 1e-10
COUNTS = [65, 1037]
LAYOUTS = ["SOA", "AOS"]
# the six cell models: the five of test_gpu_parity.MODELS and the heterogeneous FitzHugh–Nagumo model, which reads the point coordinate, at sdim 2 and 3
CASES = [(cls, oid, 0) for cls, oid in MODELS] + [("HeterogeneousFHNModel", "CELL_FHN_HETEROGENEOUS", 2), ("HeterogeneousFHNModel", "CELL_FHN_HETEROGENEOUS", 3)]
CASE_IDS = [c[0] + ("-sdim%d" % c[2] if c[2] else "") for c in CASES]
RL_CASES = [c for c in CASES if c[0] in ("PCG2019", "TT06", "ORd2011")]


def make_model(tb, cls, sdim):
    if cls == "HeterogeneousFHNModel":
        return tb.HeterogeneousFHNModel(e0=0.02, gx=0.03, gy=-0.01, gz=0.02 if sdim == 3 else 0.0)
    return getattr(tb, cls)()


def start_values(tb, model, n, layout, sdim, seed=42):
    """(flat start array, coordinates or None).  TT06: one point exactly at V = −40 mV, the ≥ side of the h / j branch."""
    rng = np.random.default_rng(seed)
    pts = initial_points(tb, model, n, rng)
    if model.nstates == 19:
        pts[1, 0] = -40.0
    xs = rng.uniform(-1, 1, size=(n, sdim)).astype(np.float32) if sdim else None
    return (np.ascontiguousarray(pts.T) if layout == "SOA" else pts).ravel().copy(), xs


def off_the_sodium_gate_branch(model, ref, n, layout):
    """TT06 switches the h and j gate rates at V = −40 mV: no reference point within 10⁻⁶ mV of it (a rounding could then put the device on the other side,
    a legitimate difference that would hide a wrong one), except points placed exactly there"""
    if model.nstates != 19:
        return
    V = ref.reshape(19, n)[0] if layout == "SOA" else ref.reshape(n, 19)[:, 0]
    near = np.abs(V + 40.0) < 1e-6
    assert not (near & (V != -40.0)).any(), V[near]


def oracle_step(oracle, oid, model, ref, n, layout, xs, t, dt, substeps=1, thr=0.0):
    code = getattr(oracle, "LAYOUT_" + layout)
    if xs is not None:
        return oracle.reaction_step_x(oid, model.params, ref, n, xs, code, t=t, dt=dt, substeps=substeps, threshold=thr)
    return oracle.reaction_step(oid, model.params, ref, n, code, t=t, dt=dt, substeps=substeps, threshold=thr)


ORD_F_RT = 96485.0 / (8314.0 * 310.0)              # F/RT of the O'Hara–Rudy model, 1/mV
ORD_CONSTANT_FIELD_SLOTS = (3, 10, 11)             # s_PCa (ICaL, ICaNa, ICaK), s_PNab, s_PCab: the scalings of the constant-field fluxes


def constant_field_allowance(oracle, oid, model, ref, n, layout):
    """What two correct Float64 evaluations of the O'Hara–Rudy rates may differ by at the points of `ref` (left unchanged) beyond the threshold, entry by
    entry, in units of a rate; zero for every other model.

    The expression is the denominator exp(z·x) − 1 of the constant-field fluxes PhiCaL, PhiCaNa, PhiCaK, INab and ICab (z = 1, 2; x = V·F/RT), with V
    moved to 10⁻⁷ mV where |V| < 10⁻⁷ mV (oracle and kernel alike; test_gpu_parity.initial_points puts one point at V = 0 exactly).  Every evaluation rounds
    exp(z·x) or exp(x) to Float64 before it subtracts 1: the oracle's exp(z·x) is within 1 ulp of 1 (libm), the kernel's exp_b(x) within 0.862 ulp
    (tb_math.hpp), squared for z = 2 (1.72 ulp; the product and the subtraction contract to one exact fused multiply-add under -ffp-contract=fast).  The two
    denominators differ by up to (1 + 1.72)·2⁻⁵² absolutely, that is 1.36·2⁻⁵²/|x| of their value z·x for z = 2 and 1.86·2⁻⁵²/|x| for z = 1: κ(V) = 2·2⁻⁵²/|x|
    bounds both.  At the moved point x = 3.74·10⁻⁹ and κ = 1.2·10⁻⁷ (the oracle itself is 1.0·10⁻⁸ off the exact expm1 there); at |V| = 1 mV κ = 1.2·10⁻¹⁴.
    Each flux carries that relative difference into every rate it enters, linearly: the part of a rate that comes from one flux is the oracle's rate
    minus the oracle's rate with that flux's scaling parameter set to zero (the rates are affine in the scalings).  The allowance is κ(V) times the sum
    of the magnitudes of the three parts, per point and per state: nothing at the points and states that have no such part."""
    if model.nstates != 41:
        return np.zeros_like(ref)
    code = getattr(oracle, "LAYOUT_" + layout)

    def rates(p):
        return oracle.reaction_step(oid, p, ref.copy(), n, code, t=0.0, dt=0.0)

    full, part = rates(model.params), np.zeros_like(ref)
    for slot in ORD_CONSTANT_FIELD_SLOTS:
        p = model.params.copy()
        p[slot] = 0.0
        part += np.abs(full - rates(p))
    V = ref.reshape(41, n)[0] if layout == "SOA" else ref.reshape(n, 41)[:, 0]
    kappa = 2.0 * 2.0 ** -52 / np.abs(np.where(np.abs(V) < 1e-7, 1e-7, V) * ORD_F_RT)
    return (part.reshape(41, n) * kappa[None, :] if layout == "SOA" else part.reshape(n, 41) * kappa[:, None]).ravel()


def figures(label, got, ref, model, n, layout, tol, allow=None):
    """prints the worst per-state figure (and which state), returns the figures.  `allow`: an absolute allowance entry by entry (constant_field_allowance),
    taken off the difference before it is measured against the state's scale"""
    diff = np.abs(np.asarray(got, dtype=np.float64) - ref)
    e = per_state_ratio(diff if allow is None else np.maximum(diff - allow, 0.0), ref, model.nstates, n, layout)
    k = int(np.argmax(e))                                # (a NaN counts as the largest)
    note = ""
    if allow is not None and allow.max() > 0.0:
        a = per_state_ratio(allow, ref, model.nstates, n, layout)
        note = "; constant-field allowance up to %.1e of a state's scale (state %d), raw worst figure %.3e" % (
            a.max(), int(np.argmax(a)), per_state_ratio(diff, ref, model.nstates, n, layout).max())
    print("%s: worst state %d (%s) %.3e, threshold %.0e%s" % (label, k, model.state_symbols[k], e[k], tol, note))
    return e


def layout_of(tb, layout):
    return tb.StateBlockedLayout() if layout == "SOA" else tb.PointBlockedLayout()


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("cls,oid,sdim", CASES, ids=CASE_IDS)
def test_forward_euler_per_state(tb, oracle, device, cls, oid, sdim, layout, n):
    """k_reaction<MODEL, layout, WRITE_DU, double>: states and rates after 1 and after 20 steps, with du materialised and without"""
    model, oid = make_model(tb, cls, sdim), getattr(oracle, oid)
    host, xs = start_values(tb, model, n, layout, sdim)
    dt = FE_DT[model.nstates]
    f = tb.PointwiseODEFunction(n, model, x=xs, layout=layout_of(tb, layout))
    ref, refs, allow_u = host.copy(), {}, np.zeros_like(host)
    for step in range(20):
        off_the_sodium_gate_branch(model, ref, n, layout)
        allow_du = constant_field_allowance(oracle, oid, model, ref, n, layout)        # zero but for O'Hara–Rudy
        allow_u += dt * allow_du                                                         # what a step adds to a state; carried on as it is (20 steps = 0.04 ms)
        du_ref = oracle_step(oracle, oid, model, ref, n, layout, xs, step * dt, dt)
        if step in (0, 19):
            refs[step + 1] = (ref.copy(), du_ref.copy(), allow_u.copy(), allow_du)
    fails = []
    for keep_du in (True, False):
        cache = tb.setup_solver_cache(f, tb.ForwardEulerCellSolver(device), u=device.to_device(host.copy()), keep_du=keep_du)
        for step in range(20):
            assert tb.perform_step(f, cache, step * dt, dt) is True
            if step + 1 in refs:
                tag = "%s-%d %s n %d forward Euler %d step(s) du %s" % (cls, sdim, layout, n, step + 1, keep_du)
                eu = figures(tag + " u", cache.un.to_host(), refs[step + 1][0], model, n, layout, TOL_U, refs[step + 1][2])
                fails += [(tag, "u", k, eu[k]) for k in range(model.nstates) if not eu[k] < TOL_U]
                if keep_du:
                    edu = figures(tag + " du", cache.du.to_host(), refs[step + 1][1], model, n, layout, TOL_DU, refs[step + 1][3])
                    fails += [(tag, "du", k, edu[k]) for k in range(model.nstates) if not edu[k] < TOL_DU]
    assert fails == []


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("cls,oid,sdim", CASES, ids=CASE_IDS)
def test_float32_storage_per_state(tb, oracle, device, cls, oid, sdim, layout, n):
    """k_reaction<MODEL, layout, true, float> (tb_reaction_step_f32, every model it accepts): one call with 1 sub-step and one with 4 (threshold 0: every
    point sub-steps).  States are read from and rounded to Float32 once per call, the arithmetic is Float64: against the oracle's Float64 step from the same
    Float32 inputs an entry may differ by that one rounding (2⁻²⁴ relative) plus the threshold times its state's scale."""
    lib, check = tb.lib(), tb._lib.check
    model, oid = make_model(tb, cls, sdim), getattr(oracle, oid)
    ns = model.nstates
    host, xs = start_values(tb, model, n, layout, sdim)
    host32 = host.astype(np.float32)
    dt = FE_DT[ns]
    dxs = None
    if xs is not None:
        dxs = tb.DeviceVector(device, xs.size, dtype=np.float32)
        dxs.copy_from_host(xs.ravel())
    fails = []
    for substeps in (1, 4):
        ref = host32.astype(np.float64)
        off_the_sodium_gate_branch(model, ref, n, layout)
        allow_du = constant_field_allowance(oracle, oid, model, ref, n, layout)        # of the first evaluation; the later sub-steps have left V = 0
        du_ref = oracle_step(oracle, oid, model, ref, n, layout, xs, 0.0, dt, substeps=substeps, thr=0.0)
        u32, du32 = device.to_device(host32.copy()), tb.DeviceVector(device, n * ns, dtype=np.float32)
        check(lib.tb_reaction_step_f32(device.h, model.model_id, model.params.ctypes.data_as(tb._lib.c_dp), len(model.params), u32.ptr, du32.ptr, n, ns,
                                       0 if layout == "SOA" else 1, dxs.ptr if dxs is not None else None, sdim, 0.0, dt, substeps, 0.0))
        for name, got, r, tol, allow in (("u", u32.to_host(), ref, TOL_U, dt * allow_du), ("du", du32.to_host(), du_ref, TOL_DU, allow_du)):
            got = got.astype(np.float64)
            assert np.isfinite(got).all()
            beyond = np.maximum(np.abs(got - r) - 2.0 ** -24 * np.abs(r) - allow, 0.0)  # what is left of the difference beyond the one rounding
            e = per_state_ratio(beyond, r, ns, n, layout)
            k = int(np.argmax(e))
            print("%s-%d %s n %d Float32 %d sub-step(s) %s: beyond the rounding, worst state %d (%s) %.3e, threshold %.0e" % (
                cls, sdim, layout, n, substeps, name, k, model.state_symbols[k], e[k], tol))
            fails += [(substeps, name, j, e[j]) for j in range(ns) if not e[j] <= tol]
    assert fails == []


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("cls,oid,sdim", CASES, ids=CASE_IDS)
def test_adaptive_substepper_per_state(tb, oracle, device, cls, oid, sdim, layout, n):
    """k_reaction with 7 sub-steps where |dφₘ/dt| reaches the threshold, 5 steps.  At the start of every step no reference point is within 10⁻⁶·threshold of
    the threshold (a rounding could otherwise move a point to the other branch: a legitimate difference that would hide a wrong one), and the first step
    has points on both branches."""
    model, oid = make_model(tb, cls, sdim), getattr(oracle, oid)
    ns = model.nstates
    host, xs = start_values(tb, model, n, layout, sdim, seed=7)
    dt, thr = ADAPTIVE_DT[ns], ADAPTIVE_THRESHOLD[ns]
    f = tb.PointwiseODEFunction(n, model, x=xs, layout=layout_of(tb, layout))
    cache = tb.setup_solver_cache(f, tb.AdaptiveForwardEulerSubstepper(device, substeps=7, reaction_threshold=thr), u=device.to_device(host.copy()))
    ref, allow_u = host.copy(), np.zeros_like(host)
    for step in range(5):
        off_the_sodium_gate_branch(model, ref, n, layout)
        allow_du = constant_field_allowance(oracle, oid, model, ref, n, layout)
        allow_u += dt * allow_du          # the first evaluation of the step, at the weight of a whole step; a sub-stepped point has left V = 0 after it
        rate = np.abs(phi_rates(oracle, oid, model.params, ref, ns, n, layout, model.phi_index, xs))
        assert np.abs(rate - thr).min() >= 1e-6 * thr, (step, np.abs(rate - thr).min())
        if step == 0:
            print("%s-%d %s n %d adaptive: %d points take one step, %d sub-step" % (cls, sdim, layout, n, (rate < thr).sum(), (rate >= thr).sum()))
            assert (rate < thr).any() and (rate >= thr).any()
        assert tb.perform_step(f, cache, step * dt, dt) is True
        du_ref = oracle_step(oracle, oid, model, ref, n, layout, xs, step * dt, dt, substeps=7, thr=thr)
    tag = "%s-%d %s n %d adaptive 7 sub-steps, 5 steps" % (cls, sdim, layout, n)
    eu = figures(tag + " u", cache.un.to_host(), ref, model, n, layout, TOL_U, allow_u)
    edu = figures(tag + " du", cache.du.to_host(), du_ref, model, n, layout, TOL_DU, allow_du)
    assert (eu < TOL_U).all(), eu
    assert (edu < TOL_DU).all(), edu


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("cls,oid,sdim", RL_CASES, ids=[c[0] for c in RL_CASES])
def test_rush_larsen_per_state(tb, oracle, device, cls, oid, sdim, layout, n):
    """k_reaction_rl (gates by the exact solution for frozen φₘ through expm1_b, the other states forward Euler) after 1 and after 5 steps at the step sizes
    of test_rush_larsen_tt06 / _ord2011_parity / _pcg2019_parity"""
    model, oid = make_model(tb, cls, sdim), getattr(oracle, oid)
    host, _ = start_values(tb, model, n, layout, 0)
    dt = RL_DT[model.nstates]
    f = tb.PointwiseODEFunction(n, model, layout=layout_of(tb, layout))
    cache = tb.setup_solver_cache(f, tb.RushLarsenCellSolver(device), u=device.to_device(host.copy()), keep_du=False)
    ref, fails, allow_u = host.copy(), [], np.zeros_like(host)
    for step in range(5):
        off_the_sodium_gate_branch(model, ref, n, layout)
        allow_u += dt * constant_field_allowance(oracle, oid, model, ref, n, layout)      # the states these fluxes enter are not gates: forward Euler
        assert tb.perform_step(f, cache, step * dt, dt) is True
        oracle.reaction_step_rl(oid, model.params, ref, n, getattr(oracle, "LAYOUT_" + layout), t=step * dt, dt=dt)
        if step in (0, 4):
            eu = figures("%s %s n %d Rush–Larsen %d step(s) u" % (cls, layout, n, step + 1), cache.un.to_host(), ref, model, n, layout, TOL_U, allow_u)
            fails += [(step + 1, k, eu[k]) for k in range(model.nstates) if not eu[k] < TOL_U]
    assert fails == []


@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("cls,oid", MODELS)
def test_fused_tangent_step_per_state(tb, oracle, device, cls, oid, layout, n):
    """tb_reaction_step_rtc: the forward-Euler step with the reaction tangent reduced inside the kernel, no du array.  States per state; R against the
    oracle's signed maximum of the φₘ rate at the suite's bound for a rate."""
    model, oid = make_model(tb, cls, 0), getattr(oracle, oid)
    ns = model.nstates
    host, _ = start_values(tb, model, n, layout, 0)
    dt = FE_DT[ns]
    f = tb.PointwiseODEFunction(n, model, layout=layout_of(tb, layout))
    cache = tb.setup_solver_cache(f, tb.ForwardEulerCellSolver(device), u=device.to_device(host.copy()), keep_du=False)
    ref = host.copy()
    off_the_sodium_gate_branch(model, ref, n, layout)
    allow_u = dt * constant_field_allowance(oracle, oid, model, ref, n, layout)
    du_ref = oracle_step(oracle, oid, model, ref, n, layout, None, 0.0, dt)
    ok, R = tb.perform_step_with_reaction_tangent(f, cache, 0.0, dt)
    sl = du_ref.reshape(ns, n)[model.phi_index] if layout == "SOA" else du_ref.reshape(n, ns)[:, model.phi_index]
    eu = figures("%s %s n %d fused tangent step u" % (cls, layout, n), cache.un.to_host(), ref, model, n, layout, TOL_U, allow_u)
    print("%s %s n %d fused tangent step R %.17g against %.17g (relative difference %.3e)" % (cls, layout, n, R, sl.max(), abs(R - sl.max()) / abs(sl.max())))
    assert ok is True
    assert (eu < TOL_U).all(), eu
    np.testing.assert_allclose(R, sl.max(), rtol=1e-10)
