"""What the per-state norm of the reaction parity tests (helpers.per_state_err) sees that the global one (helpers.rel_err) cannot, and why the project's
thresholds (1e-12 for states, 1e-10 for rates) can be asked of every state separately.  CPU oracle only: a kernel that is wrong in one constant is stood in
for by the oracle with that parameter scaled by 1.001.

rel_err divides the largest error of ALL states by the largest reference entry of ALL states: K_i ≈ 140 and V ≈ 86 in TT06 beside Ca_i and Ca_ss ≈ 7·10⁻⁵,
K ≈ 145 beside Ca ≈ 10⁻⁴ and the release fluxes ≈ 10⁻³ in O'Hara–Rudy.  An error of one part in a thousand in a calcium flux is 10⁻⁷ of such a state after
20 steps and 10⁻¹⁵ of the array's largest entry.

The GPU half is tests/test_reaction_per_state_gpu.py."""
import numpy as np
import pytest

from helpers import ADAPTIVE_DT, ADAPTIVE_THRESHOLD, FE_DT, RL_DT, per_state_err, phi_rates, rel_err
from test_gpu_parity import MODELS, initial_points

TOL_U, TOL_DU = 1e-12, 1e-10                      # the suite's thresholds (test_gpu_parity.TOL; the bound of the materialised rates)
N = 1037                                          # the point count and the seed of test_reaction_forward_euler_parity
VXFER = 35                                        # TT06 parameter slot of the Ca_ss → Ca_i transfer rate
HETERO = ("HeterogeneousFHNModel", "CELL_FHN_HETEROGENEOUS")
HETERO_PARAMS = np.array([0.1, 0.5, 1.0, 0.0, 0.02, 0.03, -0.01, 0.02])       # e(x) = e0 + g·x with all three gradients on (test_reaction_reads_point_coordinates)


class OracleModel:
    """What initial_points reads of a cell model, from the oracle"""

    def __init__(self, oracle, oid_name):
        self.oid = getattr(oracle, oid_name)
        self.params = HETERO_PARAMS.copy() if oid_name == HETERO[1] else oracle.cell_default_params(self.oid)
        self.nstates = oracle.cell_nstates(self.oid)
        self.phi_index = 1 if oid_name == "CELL_ALIEV_PANFILOV" else 0
        self._u0 = oracle.cell_default_state(self.oid, self.params)

    def default_initial_state(self):
        return self._u0.copy()


@pytest.fixture(scope="module")
def cases(oracle):
    """model, start (SOA, flat) and coordinates (heterogeneous FHN only) of every cell model at the points of test_reaction_forward_euler_parity"""
    out = {}
    for cls, oid in MODELS + [HETERO]:
        m = OracleModel(oracle, oid)
        pts = initial_points(None, m, N, np.random.default_rng(42))
        xs = np.random.default_rng(12).uniform(-1, 1, size=(N, 3)).astype(np.float32) if oid == HETERO[1] else None
        out[cls] = (m, np.ascontiguousarray(pts.T).ravel(), xs)
    return out


def forward_euler(oracle, m, params, start, xs, steps=20, substeps=1, thr=0.0, dt=None):
    u, dt = start.copy(), FE_DT[m.nstates] if dt is None else dt
    for s in range(steps):
        if xs is None:
            du = oracle.reaction_step(m.oid, params, u, N, oracle.LAYOUT_SOA, t=s * dt, dt=dt, substeps=substeps, threshold=thr)
        else:
            du = oracle.reaction_step_x(m.oid, params, u, N, xs, oracle.LAYOUT_SOA, t=s * dt, dt=dt, substeps=substeps, threshold=thr)
    return u, du


def rush_larsen(oracle, m, params, start, steps=1):
    u, dt = start.copy(), RL_DT[m.nstates]
    for s in range(steps):
        oracle.reaction_step_rl(m.oid, params, u, N, oracle.LAYOUT_SOA, t=s * dt, dt=dt)
    return u


@pytest.fixture(scope="module")
def sweep(oracle, cases):
    """every parameter slot of every model scaled by 1.001: rows (model, slot, form, global u, global du, worst per-state u, worst per-state du, du changed)"""
    rows = []
    for cls, (m, start, xs) in cases.items():
        ref_u, ref_du = forward_euler(oracle, m, m.params, start, xs)
        ref_rl = rush_larsen(oracle, m, m.params, start) if m.nstates in RL_DT else None
        for slot in range(len(m.params)):
            p = m.params.copy()
            p[slot] *= 1.001
            u, du = forward_euler(oracle, m, p, start, xs)
            rows.append((cls, slot, "FE", rel_err(u, ref_u), rel_err(du, ref_du), per_state_err(u, ref_u, m.nstates, N, "SOA").max(),
                         per_state_err(du, ref_du, m.nstates, N, "SOA").max(), bool((du != ref_du).any())))
            if ref_rl is not None:
                u = rush_larsen(oracle, m, p, start)
                rows.append((cls, slot, "RL", rel_err(u, ref_rl), np.nan, per_state_err(u, ref_rl, m.nstates, N, "SOA").max(), np.nan, bool((u != ref_rl).any())))
    print("\nparameter × 1.001: 20 forward-Euler steps (FE) and one Rush–Larsen step (RL), n = %d; thresholds u %.0e, du %.0e" % (N, TOL_U, TOL_DU))
    print("%-20s %4s %4s %11s %11s %13s %13s" % ("model", "slot", "form", "global u", "global du", "per-state u", "per-state du"))
    for r in rows:
        print("%-20s %4d %4s %11.3e %11.3e %13.3e %13.3e%s" % (r[:7] + ("" if r[7] else "   (no effect)",)))
    return rows


def test_per_state_err_definition():
    """the figure per state, both layouts, the zero-reference rule and a NaN"""
    ref = np.array([[100.0, -200.0, 50.0], [1e-4, 2e-4, -4e-4], [0.0, 0.0, 0.0]])          # 3 states × 3 points
    got = ref.copy()
    got[0, 1] += 2e-10
    got[1, 0] -= 4e-12
    for layout, f in (("SOA", lambda a: a.ravel()), ("AOS", lambda a: np.ascontiguousarray(a.T).ravel())):
        e = per_state_err(f(got), f(ref), 3, 3, layout)
        np.testing.assert_allclose(e, [2e-10 / 200.0, 4e-12 / 4e-4, 0.0], rtol=1e-3)
        bad = got.copy()
        bad[2, 2] = 1e-300                                                                   # a state that is identically zero in the reference must be exactly zero
        assert per_state_err(f(bad), f(ref), 3, 3, layout)[2] == np.inf
        bad[1, 1] = np.nan
        assert np.isnan(per_state_err(f(bad), f(ref), 3, 3, layout)[1])
    assert rel_err(got.ravel(), ref.ravel()) < 1e-11 < per_state_err(got.ravel(), ref.ravel(), 3, 3, "SOA")[1]


def test_vxfer_off_by_a_thousandth_passes_the_global_norm_and_fails_per_state(sweep):
    """TT06 with Vxfer × 1.001, 20 forward-Euler steps: the global figures stay under the thresholds the suite asserts, the per-state ones exceed the same
    thresholds by more than 10³ (measured: global u 2.5e-15, du 4.2e-13; per state u 4.5e-9, du 3.3e-6)"""
    (row,) = [r for r in sweep if r[0] == "TT06" and r[1] == VXFER and r[2] == "FE"]
    _, _, _, gu, gdu, pu, pdu, changed = row
    print("TT06 Vxfer × 1.001: global u %.3e du %.3e, per state u %.3e du %.3e" % (gu, gdu, pu, pdu))
    assert changed
    assert gu < TOL_U and gdu < TOL_DU
    assert pu >= 1e3 * TOL_U and pdu >= 1e3 * TOL_DU


def test_no_slot_is_seen_by_the_global_norm_and_missed_per_state(sweep):
    """the per-state norm flags every parameter slot the global norm flags (of those that change any rate at all), and more of them"""
    def flagged(u, du, tu=TOL_U, tdu=TOL_DU):
        return bool(u >= tu or (not np.isnan(du) and du >= tdu))

    active = [r for r in sweep if r[7]]
    assert len(active) > 100
    missed = [r[:3] for r in active if flagged(r[3], r[4]) and not flagged(r[5], r[6])]
    only_per_state = [r[:3] for r in active if flagged(r[5], r[6]) and not flagged(r[3], r[4])]
    unseen = [r[:3] for r in active if not flagged(r[5], r[6])]
    print("%d active rows: %d seen per state only, %d seen by neither norm: %s" % (len(active), len(only_per_state), len(unseen), unseen))
    assert missed == []
    assert ("TT06", VXFER, "FE") in only_per_state


def one_ulp(rng, a):
    """every non-zero entry moved to one of its two neighbours in Float64 (a relative change of at most 2⁻⁵²), zeros kept"""
    a = np.asarray(a, dtype=np.float64)
    moved = np.nextafter(a, np.where(rng.integers(0, 2, a.shape) == 1, np.inf, -np.inf))
    return np.where(a != 0.0, moved, a)


def test_reference_spread_under_one_ulp_perturbations_is_far_below_the_thresholds(oracle, cases):
    """The condition that makes a per-state threshold legitimate, checked on the reference alone: states and parameters perturbed by one unit in the last
    place (8 draws) move no state of the oracle's result by more than 1/50 of the state threshold relative to that state's scale, for every model and every
    stepper form the GPU tests compare (nor any rate by more than 1/50 of the rate threshold).  A device whose functions are good to 2 ulp each then has the
    other 49/50 for itself.  The sub-stepper's branch is kept fixed: no point of the unperturbed run is within 10⁻⁶·threshold of the threshold."""
    worst_u, worst_du = 0.0, 0.0
    print()
    for cls, (m, start, xs) in cases.items():
        ns, thr, adt = m.nstates, ADAPTIVE_THRESHOLD[m.nstates], ADAPTIVE_DT[m.nstates]
        forms = {"FE 20": lambda p, u: forward_euler(oracle, m, p, u, xs),
                 "adaptive 7×5": lambda p, u: forward_euler(oracle, m, p, u, xs, steps=5, substeps=7, thr=thr, dt=adt)}
        if ns in RL_DT:
            forms["RL 1"] = lambda p, u: (rush_larsen(oracle, m, p, u, 1), None)
            forms["RL 5"] = lambda p, u: (rush_larsen(oracle, m, p, u, 5), None)
        # the branch condition of the sub-stepper on the unperturbed trajectory
        u = start.copy()
        for s in range(5):
            gap = np.abs(np.abs(phi_rates(oracle, m.oid, m.params, u, ns, N, "SOA", m.phi_index, xs)) - thr)
            assert gap.min() >= 1e-6 * thr, (cls, s, gap.min())
            u, _ = forward_euler(oracle, m, m.params, u, xs, steps=1, substeps=7, thr=thr, dt=adt)
        for name, run in forms.items():
            ref_u, ref_du = run(m.params, start)
            rng = np.random.default_rng(2024)
            eu, edu = 0.0, 0.0
            for _ in range(8):
                got_u, got_du = run(one_ulp(rng, m.params), one_ulp(rng, start))
                eu = max(eu, per_state_err(got_u, ref_u, ns, N, "SOA").max())
                if ref_du is not None:
                    edu = max(edu, per_state_err(got_du, ref_du, ns, N, "SOA").max())
            print("%-20s %-13s spread per state: u %.3e%s" % (cls, name, eu, "  du %.3e" % edu if ref_du is not None else ""))
            worst_u, worst_du = max(worst_u, eu), max(worst_du, edu)
            assert eu < TOL_U / 50
            assert edu < TOL_DU / 50
    print("worst: u %.3e (bound %.1e), du %.3e (bound %.1e)" % (worst_u, TOL_U / 50, worst_du, TOL_DU / 50))
