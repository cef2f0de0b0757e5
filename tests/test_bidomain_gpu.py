"""Parabolic–elliptic bidomain on the device (csrc/tb_bidomain.hip, thunderbolt.jl_amd/bidomain.py) against the dense NumPy reference of
tests/bidomain_reference.py: the fused block product row by row, the grounded block-Jacobi PCG by an a-posteriori bound, the monodomain limit against
the existing BackwardEulerStage, the extracellular source, Δt changes, the unchanged LieTrotterGodunov loop, capture and refusals."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bidomain_reference as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUNDS = {"one": (0,), "three": (0, 7, 13)}
# 20-step LieTrotterGodunov loop on the 16 × 4 × 4 slab, device against the dense-solve-plus-oracle reference loop, max over all entries of the state,
# solver rtol 1e-12, atol 0.  The stimulus adds 0.3 per step for three steps (the stage adds `source` per step, as BackwardEulerStage does), so φₘ stays
# inside FitzHugh–Nagumo's range: a stimulus of 3 per step for ten steps drove φₘ to 5.9, where forward Euler on the cubic amplifies a 1e-12 solve error
# to 1e-9 in both loops and the loop measures the cell model's conditioning instead of the stage (per-step figures in DESIGN.md §4.6e).  Measured on an
# MI355X: the monodomain loop (the parent commit's path, the yardstick) deviates by 1.05e-13; the bidomain loop is allowed ten times that — twice the
# unknowns on a worse-conditioned block.  Measured bidomain: state 4.90e-14, φₑ 3.98e-14.
LOOP_MONODOMAIN_DEVIATION = 1.05e-13
LOOP_TOLERANCE = 10.0 * LOOP_MONODOMAIN_DEVIATION


def strict_solver(tb, n):
    return tb.BackwardEulerSolver(rtol=1e-12, atol=0.0, maxiter=8 * n)


@pytest.fixture(scope="module")
def cases(tb, device, oracle):
    """per mesh: grid, dof handler, pattern, the oracle's (M, Kᵢ, Kₑ) on the host and on the device — computed once, never written"""
    cache = {}

    def get(name):
        if name not in cache:
            g, dh, sp = ref.build_mesh(tb, name)
            host = ref.oracle_matrices(tb, oracle, g, dh, sp)
            dmesh = dh.device_mesh(device)
            cache[name] = dict(g=g, dh=dh, sp=sp, host=host, dev=tuple(device.to_device(a) for a in host), pattern=dmesh.pattern(sp))
        return cache[name]
    return get


def grounded_system(tb, device, case, ground, dt=ref.DT):
    sp, (M, Ki, Ke) = case["sp"], case["host"]
    n = case["dh"].ndofs
    flags = np.zeros(n, dtype=np.uint8)
    flags[list(ground)] = 1
    gd = ref.ground_diagonal(sp.rowptr, sp.colidx, Ki, Ke, dt)
    system = tb.BidomainSystem(case["pattern"])
    system.set_matrices(*case["dev"], dt, device.to_device(flags), gd)
    return system, ref.block_matrix(sp.rowptr, sp.colidx, M, Ki, Ke, dt, ground, gd), gd


# ------------------------------------------------------------------------------------------------ 1. the product
@pytest.mark.parametrize("name,ground", [("hex_5x4x3", "one"), ("hex_5x4x3", "three"), ("tet_3x3x2", "one"), ("quad_7x5", "three"), ("hex_11x10x9", "three")])
def test_product_row_by_row(tb, device, cases, name, ground):
    """|y − A x|ᵢ ≤ 1e-13 Σⱼ|aᵢⱼ||xⱼ|: at most 2·27 products per row, γ₅₄ ≈ 6e-15, the rest margin for the fused multiply-adds of the combine pass"""
    case = cases(name)
    n = case["dh"].ndofs
    system, A, gd = grounded_system(tb, device, case, GROUNDS[ground])
    x = np.random.default_rng(11).uniform(-1.0, 1.0, 2 * n)                    # blocked (φₘ; φₑ)
    dx, dy = device.to_device(ref.interleave(x)), device.zeros(2 * n)
    system.apply(dx, dy)
    y1 = dy.to_host()
    dy.fill_zero()
    system.apply(dx, dy)
    y2 = dy.to_host()
    assert np.array_equal(y1, y2)
    y, want = ref.deinterleave(y1), A @ x
    ratio = np.abs(y - want) / ref.row_bound(A, x)
    print("%s ground %s: max |y - Ax|_i / sum_j |a_ij||x_j| = %.3e (allowed 1e-13)" % (name, ground, ratio.max()))
    assert ratio.max() <= 1e-13
    for g in GROUNDS[ground]:
        assert abs(y[n + g] - gd * x[n + g]) <= 1e-13 * abs(gd * x[n + g])


def test_stored_operator_is_the_host_formula_bit_for_bit(tb, device, cases):
    """A eⱼ is a column of the stored operator, exactly (one product with 1.0 per row, the rest zeros): it has the bits of the dense reference, whose
    entries are M − Δt·Kᵢ, −Δt·Kᵢ and −Δt·(Kᵢ + Kₑ) with every operation rounded on its own.  On a matrix of condition 1e5 an ε-sized disagreement
    between the combine pass and the host shows as 1e-11 in a solution."""
    case = cases("hex_5x4x3")
    n = case["dh"].ndofs
    system, A, _ = grounded_system(tb, device, case, GROUNDS["three"])
    dy = device.zeros(2 * n)
    for col in (0, 1, 7, 64, n - 1, n + 1, n + 7, n + 63, n + 64, 2 * n - 1):
        e = np.zeros(2 * n)
        e[col] = 1.0
        system.apply(device.to_device(ref.interleave(e)), dy)
        assert np.array_equal(ref.deinterleave(dy.to_host()), A[:, col]), col


# ------------------------------------------------------------------------------------------------ 2. the solve
@pytest.mark.parametrize("name", ref.SOLVE_MESHES)
@pytest.mark.parametrize("ground", ["one", "three"])
def test_solve_against_the_dense_solution(tb, device, cases, name, ground):
    """‖x − x*‖₂ ≤ (‖b − A x‖₂ + 4ε‖ |A||x| ‖₂)/λ_min(A), residual and λ_min from the dense reference matrix"""
    case = cases(name)
    n = case["dh"].ndofs
    system, A, _ = grounded_system(tb, device, case, GROUNDS[ground])
    b = np.random.default_rng(12).uniform(-1.0, 1.0, 2 * n)
    b[n + np.asarray(GROUNDS[ground])] = 0.0
    db = device.to_device(ref.interleave(b))
    runs = []
    for _ in range(2):
        dx = device.zeros(2 * n)
        its, res = system.solve(db, dx, rtol=1e-12, atol=0.0, maxiter=8 * n)
        runs.append((dx.to_host(), its, res))
    (x1, its, res), (x2, its2, res2) = runs
    assert np.array_equal(x1, x2) and (its, res) == (its2, res2)
    tol = C.c_double()
    tb.check(tb.lib().tb_solver_last_tolerance(case["pattern"].h, C.byref(tol)))
    x, xs = ref.deinterleave(x1), np.linalg.solve(A, b)
    err, bound = np.linalg.norm(x - xs), ref.error_bound(A, b, x)
    print("%s ground %s: %d iterations, reported |r| %.3e <= tolerance %.3e, |x - x*| %.3e <= bound %.3e (|x*| %.3e)" % (name, ground, its, res, tol.value, err, bound,
                                                                                                                      np.linalg.norm(xs)))
    assert res <= tol.value
    assert abs(tol.value - 1e-12 * np.linalg.norm(b)) <= 1e-12 * tol.value                         # x₀ = 0: ‖r₀‖ = ‖b‖ to the rounding of the sum
    assert tb.solve_converged(case["pattern"], res)
    assert err <= bound
    assert np.all(x[n + np.asarray(GROUNDS[ground])] == 0.0)


# ------------------------------------------------------------------------------------------------ stages on device-assembled operators
def make_stage(tb, device, dh, sp, kappa_i, kappa_e, ground, n, **kw):
    one = tb.ConstantCoefficient(1.0)
    Di = tb.ConductivityToDiffusivityCoefficient(tb.ConstantCoefficient(kappa_i), one, one)
    De = tb.ConductivityToDiffusivityCoefficient(tb.ConstantCoefficient(kappa_e), one, one)
    return tb.BidomainBackwardEulerStage(kw.pop("solver", None) or strict_solver(tb, n), tb.PerColorAssemblyStrategy(device), dh, Di, De, list(ground), pattern=sp, **kw)


def stage_dense(stage, dt):
    sp = stage.sp
    M, Ki, Ke = stage.M.A.to_host(), stage.Ki.A.to_host(), stage.Ke.A.to_host()
    return ref.block_matrix(sp.rowptr, sp.colidx, M, Ki, Ke, dt, stage.ground_dofs, stage.ground_diag(dt)), ref.dense_of_csr(sp.rowptr, sp.colidx, M)


def test_monodomain_limit_on_the_device(tb, device):
    """κₑ = 2κᵢ: one BidomainBackwardEulerStage step against one step of the existing BackwardEulerStage with D = ⅔Dᵢ from the same φₘ — each side
    held to its own dense solution (device-assembled matrices read back), the two φₘ compared by the sum of the two bounds"""
    g, dh, sp = ref.build_mesh(tb, "hex_5x4x3")
    n = dh.ndofs
    phi0 = np.random.default_rng(13).uniform(-1.0, 1.0, n)
    stage = make_stage(tb, device, dh, sp, ref.KAPPA_I, 2.0 * ref.KAPPA_I, (0,), n)
    phi = device.to_device(phi0)
    assert stage.perform_step(phi, 0.0, ref.DT)
    A, Md = stage_dense(stage, ref.DT)
    b = np.concatenate([Md @ phi0, np.zeros(n)])
    x = np.concatenate([phi.to_host(), stage.phi_e.to_host()])
    bound_bi, err_bi = ref.error_bound(A, b, x), np.linalg.norm(x - np.linalg.solve(A, b))
    one = tb.ConstantCoefficient(1.0)
    mono = tb.BackwardEulerStage(strict_solver(tb, n), tb.PerColorAssemblyStrategy(device), dh,
                                 tb.ConductivityToDiffusivityCoefficient(tb.ConstantCoefficient((2.0 / 3.0) * ref.KAPPA_I), one, one), None, sp)
    phi2 = device.to_device(phi0)
    assert mono.perform_step(phi2, 0.0, ref.DT)
    Am = ref.heat_matrix(sp.rowptr, sp.colidx, mono.M.A.to_host(), mono.K.A.to_host(), ref.DT)
    bm = ref.dense_of_csr(sp.rowptr, sp.colidx, mono.M.A.to_host()) @ phi0
    xm = phi2.to_host()
    bound_mono, err_mono = ref.error_bound(Am, bm, xm), np.linalg.norm(xm - np.linalg.solve(Am, bm))
    diff = np.linalg.norm(x[:n] - xm)
    print("bidomain: %d iterations, error %.3e <= bound %.3e; monodomain: %d iterations, error %.3e <= bound %.3e; |phi_m - phi_m(mono)| %.3e <= %.3e"
          % (stage.last_iters, err_bi, bound_bi, mono.last_iters, err_mono, bound_mono, diff, bound_bi + bound_mono))
    assert err_bi <= bound_bi and err_mono <= bound_mono
    assert diff <= bound_bi + bound_mono


def test_it_is_not_the_monodomain_in_disguise(tb, device, cases):
    """unequal anisotropy ratios: φₘ⁺ is no monodomain step for any scalar multiple of Dᵢ tried — the harmonic means along (3·2/5 : 3) and across
    (1·1.5/2.5 : 1) the fibre — by more than 100 × the bound of the solve test; φₑ is non-zero away from the ground"""
    case = cases("hex_5x4x3")
    sp, (M, Ki, Ke), n = case["sp"], case["host"], case["dh"].ndofs
    system, A, _ = grounded_system(tb, device, case, (0,))
    phi0 = np.random.default_rng(14).uniform(-1.0, 1.0, n)
    b = np.concatenate([ref.dense_of_csr(sp.rowptr, sp.colidx, M) @ phi0, np.zeros(n)])
    dx = device.to_device(ref.interleave(np.concatenate([phi0, np.zeros(n)])))
    system.solve(device.to_device(ref.interleave(b)), dx, rtol=1e-12, atol=0.0, maxiter=8 * n)
    x = ref.deinterleave(dx.to_host())
    bound = ref.error_bound(A, b, x)
    for s in (0.4, 0.6):
        mono = np.linalg.solve(ref.heat_matrix(sp.rowptr, sp.colidx, M, s * Ki, ref.DT), b[:n])
        d = np.linalg.norm(x[:n] - mono)
        print("D = %.1f D_i: |phi_m(bidomain) - phi_m(monodomain)| = %.3e, 100 x bound = %.3e" % (s, d, 100 * bound))
        assert d > 100.0 * bound
    away = np.setdiff1d(np.arange(n), [0])
    assert np.abs(x[n + away]).max() > 1e-3 * np.abs(x[:n]).max() and x[n] == 0.0


def test_extracellular_source(tb, device):
    """a balanced pair of nodal currents gives the dense reference's φₑ; an unbalanced one is refused when the stage is built"""
    g, dh, sp = ref.build_mesh(tb, "hex_5x4x3")
    n = dh.ndofs
    Ie = np.zeros(n)
    Ie[5], Ie[n - 3] = 0.25, -0.25
    stage = make_stage(tb, device, dh, sp, ref.KAPPA_I, ref.KAPPA_E, (0,), n, source_e=Ie)
    phi = device.zeros(n)
    assert stage.perform_step(phi, 0.0, ref.DT)
    A, _ = stage_dense(stage, ref.DT)
    b = np.concatenate([np.zeros(n), Ie])
    x, xs = np.concatenate([phi.to_host(), stage.phi_e.to_host()]), np.linalg.solve(A, b)
    err, bound = np.linalg.norm(x - xs), ref.error_bound(A, b, x)
    print("balanced pair: %d iterations, |x - x*| %.3e <= bound %.3e, phi_e range [%.3e, %.3e]" % (stage.last_iters, err, bound, x[n:].min(), x[n:].max()))
    assert err <= bound and np.abs(xs[n:]).max() > 0.0 and np.linalg.norm(x[n:] - xs[n:]) <= bound
    Ie[5] = 0.26
    with pytest.raises(ValueError, match="sums to"):
        make_stage(tb, device, dh, sp, ref.KAPPA_I, ref.KAPPA_E, (0,), n, source_e=Ie)


def test_dt_change_rebuilds_the_operator_and_the_same_dt_does_not(tb, device):
    g, dh, sp = ref.build_mesh(tb, "hex_5x4x3")
    n = dh.ndofs
    phi0 = np.random.default_rng(15).uniform(-1.0, 1.0, n)
    stage = make_stage(tb, device, dh, sp, ref.KAPPA_I, ref.KAPPA_E, (0, 7, 13), n)
    phi = device.to_device(phi0)
    assert stage.generation == 0
    assert stage.perform_step(phi, 0.0, 0.1) and stage.generation == 1 and stage.dt_last == 0.1
    assert stage.perform_step(phi, 0.1, 0.1) and stage.generation == 1
    mid_m, mid_e = phi.to_host(), stage.phi_e.to_host()
    assert stage.perform_step(phi, 0.2, 0.05) and stage.generation == 2 and stage.dt_last == 0.05
    fresh = make_stage(tb, device, dh, sp, ref.KAPPA_I, ref.KAPPA_E, (0, 7, 13), n)
    phi2 = device.to_device(mid_m)
    fresh.phi_e.copy_from_host(mid_e)                                       # the same initial guess: the same iterates
    assert fresh.perform_step(phi2, 0.2, 0.05) and fresh.generation == 1
    assert np.array_equal(phi.to_host(), phi2.to_host()) and np.array_equal(stage.phi_e.to_host(), fresh.phi_e.to_host())
    A, Md = stage_dense(stage, 0.05)
    b = np.concatenate([Md @ mid_m, np.zeros(n)])
    x = np.concatenate([phi.to_host(), stage.phi_e.to_host()])
    assert np.linalg.norm(x - np.linalg.solve(A, b)) <= ref.error_bound(A, b, x)


# ------------------------------------------------------------------------------------------------ 7. the time loop
def loop_deviation(tb, device, oracle, bidomain, steps=20, dt=0.1):
    """max |device − reference| over the state (and φₑ) after `steps` LieTrotterGodunov steps on the 16 × 4 × 4 slab: FitzHugh–Nagumo, forward Euler
    cell solver, a corner stimulus through `source`; the reference loop is a dense solve (iteratively refined, so
    that its own error stays below what it measures) plus oracle.reaction_step per step"""
    g = tb.generate_mesh(tb.Hexahedron, (16, 4, 4), (0.0, 0.0, 0.0), (4.0, 1.0, 1.0))
    dh = tb.DofHandler(g)
    sp = tb.allocate_matrix(dh)
    n = dh.ndofs
    solver = strict_solver(tb, n)                                          # the tolerances of every solve test here: rtol 1e-12, atol 0
    stim = tb.LinearIntegrator(tb.AnalyticalCoefficient(lambda x, t: 0.3 * (t <= 0.35) * (x[0] <= 0.5 and x[1] <= 0.5 and x[2] <= 0.5)))
    strategy = tb.PerColorAssemblyStrategy(device)
    one = tb.ConstantCoefficient(1.0)
    Di = tb.ConductivityToDiffusivityCoefficient(tb.ConstantCoefficient(ref.KAPPA_I * 10.0), one, one)
    De = tb.ConductivityToDiffusivityCoefficient(tb.ConstantCoefficient(ref.KAPPA_E * 10.0), one, one)
    if bidomain:
        stage = tb.BidomainBackwardEulerStage(solver, strategy, dh, Di, De, [0], source=stim, pattern=sp)
        A, Md = stage_dense(stage, dt)
    else:
        stage = tb.BackwardEulerStage(solver, strategy, dh, Di, stim, sp)
        Md = ref.dense_of_csr(sp.rowptr, sp.colidx, stage.M.A.to_host())
        A = ref.heat_matrix(sp.rowptr, sp.colidx, stage.M.A.to_host(), stage.K.A.to_host(), dt)
    # the stimulus vector of every step, from an operator of its own (the loop's is updated as it goes)
    probe = tb.setup_operator(strategy, stim, dh)
    sources = [tb.update_operator(probe, (s + 1) * dt).b.to_host() for s in range(steps)]
    model = tb.FHNModel()
    u0 = np.zeros((2, n))
    u0[1] = 0.05
    f = tb.PointwiseODEFunction(n, model)
    cache = tb.setup_solver_cache(f, tb.ForwardEulerCellSolver(device), u=device.to_device(u0.ravel()))
    ltg = tb.LieTrotterGodunov(stage, f, cache)
    u, phie, its = u0.ravel().copy(), np.zeros(n), 0
    for s in range(steps):
        assert ltg.step(s * dt, dt)
        its += stage.last_iters
        if bidomain:
            x = ref.solve_refined(A, np.concatenate([Md @ u[:n] + sources[s], np.zeros(n)]))
            u[:n], phie = x[:n], x[n:]
        else:
            u[:n] = ref.solve_refined(A, Md @ u[:n] + sources[s])
        oracle.reaction_step(oracle.CELL_FHN, model.params, u, n, oracle.LAYOUT_SOA, t=s * dt, dt=dt)
    got = cache.un.to_host()
    dev_state = float(np.abs(got - u).max())
    dev_e = float(np.abs(stage.phi_e.to_host() - phie).max()) if bidomain else 0.0
    return {"state": dev_state, "phi_e": dev_e, "phi_range": [float(u[:n].min()), float(u[:n].max())], "phi_e_range": [float(phie.min()), float(phie.max())],
            "iterations_per_step": its / steps}


def test_time_loop_against_the_reference_loop(tb, device, oracle):
    """the bidomain loop within ten times the deviation of the monodomain loop from its own reference loop (LOOP_MONODOMAIN_DEVIATION above)"""
    mono = loop_deviation(tb, device, oracle, False)
    bi = loop_deviation(tb, device, oracle, True)
    print("20-step loop, device against reference: monodomain %r; bidomain %r; tolerance %r" % (mono, bi, LOOP_TOLERANCE))
    assert bi["phi_range"][1] > 0.5 and max(abs(v) for v in bi["phi_e_range"]) > 0.1      # the corner fired, φₑ answered
    assert mono["state"] <= LOOP_TOLERANCE                                   # the yardstick still measures what it measured
    assert bi["state"] <= LOOP_TOLERANCE and bi["phi_e"] <= LOOP_TOLERANCE


# ------------------------------------------------------------------------------------------------ 8. capture, 9. refusals
def test_apply_replays_from_a_capture_and_the_solve_refuses_inside_one(tb, cases):
    dev2 = tb.MI355XDevice(0)                                               # a device of its own: a refused call must not disturb the shared one
    g, dh, sp = ref.build_mesh(tb, "hex_5x4x3")
    n = dh.ndofs
    M, Ki, Ke = cases("hex_5x4x3")["host"]
    pattern = tb.DeviceMesh(dev2, dh).pattern(sp)
    flags = np.zeros(n, dtype=np.uint8)
    flags[0] = 1
    system = tb.BidomainSystem(pattern)
    system.set_matrices(dev2.to_device(M), dev2.to_device(Ki), dev2.to_device(Ke), ref.DT, dev2.to_device(flags), ref.ground_diagonal(sp.rowptr, sp.colidx, Ki, Ke, ref.DT))
    dx, dy = dev2.to_device(np.random.default_rng(16).uniform(-1.0, 1.0, 2 * n)), dev2.zeros(2 * n)
    system.apply(dx, dy)
    direct = dy.to_host()
    graph = dev2.capture(lambda: system.apply(dx, dy))
    dy.fill_zero()
    graph.launch(0.0)
    dev2.synchronize()
    assert np.array_equal(dy.to_host(), direct)
    with pytest.raises(tb.TBError) as e:
        dev2.capture(lambda: system.solve(dx, dy, maxiter=5))
    assert e.value.code == tb._lib.TB_ERR_BAD_ARG and "capture" in str(e.value)
    system.apply(dx, dy)                                                    # the stream is still usable
    assert np.array_equal(dy.to_host(), direct)


def test_refusals(tb, device, cases):
    case = cases("hex_5x4x3")
    n = case["dh"].ndofs
    flags = device.to_device(np.eye(1, n, 0, dtype=np.uint8).ravel())
    system = tb.BidomainSystem(case["pattern"])
    M, Ki, Ke = case["dev"]
    lib = tb.lib()
    for dt in (0.0, -0.1, float("nan"), float("inf")):
        assert lib.tb_bidomain_set_matrices(system.h, case["pattern"].h, M.ptr, Ki.ptr, Ke.ptr, dt, flags.ptr, 1.0) == tb._lib.TB_ERR_BAD_ARG, dt
    x, y = device.zeros(2 * n), device.zeros(2 * n)
    assert lib.tb_bidomain_apply(system.h, x.ptr, y.ptr) == tb._lib.TB_ERR_BAD_ARG            # no matrices yet
    other = case["dh"].device_mesh(device).pattern(tb.allocate_matrix(case["dh"]))             # the same sparsity, another pattern object
    assert other.h.value != case["pattern"].h.value
    assert lib.tb_bidomain_set_matrices(system.h, other.h, M.ptr, Ki.ptr, Ke.ptr, 0.1, flags.ptr, 1.0) == tb._lib.TB_ERR_BAD_ARG
    assert b"another pattern" in lib.tb_last_error_string()
    assert lib.tb_bidomain_set_matrices(system.h, case["pattern"].h, M.ptr, Ki.ptr, Ke.ptr, 0.1, flags.ptr, 1.0) == 0
    assert lib.tb_bidomain_apply(system.h, x.ptr, x.ptr) == tb._lib.TB_ERR_BAD_ARG            # aliasing
    assert lib.tb_bidomain_apply(system.h, C.c_void_p(x.ptr.value + 8), y.ptr) == tb._lib.TB_ERR_BAD_ARG   # alignment of the pairs
    g2 = tb.generate_mesh(tb.Hexahedron, (2, 2, 2))
    dh2 = tb.DofHandler(g2, tb.LagrangeCollection(2))
    D = tb.ConstantCoefficient(ref.KAPPA_I)
    with pytest.raises(NotImplementedError):
        tb.BidomainBackwardEulerStage(tb.BackwardEulerSolver(), tb.PerColorAssemblyStrategy(device), dh2, D, D, [0])
    with pytest.raises(ValueError, match="ground"):
        tb.BidomainBackwardEulerStage(tb.BackwardEulerSolver(), tb.PerColorAssemblyStrategy(device), case["dh"], D, D, [])
    h = C.c_void_p()
    sp2 = tb.allocate_matrix(dh2)
    assert lib.tb_bidomain_create(dh2.device_mesh(device).pattern(sp2).h, C.byref(h)) == tb._lib.TB_ERR_UNSUPPORTED and not h


def test_the_bidomain_example_runs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "bidomain_block.py"), "--nx", "12", "--steps", "4"], capture_output=True, text=True, timeout=300,
                         cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads(out.stdout.strip().splitlines()[-1])
    assert d["all_converged"] and d["phi_m_range"][1] > 0.1 and d["lead"] != 0.0 and d["cg_iterations_per_step"] > 0
