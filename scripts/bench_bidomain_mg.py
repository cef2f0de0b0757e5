"""Times the multigrid preconditioner of the bidomain block system against the block-Jacobi solve on one MI355X: the box, the conductivities, the solver
tolerances and the Gaussian-bump step of scripts/bench_bidomain.py, on the finest grid of a GridHierarchy (default: 4³ cells refined five times, 128³).
Prints ONE JSON line.

  (a) step      BidomainBackwardEulerStage.perform_step with block-Jacobi PCG (the yardstick) and with precond=GMGPrecon(gh) at (degree, interval_ratio) =
                (2, 4), (2, 10), (3, 4): time and CG iterations, at Δt = --dt and at --dt2
  (b) cycle     one application of the V-cycle, and the part below the finest level (BidomainMultigrid.cycle_below): the finest level's share is the
                difference
  (c) set-up    tb_bidomain_set_matrices + tb_bidomain_mg_setup, what a Δt change costs on top of the step
  (d) smoother  the fused smoother step against product + vector kernel, as the time of a whole cycle: only when TB_LIBTBHIP names the profiling build
                (make ablation), whose TB_BDMG_SMOOTHER=split selects the composition

Protocol: every timed loop runs behind the _preroll pre-roll and is timed with device events; the variants of (a) ALTERNATE in `--rounds` rounds in one
process on one box, every round is reported, and each timed step starts from the same state.

    python scripts/bench_bidomain_mg.py [--coarse 4] [--refinements 5] [--rounds 3] [--step-reps 2] [--dt 0.01] [--dt2 0.1]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import numpy as np  # noqa: E402

import thunderbolt_jl_amd as tb  # noqa: E402
from _preroll import preroll  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--coarse", type=int, default=4)
ap.add_argument("--refinements", type=int, default=5)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--step-reps", type=int, default=2)
ap.add_argument("--cycle-reps", type=int, default=20)
ap.add_argument("--dt", type=float, default=0.01)
ap.add_argument("--dt2", type=float, default=0.1)
ap.add_argument("--maxiter", type=int, default=50000)
args = ap.parse_args()
SETTINGS = ((2, 4.0), (2, 10.0), (3, 4.0))

dev = tb.MI355XDevice(0)
lib, check = tb.lib(), tb._lib.check


def say(msg):
    print("[bench_bidomain_mg] " + msg, file=sys.stderr, flush=True)


def loop_ms(fn, reps):
    e0, e1 = dev.event(), dev.event()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    dev.synchronize()
    return e0.elapsed_ms(e1) / reps


kap_i = tb.ConstantCoefficient(np.diag([4.5e-2, 2.0e-2, 2.0e-2]))
kap_e = tb.ConstantCoefficient(np.diag([3.0e-2, 2.25e-2, 2.25e-2]))
one = tb.ConstantCoefficient(1.0)
Di, De = tb.ConductivityToDiffusivityCoefficient(kap_i, one, one), tb.ConductivityToDiffusivityCoefficient(kap_e, one, one)
t0 = time.time()
gh = tb.GridHierarchy(tb.generate_mesh(tb.Hexahedron, (args.coarse,) * 3, (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)), args.refinements)
dh = tb.DofHandler(gh.finest)
sp = tb.allocate_matrix(dh)
nd = dh.ndofs
n = args.coarse * 2 ** args.refinements
res = {"device": dev.info()["name"], "box": "%d^3 hexahedra (%d^3 cells refined %d times)" % (n, args.coarse, args.refinements), "dofs": nd, "unknowns": 2 * nd,
       "nnz_scalar": int(sp.nnz), "rounds": args.rounds, "step_reps": args.step_reps}
say("grids and pattern: %.1f s; assembling and planning" % (time.time() - t0))
t0 = time.time()
stage = tb.BidomainBackwardEulerStage(tb.BackwardEulerSolver(maxiter=args.maxiter), tb.PatchAssemblyStrategy(dev), dh, Di, De, [0], pattern=sp, precond=tb.GMGPrecon(gh))
mg = stage.multigrid
res["host_seconds_assembly_and_plans"] = round(time.time() - t0, 1)
res["levels"] = mg.n_levels
say("stage with %d levels: %.1f s" % (mg.n_levels, time.time() - t0))
X = tb.dof_coordinates(dh)
phi_h = np.exp(-8.0 * ((X[:, 0] + 0.1) ** 2 + X[:, 1] ** 2 + X[:, 2] ** 2))
phi, keep = dev.to_device(phi_h), dev.to_device(phi_h)


def set_operator(dt, setting):
    """what perform_step does on a Δt change, under our control: the matrices of `dt`, the hierarchy at `setting` (None: none)"""
    stage.system.set_matrices(stage.M.A, stage.Ki.A, stage.Ke.A, dt, stage.ground_flags, stage.ground_diag(dt))
    stage.dt_last = dt
    if setting is not None:
        mg.degree, mg.interval_ratio = setting
        mg.setup()


def make_step(dt, use_mg):
    def step():
        check(lib.tb_memcpy_d2d(dev.h, phi.ptr, keep.ptr, phi.nbytes))
        stage.phi_e.fill_zero()
        stage.multigrid = mg if use_mg else None
        if not stage.perform_step(phi, 0.0, dt):
            raise SystemExit("the step did not converge in %d iterations" % args.maxiter)
    return step


def time_steps(dt):
    names = ["block_jacobi"] + ["mg_degree%d_ratio%g" % s for s in SETTINGS]
    out = {k: {"rounds_ms": [], "cg_iterations": None} for k in names}
    for r in range(args.rounds):
        for name, setting in zip(names, (None,) + SETTINGS):
            set_operator(dt, setting)
            step = make_step(dt, setting is not None)
            step()
            dev.synchronize()
            out[name]["cg_iterations"], out[name]["resnorm"] = stage.last_iters, stage.last_resnorm
            preroll(dev, step, ms=0.0)
            out[name]["rounds_ms"].append(round(loop_ms(step, args.step_reps), 3))
        say("dt %g round %d: %s" % (dt, r, {k: (v["rounds_ms"][-1], v["cg_iterations"]) for k, v in out.items()}))
    for v in out.values():
        v["min_ms"], v["max_ms"] = min(v["rounds_ms"]), max(v["rounds_ms"])
        v["ms_per_iteration"] = round(v["min_ms"] / max(v["cg_iterations"], 1), 4)
    best = min((k for k in names[1:]), key=lambda k: out[k]["min_ms"])
    out["best_multigrid"] = best
    out["block_jacobi_over_best_multigrid"] = round(out["block_jacobi"]["min_ms"] / out[best]["min_ms"], 3)
    return out


res["step_dt_%g" % args.dt] = time_steps(args.dt)
res["step_dt_%g" % args.dt2] = time_steps(args.dt2)

# ---- (b) one cycle, split; (c) the set-up
set_operator(args.dt, SETTINGS[0])
res["lambda_max"] = [mg.lambda_max(l) for l in range(1, mg.n_levels)]
r, z = dev.to_device(np.random.default_rng(1).uniform(-1, 1, 2 * nd)), dev.zeros(2 * nd)
cyc, tail, setup_ms = [], [], []
for _ in range(args.rounds):
    preroll(dev, lambda: mg.apply(r, z))
    cyc.append(round(loop_ms(lambda: mg.apply(r, z), args.cycle_reps), 4))
    preroll(dev, lambda: mg.cycle_below(mg.n_levels - 2))
    tail.append(round(loop_ms(lambda: mg.cycle_below(mg.n_levels - 2), args.cycle_reps), 4))
    t0 = time.time()
    set_operator(args.dt, SETTINGS[0])
    dev.synchronize()
    setup_ms.append(round(1e3 * (time.time() - t0), 2))
res["cycle_ms"] = {"whole": cyc, "below_the_finest_level": tail, "finest_level_min": round(min(cyc) - min(tail), 4), "levels_below": mg.n_levels - 1}
res["setup_ms_wall"] = setup_ms

# ---- (d) fused smoother step against product + vector kernel (profiling build only)
if os.environ.get("TB_LIBTBHIP"):
    os.environ["TB_BDMG_SMOOTHER"] = "split"
    mg_split = tb.BidomainMultigrid(stage.system, gh, *SETTINGS[0]).setup()
    del os.environ["TB_BDMG_SMOOTHER"]
    z2 = dev.zeros(2 * nd)
    mg.apply(r, z)
    mg_split.apply(r, z2)
    a, b = z.to_host(), z2.to_host()
    fused, split = [], []
    for _ in range(args.rounds):
        preroll(dev, lambda: mg.apply(r, z))
        fused.append(round(loop_ms(lambda: mg.apply(r, z), args.cycle_reps), 4))
        preroll(dev, lambda: mg_split.apply(r, z2))
        split.append(round(loop_ms(lambda: mg_split.apply(r, z2), args.cycle_reps), 4))
    res["smoother_cycle_ms"] = {"fused": fused, "product_plus_vector_kernel": split, "agreement_max_abs_over_scale": float(np.abs(a - b).max() / np.abs(a).max())}
print(json.dumps(res))
