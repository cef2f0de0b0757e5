"""Times the algebraic multigrid preconditioner of the bidomain block system (BidomainAMGPrecon) against the block-Jacobi solve on one MI355X, on the
meshes the geometric block multigrid cannot take and on one it can.  Prints ONE JSON line per problem.

  --problem tet        a box of n³ lattice cells cut into 6 n³ linear tetrahedra
  --problem ventricle  the generated ideal left ventricle (n cells around, n / 4 through the wall, n along), hexahedra without nested grids
  --problem hex        the box of scripts/bench_bidomain_mg.py (--coarse cells refined --refinements times; default 128³): also against GMGPrecon(gh)

  (a) step      BidomainBackwardEulerStage.perform_step from a Gaussian bump with block-Jacobi PCG (the yardstick: tb_bidomain_solve), with
                precond=BidomainAMGPrecon(...) and, on `hex`, with precond=GMGPrecon(gh): time and CG iterations.  The variants ALTERNATE in --rounds rounds in
                one process, every round is reported, each timed step starts from the same state.
  (b) set-up    the first set-up (strength, host aggregation, uploads, numeric phase) and the numeric set-up alone (what a new Δt repeats), wall time
  (c) cycle     one application of the V-cycle
  (d) products  the fused three-plane Galerkin products of every level against three launch pairs of the scalar product kernel (k_amg_spgemm, the kernel
                the scalar hierarchy runs unchanged) on the same plans: BidomainAlgebraicMultigrid.products(level, fused), alternating

Every timed loop runs behind the _preroll pre-roll and is timed with device events.

    python scripts/bench_bidomain_amg.py --problem tet [--n 48] [--rounds 3] [--dt 0.05] [--max-coarse 128]"""
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
ap.add_argument("--problem", default="tet", choices=["tet", "ventricle", "hex"])
ap.add_argument("--n", type=int, default=48)
ap.add_argument("--coarse", type=int, default=4)
ap.add_argument("--refinements", type=int, default=5)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--step-reps", type=int, default=2)
ap.add_argument("--cycle-reps", type=int, default=20)
ap.add_argument("--dt", type=float, default=0.05)
ap.add_argument("--max-coarse", type=int, default=128)
ap.add_argument("--maxiter", type=int, default=50000)
args = ap.parse_args()

dev = tb.MI355XDevice(0)
lib, check = tb.lib(), tb._lib.check


def say(msg):
    print("[bench_bidomain_amg] " + msg, file=sys.stderr, flush=True)


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
gh = None
if args.problem == "tet":
    g = tb.generate_mesh(tb.Tetrahedron, (args.n,) * 3, (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
    box = "%d^3 lattice cells, %d linear tetrahedra" % (args.n, g.n_cells)
elif args.problem == "ventricle":
    g = tb.generate_ideal_lv_mesh_hex(args.n, max(args.n // 4, 1), args.n)
    box = "ideal left ventricle, %d x %d x %d hexahedra" % (args.n, max(args.n // 4, 1), args.n)
else:
    gh = tb.GridHierarchy(tb.generate_mesh(tb.Hexahedron, (args.coarse,) * 3, (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)), args.refinements)
    g = gh.finest
    box = "%d^3 hexahedra (%d^3 cells refined %d times)" % (args.coarse * 2 ** args.refinements, args.coarse, args.refinements)
dh = tb.DofHandler(g)
sp = tb.allocate_matrix(dh)
nd = dh.ndofs
res = {"device": dev.info()["name"], "problem": args.problem, "box": box, "dofs": nd, "unknowns": 2 * nd, "nnz_scalar": int(sp.nnz), "dt": args.dt, "rounds": args.rounds,
       "step_reps": args.step_reps, "max_coarse": args.max_coarse}
say("%s: grid and pattern %.1f s; assembling" % (box, time.time() - t0))
strategy = tb.PatchAssemblyStrategy(dev) if args.problem == "hex" else tb.PerColorAssemblyStrategy(dev)
stage = tb.BidomainBackwardEulerStage(tb.BackwardEulerSolver(maxiter=args.maxiter), strategy, dh, Di, De, [0], pattern=sp)
system = stage.system
X = tb.dof_coordinates(dh)
c = X.mean(axis=0)
phi_h = np.exp(-8.0 * ((X - c) ** 2).sum(axis=1) / (X.max() - X.min()) ** 2 * 4.0)
phi, keep = dev.to_device(phi_h), dev.to_device(phi_h)


def set_matrices():
    system.set_matrices(stage.M.A, stage.Ki.A, stage.Ke.A, args.dt, stage.ground_flags, stage.ground_diag(args.dt))
    stage.dt_last = args.dt


# ---- (b) the set-ups
set_matrices()
amg = tb.BidomainAMGPrecon(max_coarse=args.max_coarse).materialize(system)
dev.synchronize()
t0 = time.time()
amg.setup()
dev.synchronize()
res["first_setup_ms_wall"] = round(1e3 * (time.time() - t0), 1)
numeric = []
for _ in range(args.rounds):
    t0 = time.time()
    amg.setup()
    dev.synchronize()
    numeric.append(round(1e3 * (time.time() - t0), 2))
res["numeric_setup_ms_wall"] = numeric
res["levels"] = [amg.level_size(l) for l in range(amg.n_levels)]
res["lambda_max"] = [amg.lambda_max(l) for l in range(amg.n_levels - 1)]
say("levels %s; first set-up %.0f ms, numeric %s ms" % (res["levels"], res["first_setup_ms_wall"], numeric))
variants = {"block_jacobi": None, "amg": amg}
if gh is not None:
    t0 = time.time()
    variants["gmg"] = tb.BidomainMultigrid(system, gh).setup()
    res["gmg_levels"] = variants["gmg"].n_levels
    say("geometric hierarchy: %.1f s" % (time.time() - t0))


# ---- (a) the step
def make_step(precond):
    def step():
        check(lib.tb_memcpy_d2d(dev.h, phi.ptr, keep.ptr, phi.nbytes))
        stage.phi_e.fill_zero()
        stage.multigrid = precond
        if not stage.perform_step(phi, 0.0, args.dt):
            raise SystemExit("the step did not converge in %d iterations" % args.maxiter)
    return step


out = {k: {"rounds_ms": [], "cg_iterations": None} for k in variants}
for r in range(args.rounds):
    for name, precond in variants.items():
        step = make_step(precond)
        step()
        dev.synchronize()
        out[name]["cg_iterations"], out[name]["resnorm"] = stage.last_iters, stage.last_resnorm
        preroll(dev, step, ms=0.0)
        out[name]["rounds_ms"].append(round(loop_ms(step, args.step_reps), 3))
    say("round %d: %s" % (r, {k: (v["rounds_ms"][-1], v["cg_iterations"]) for k, v in out.items()}))
for v in out.values():
    v["min_ms"], v["max_ms"] = min(v["rounds_ms"]), max(v["rounds_ms"])
    v["ms_per_iteration"] = round(v["min_ms"] / max(v["cg_iterations"], 1), 4)
out["block_jacobi_over_amg"] = round(out["block_jacobi"]["min_ms"] / out["amg"]["min_ms"], 3)
res["step"] = out

# ---- (c) one cycle; (d) the fused products against three launch pairs of the scalar kernel
rv, z = dev.to_device(np.random.default_rng(1).uniform(-1, 1, 2 * nd)), dev.zeros(2 * nd)
cyc = []
for _ in range(args.rounds):
    preroll(dev, lambda: amg.apply(rv, z))
    cyc.append(round(loop_ms(lambda: amg.apply(rv, z), args.cycle_reps), 4))
res["cycle_ms"] = cyc
prod = []
for l in range(amg.n_levels - 1):
    before = amg.level_blocks(l + 1)
    fused, three = [], []
    for _ in range(args.rounds):
        for fl, acc in ((True, fused), (False, three)):
            preroll(dev, lambda: amg.products(l, fl), ms=50.0)
            acc.append(round(loop_ms(lambda: amg.products(l, fl), args.cycle_reps), 4))
    same = all(np.array_equal(a, b) for a, b in zip(before, amg.level_blocks(l + 1)))
    prod.append({"level": l, "nodes": amg.level_size(l)[0], "fused_ms": fused, "three_scalar_pairs_ms": three, "three_over_fused": round(min(three) / min(fused), 3),
                 "planes_keep_their_bits": bool(same)})
res["products"] = prod
print(json.dumps(res))
