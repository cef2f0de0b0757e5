"""Times the parabolic–elliptic bidomain block system on one MI355X, on the n³ box of scripts/bench_multidomain.py (default 128³).  Prints ONE JSON line.

  (a) product   tb_bidomain_apply (one fused pass, node-interleaved unknown) against the composition of existing entries that computes the same y on
                the same matrices: four tb_spmv_csr calls with α and β over the value arrays M − ΔtKᵢ, −ΔtKᵢ, −Δt(Kᵢ + Kₑ) — once as they are
                (signature-row kernel) and once with the two sliced mirrors a pattern can bind (tb_spmv_mirror on −ΔtKᵢ and −Δt(Kᵢ + Kₑ))
  (b) step      BidomainBackwardEulerStage.perform_step against BackwardEulerStage.perform_step (D = Dᵢ) from the same φₘ: time, CG iterations, time
                per iteration

Protocol: every timed loop runs behind the _preroll pre-roll and is timed with device events; the variants of (a) ALTERNATE (`--rounds` rounds of
fused, composition, mirrored composition, `--reps` calls each) in one process on one box, and every round is reported beside the minimum, so the
run-to-run spread can be read off.  Each timed step of (b) starts from the same state.

    python scripts/bench_bidomain.py [--n 128] [--reps 20] [--rounds 5] [--step-reps 2] [--dt 0.01]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import numpy as np  # noqa: E402

import thunderbolt_jl_amd as tb  # noqa: E402
from _preroll import preroll  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=128)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--step-reps", type=int, default=2)
ap.add_argument("--dt", type=float, default=0.01)
ap.add_argument("--maxiter", type=int, default=50000)
args = ap.parse_args()

dev = tb.MI355XDevice(0)
lib, check = tb.lib(), tb._lib.check
n, dt = args.n, args.dt


def say(msg):
    print("[bench_bidomain] " + msg, file=sys.stderr, flush=True)


def loop_ms(fn, reps):
    e0, e1 = dev.event(), dev.event()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    dev.synchronize()
    return e0.elapsed_ms(e1) / reps


# the box and the intracellular conductivity of bench_multidomain.py; κₑ with another anisotropy ratio (3 : 2.25 against 4.5 : 2)
kap_i = tb.ConstantCoefficient(np.diag([4.5e-2, 2.0e-2, 2.0e-2]))
kap_e = tb.ConstantCoefficient(np.diag([3.0e-2, 2.25e-2, 2.25e-2]))
one = tb.ConstantCoefficient(1.0)
Di, De = tb.ConductivityToDiffusivityCoefficient(kap_i, one, one), tb.ConductivityToDiffusivityCoefficient(kap_e, one, one)
strategy = tb.PatchAssemblyStrategy(dev)
g = tb.generate_mesh(tb.Hexahedron, (n, n, n), (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
dh = tb.DofHandler(g)
sp = tb.allocate_matrix(dh)
nd, nnz = dh.ndofs, sp.nnz
res = {"device": dev.info()["name"], "box": "%d^3 hexahedra" % n, "dofs": nd, "unknowns": 2 * nd, "nnz_scalar": int(nnz), "dt": dt, "reps": args.reps, "rounds": args.rounds}
say("assembling")
stage = tb.BidomainBackwardEulerStage(tb.BackwardEulerSolver(maxiter=args.maxiter), strategy, dh, Di, De, [0], pattern=sp)
pat = stage.M.pattern
stage.system.set_matrices(stage.M.A, stage.Ki.A, stage.Ke.A, dt, stage.ground_flags, stage.ground_diag(dt))

# ---- (a) the product
A11, A12, A22 = dev.zeros(nnz), dev.zeros(nnz), dev.zeros(nnz)
check(lib.tb_heat_matrix(dev.h, nnz, stage.M.A.ptr, stage.Ki.A.ptr, dt, A11.ptr))
check(lib.tb_axpy(dev.h, nnz, -dt, stage.Ki.A.ptr, A12.ptr))
check(lib.tb_axpy(dev.h, nnz, -dt, stage.Ki.A.ptr, A22.ptr))
check(lib.tb_axpy(dev.h, nnz, -dt, stage.Ke.A.ptr, A22.ptr))
rng = np.random.default_rng(1)
xm_h, xe_h = rng.uniform(-1, 1, nd), rng.uniform(-1, 1, nd)
xe_h[stage.ground_dofs] = 0.0                                       # the composition knows no ground: keep the grounded column out of the comparison
xm, xe, ym, ye = dev.to_device(xm_h), dev.to_device(xe_h), dev.zeros(nd), dev.zeros(nd)
x, y = dev.zeros(2 * nd), dev.zeros(2 * nd)
stage.system.pack(xm, xe, x)


def fused():
    stage.system.apply(x, y)


def composition():
    check(lib.tb_spmv_csr(pat.h, A11.ptr, xm.ptr, 1.0, 0.0, ym.ptr))
    check(lib.tb_spmv_csr(pat.h, A12.ptr, xe.ptr, 1.0, 1.0, ym.ptr))
    check(lib.tb_spmv_csr(pat.h, A12.ptr, xm.ptr, 1.0, 0.0, ye.ptr))
    check(lib.tb_spmv_csr(pat.h, A22.ptr, xe.ptr, 1.0, 1.0, ye.ptr))


fused(); composition()
yf = y.to_host()
free = np.setdiff1d(np.arange(nd), stage.ground_dofs)
scale = max(np.abs(yf).max(), 1e-300)
res["product_agreement_max_abs_over_scale"] = float(max(np.abs(yf[0::2] - ym.to_host()).max(), np.abs(yf[1::2][free] - ye.to_host()[free]).max()) / scale)
say("timing the product")
rounds = {"fused": [], "composition": [], "composition_mirrored": []}
for r in range(args.rounds):
    pat.mirror(None)
    preroll(dev, fused)
    rounds["fused"].append(loop_ms(fused, args.reps))
    preroll(dev, composition)
    rounds["composition"].append(loop_ms(composition, args.reps))
    mirrored = pat.mirror(A12) and pat.mirror(A22)
    if mirrored:
        preroll(dev, composition)
        rounds["composition_mirrored"].append(loop_ms(composition, args.reps))
pat.mirror(None)
res["product_ms"] = {k: {"rounds": [round(v, 4) for v in vs], "min": round(min(vs), 4), "max": round(max(vs), 4)} for k, vs in rounds.items() if vs}
best_comp = min(v["min"] for k, v in res["product_ms"].items() if k != "fused")
res["fused_over_best_composition"] = round(res["product_ms"]["fused"]["min"] / best_comp, 4)
del A11, A12, A22, xm, xe, ym, ye, x, y

# ---- (b) the step
say("timing the steps")
X = tb.dof_coordinates(dh)
phi_h = np.exp(-8.0 * ((X[:, 0] + 0.1) ** 2 + X[:, 1] ** 2 + X[:, 2] ** 2))
phi, keep = dev.to_device(phi_h), dev.to_device(phi_h)


def restore_bi():
    check(lib.tb_memcpy_d2d(dev.h, phi.ptr, keep.ptr, phi.nbytes))
    stage.phi_e.fill_zero()


def step_bi():
    restore_bi()
    if not stage.perform_step(phi, 0.0, dt):
        raise SystemExit("the bidomain step did not converge in %d iterations" % args.maxiter)


step_bi()
dev.synchronize()
say("bidomain step: %d iterations" % stage.last_iters)
preroll(dev, step_bi, ms=0.0)
t_bi = min(loop_ms(step_bi, args.step_reps) for _ in range(2))
res["bidomain_step"] = {"ms": round(t_bi, 3), "cg_iterations": stage.last_iters, "ms_per_iteration": round(t_bi / max(stage.last_iters, 1), 4), "resnorm": stage.last_resnorm}
mono = tb.BackwardEulerStage(tb.BackwardEulerSolver(maxiter=args.maxiter), strategy, dh, Di, None, sp)


def step_mono():
    check(lib.tb_memcpy_d2d(dev.h, phi.ptr, keep.ptr, phi.nbytes))
    if not mono.perform_step(phi, 0.0, dt):
        raise SystemExit("the monodomain step did not converge")


preroll(dev, step_mono)
t_mono = min(loop_ms(step_mono, 10) for _ in range(2))
res["monodomain_step"] = {"ms": round(t_mono, 3), "cg_iterations": mono.last_iters, "ms_per_iteration": round(t_mono / max(mono.last_iters, 1), 4)}
res["step_ratio"] = round(t_bi / t_mono, 2)
print(json.dumps(res))
