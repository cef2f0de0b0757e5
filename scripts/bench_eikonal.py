"""Times the eikonal solver (tb_eikonal_solve: the fast iterative method of csrc/tb_eikonal.hip) on one MI355X.  Prints ONE JSON line.

Cases: an n³ hexahedral box (default 128³, 2.1 M nodes, 50 M corner records) with G = diag(4, 1, 1) from one corner source and from a mid-face
source, and the idealised ventricle with its rule-based fibre field (G = 4 : 1 : 0.5 along fibre, sheet, normal) from three endocardial sources.
Per case: sweeps, wall time of a whole solve (host clock around the call and a device synchronise; the better of `--reps` solves after one untimed
solve), nodes evaluated / updates accepted / local solves of the solve (tb_eikonal_last_counts) and their rates, and the time between two
convergence checks (solve time over the number of batches of 16 sweeps).

A/B of the data layout (`--ab`, needs the profiling build: make -C thunderbolt.jl_amd/csrc ablation, TB_LIBTBHIP=…/libtbhip_ablation.so): two solver
objects on the same form in one process — edge vectors from the coordinates (what ships) and the per-tetrahedron table of six edge products
(TB_EIKONAL_LAYOUT=table) — solved alternately on the box's corner case; both times and the largest difference of the two fields are reported.

For context only, `monodomain_steps_equivalent` is the number of steps of the existing monodomain loop the solve time equals, ESTIMATED from the
project's recorded 4.8 ms per step at 216³ (10 077 696 dofs) scaled by the dof count — not a measured comparison.

    python scripts/bench_eikonal.py [--n 128] [--lv 256 24 128] [--reps 2] [--ab]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import thunderbolt_jl_amd as tb  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=128)
ap.add_argument("--lv", type=int, nargs=3, default=[256, 24, 128], help="ideal ventricle: cells around, across the wall, apex to base")
ap.add_argument("--reps", type=int, default=2)
ap.add_argument("--rtol", type=float, default=1e-12)
ap.add_argument("--ab", action="store_true")
args = ap.parse_args()
CHECK_EVERY = 16                      # csrc/tb_eikonal.hip: EIK_CHECK_EVERY
MONODOMAIN_MS_PER_STEP, MONODOMAIN_DOFS = 4.8, 216 ** 3 + 3 * 216 ** 2 + 3 * 216 + 1

dev = tb.MI355XDevice(0)


def timed_solve(cache, sources, times, out):
    tb.solve_activation(cache, sources, times=times, rtol=args.rtol, out=out)       # untimed: first launches, clocks
    dev.synchronize()
    best = None
    for _ in range(args.reps):
        t0 = time.perf_counter()
        tb.solve_activation(cache, sources, times=times, rtol=args.rtol, out=out)
        dev.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        best = ms if best is None else min(best, ms)
    return best


def report(cache, ms, ndofs):
    batches = -(-cache.sweeps // CHECK_EVERY)
    return {"nodes": int(ndofs), "sweeps": cache.sweeps, "converged": cache.converged, "ms": round(ms, 3),
            "nodes_evaluated": cache.evaluations, "updates_accepted": cache.updates, "local_solves": cache.local_solves,
            "node_evaluations_per_s": round(cache.evaluations / (ms * 1e-3), 1), "node_updates_per_s": round(cache.updates / (ms * 1e-3), 1),
            "local_solves_per_s": round(cache.local_solves / (ms * 1e-3), 1), "ms_between_convergence_checks": round(ms / batches, 3),
            "monodomain_steps_equivalent_estimate": round(ms / (MONODOMAIN_MS_PER_STEP * ndofs / MONODOMAIN_DOFS), 2)}


res = {"device": dev.info()["name"], "n_cu": dev.info()["n_cu"], "rtol": args.rtol, "check_every": CHECK_EVERY,
       "library": os.path.basename(tb._lib.LIB_PATH)}
n = args.n
g = tb.generate_mesh(tb.Hexahedron, (n, n, n), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
dh = tb.DofHandler(g)
model = tb.EikonalModel(tb.ConstantCoefficient(np.diag([4.0, 1.0, 1.0])))
t0 = time.perf_counter()
cache = tb.EikonalActivationCache(dev, model, dh)
res["box"] = {"cells": "%d^3 hexahedra" % n, "plan_and_upload_s": round(time.perf_counter() - t0, 2)}
T = tb.DeviceVector(dev, dh.ndofs)
corner = [0]
midface = [tb.get_closest_vertex([0.0, 0.5, 0.5], g)]
res["box"]["corner_source"] = report(cache, timed_solve(cache, corner, None, T), dh.ndofs)
res["box"]["midface_source"] = report(cache, timed_solve(cache, midface, None, T), dh.ndofs)

if args.ab:
    os.environ["TB_EIKONAL_LAYOUT"] = "table"
    table = tb.EikonalActivationCache(dev, model, dh)
    del os.environ["TB_EIKONAL_LAYOUT"]
    T2 = tb.DeviceVector(dev, dh.ndofs)
    ms = {"coordinates": [], "table": []}
    for _ in range(3):                                              # alternating, same process, same device
        ms["coordinates"].append(round(timed_solve(cache, corner, None, T), 3))
        ms["table"].append(round(timed_solve(table, corner, None, T2), 3))
    a, b = T.to_host(), T2.to_host()
    res["layout_ab_corner_source"] = {"ms": ms, "sweeps": [cache.sweeps, table.sweeps], "max_difference_of_T": float(np.abs(a - b).max()),
                                      "max_T": float(a.max())}
    del table, T2
del cache, T, dh, g

nc, nr, nl = args.lv
lv = tb.generate_ideal_lv_mesh_hex(nc, nr, nl)
ldh = tb.DofHandler(lv)
f, s, nrm = tb.ideal_lv_microstructure(lv)
G = tb.SpectralTensorCoefficient(tb.OrthotropicMicrostructureModel(f, s, nrm), tb.ConstantCoefficient(np.array([4.0, 1.0, 0.5])))
lcache = tb.EikonalActivationCache(dev, tb.EikonalModel(G), ldh)
endo = np.flatnonzero(lv.parametric[:, 2] == 0.0)
src = endo[np.linspace(0, len(endo) - 1, 5).astype(int)[1:4]]
LT = tb.DeviceVector(dev, ldh.ndofs)
res["ideal_ventricle"] = dict(report(lcache, timed_solve(lcache, src, [0.0, 0.1, 0.2], LT), ldh.ndofs), cells=int(lv.n_cells),
                              mesh="%d x %d x %d" % (nc, nr, nl))
print(json.dumps(res))
