"""Times the pseudo-ECG kernels on one MI355X: tb_ecg_update and tb_ecg_evaluate (12 electrodes) on an n³ hexahedral heart (default 128³: 16.8 M
quadrature points) and tb_ecg_leads (12 leads × 2 M dofs).  Prints ONE JSON line.

Per kernel: device-event time per call after the _preroll pre-roll (the better of two loops of `--reps` calls, no profiler), the bytes the algorithm
moves and their rate as a fraction of the copy rate of the part that DESIGN.md §5 quotes (4.6 TB/s).  Bytes:
  update    per cell connectivity + dof table (2 × 8 × 4 B), vertex coordinates (8 × 24 B) and φ (8 × 8 B), plus 24 B of flux stored per point
  evaluate  56 B per point (x̃, dΩ, flux) for ONE pass; with more electrodes than the kernel's tile the points are passed over once per tile
            (`evaluate_passes` in the output) and the rate is quoted for the bytes of all passes
  leads     8 B · (n_leads + 1) · n
The electrode / row tile is the library's (16); a profiling build (make ablation, TB_LIBTBHIP) reads TB_ECG_TILE = 4 | 8 | 16 for the sweep.

    python scripts/bench_ecg.py [--n 128] [--electrodes 12] [--leads 12] [--lead-dofs 2000000] [--reps 20]"""
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

COPY_RATE_GBS = 4600.0         # copy rate of the part (profiles/r03_v2/stream_rates.txt)

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=128)
ap.add_argument("--electrodes", type=int, default=12)
ap.add_argument("--leads", type=int, default=12)
ap.add_argument("--lead-dofs", type=int, default=2000000)
ap.add_argument("--reps", type=int, default=20)
args = ap.parse_args()

dev = tb.MI355XDevice(0)
lib, check = tb.lib(), tb._lib.check
tile = int(os.environ.get("TB_ECG_TILE", "16")) if os.environ.get("TB_LIBTBHIP") else 16


def timed(fn):
    """ms per call: pre-roll, then the better of two event-timed loops"""
    preroll(dev, fn)
    best = None
    for _ in range(2):
        e0, e1 = dev.event(), dev.event()
        e0.record()
        for _ in range(args.reps):
            fn()
        e1.record()
        dev.synchronize()
        ms = e0.elapsed_ms(e1) / args.reps
        best = ms if best is None else min(best, ms)
    return best


def line(ms, nbytes):
    gbs = nbytes / (ms * 1e-3) / 1e9
    return {"ms": round(ms, 4), "bytes": int(nbytes), "GB_per_s": round(gbs, 1), "fraction_of_copy_rate": round(gbs / COPY_RATE_GBS, 3)}


n = args.n
g = tb.generate_mesh(tb.Hexahedron, (n, n, n), (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), perturb=0.2)
dh = tb.DofHandler(g)
op = tb.setup_operator(tb.PerColorAssemblyStrategy(dev), tb.BilinearDiffusionIntegrator(tb.ConstantCoefficient(np.diag([4.5e-5, 2.0e-5, 2.0e-5]))), dh)
cache = tb.Plonsey1964ECGGaussCache(op, dev.zeros(dh.ndofs))
ecg, npts = cache.h, cache.n_points
X = tb.dof_coordinates(dh)
phi = dev.to_device(np.tanh(4.0 * X[:, 0]) + 0.1 * X[:, 1])
rng = np.random.default_rng(0)
el = rng.uniform(1.5, 3.0, (args.electrodes, 3)) * rng.choice([-1.0, 1.0], (args.electrodes, 3))
x, out = dev.to_device(el.ravel()), dev.zeros(args.electrodes)

t_update = timed(lambda: check(lib.tb_ecg_update(ecg, phi.ptr)))
t_eval = timed(lambda: check(lib.tb_ecg_evaluate(ecg, args.electrodes, x.ptr, 1.0, out.ptr)))
passes = -(-args.electrodes // tile)
res = {"device": dev.info()["name"], "n_cu": dev.info()["n_cu"], "heart": "%d^3 hexahedra" % n, "cells": g.n_cells, "points": npts, "electrodes": args.electrodes,
       "tile": tile, "evaluate_passes": passes,
       "update": line(t_update, g.n_cells * (2 * 8 * 4 + 8 * 24 + 8 * 8) + 24 * npts),
       "evaluate": line(t_eval, 56 * npts * passes),
       "evaluate_one_pass_bytes": 56 * npts,
       "ecg_at_electrode_0": float(out.to_host()[0])}
del phi, cache, op

nd, nl = args.lead_dofs, args.leads
Z = dev.to_device(rng.uniform(-1.0, 1.0, nl * nd))
v = dev.to_device(rng.uniform(-1.0, 1.0, nd))
lo = dev.zeros(nl)
t_leads = timed(lambda: check(lib.tb_ecg_leads(dev.h, nl, nd, Z.ptr, nd, v.ptr, -1.0, lo.ptr)))
res["leads"] = dict(line(t_leads, 8 * (nl + 1) * nd * 1.0), shape="%d x %d" % (nl, nd), passes=-(-nl // tile))
print(json.dumps(res))
