#!/usr/bin/env python3
"""Times the smoothed-aggregation multigrid (AMGPrecon, tb_amg_*) against the other preconditioners on the same system, in one process:
  --problem box        −K (or M − Δt·K with --dt) of the Q1 diffusion operator (tensor diag(9, 4, 4)) on an n³ hexahedral box, Dirichlet on x = 0; with
                       --coarse the geometric multigrid of a coarse³ box refined to n runs beside it
  --problem tet        the same operator on an n³ box cut into linear tetrahedra (no geometric multigrid exists for it)
  --problem ventricle  the Laplacian on the generated ideal left ventricle (n cells around, n / 4 through the wall, n along), Dirichlet on the base
Reported: host seconds of the first setup (strength, aggregation and pattern planning on the host, uploads, numeric phase), milliseconds of the
numeric-only setup a Newton iteration or a new Δt repeats, milliseconds per cycle, the levels, and for every preconditioner the iterations and
milliseconds of the solve to --rtol.  The candidates alternate inside each repetition, medians over --reps.  HIP events around enqueued work, a device
synchronise at the end, a pre-roll.  Prints one JSON line and, with --out, writes it to a file."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _preroll import preroll  # noqa: E402  (scripts/ is on sys.path: this file lives there)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problem", default="box", choices=["box", "tet", "ventricle"])
    ap.add_argument("--n", type=int, default=64, help="cells per side (ventricle: cells around, a multiple of 4)")
    ap.add_argument("--coarse", type=int, default=0, help="box: cells per side of the coarsest grid of the geometric multigrid run beside the AMG (0: none)")
    ap.add_argument("--dt", type=float, default=0.0, help="A = M − Δt·K; 0: A = −K")
    ap.add_argument("--rtol", type=float, default=1e-8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--theta", type=float, default=0.25)
    ap.add_argument("--degree", type=int, default=2)
    ap.add_argument("--ratio", type=float, default=4.0)
    ap.add_argument("--max-coarse", type=int, default=1024)
    ap.add_argument("--jacobi-maxiter", type=int, default=20000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import thunderbolt_jl_amd as tb
    dev = tb.MI355XDevice(0)
    n, gh = args.n, None
    if args.problem == "box" and args.coarse:
        refinements = int(round(np.log2(n / args.coarse)))
        assert args.coarse * 2 ** refinements == n and refinements >= 1, "n / coarse must be a power of two"
        gh = tb.GridHierarchy(tb.generate_mesh(tb.Hexahedron, (args.coarse,) * 3, (0, 0, 0), (1, 1, 1)), refinements)
        g = gh.grids[-1]
    elif args.problem == "ventricle":
        g = tb.generate_ideal_lv_mesh_hex(n, max(n // 4, 1), n)
    else:
        g = tb.generate_mesh(tb.Tetrahedron if args.problem == "tet" else tb.Hexahedron, (n, n, n), (0, 0, 0), (1, 1, 1))
    dh = tb.DofHandler(g)
    sp = tb.allocate_matrix(dh)
    X = tb.dof_coordinates(dh)
    fixed = np.flatnonzero(X[:, 2] >= X[:, 2].max() - 1e-9) if args.problem == "ventricle" else np.flatnonzero(X[:, 0] == 0.0)
    ch = tb.ConstraintHandler(dh, fixed)
    st = tb.PatchAssemblyStrategy(dev) if args.problem != "ventricle" else tb.PerColorAssemblyStrategy(dev)
    tensor = np.eye(3) if args.problem == "ventricle" else np.diag([9.0, 4.0, 4.0])
    D = tb.ConductivityToDiffusivityCoefficient(tb.ConstantCoefficient(tensor), tb.ConstantCoefficient(1.0), tb.ConstantCoefficient(1.0))
    K = tb.update_operator(tb.setup_operator(st, tb.BilinearDiffusionIntegrator(D), dh, sp), 0.0)
    pattern = K.pattern
    vals = -K.A.to_host()
    if args.dt > 0:
        M = tb.update_operator(tb.setup_operator(st, tb.BilinearMassIntegrator(tb.ConstantCoefficient(1.0)), dh, sp), 0.0)
        vals = M.A.to_host() + args.dt * vals
    A = dev.to_device(vals)
    tb.apply_zero(A, None, ch, pattern=pattern)
    b = np.random.default_rng(0).uniform(0.0, 1.0, dh.ndofs)
    b[ch.prescribed_dofs] = 0.0
    db = dev.to_device(b)
    dev.synchronize()
    t0 = time.perf_counter()
    amg = tb.AMGPrecon(args.theta, args.degree, args.ratio, args.max_coarse).materialize(pattern, ch)
    amg.setup(A)
    dev.synchronize()
    first_setup_s = time.perf_counter() - t0
    candidates = {"amg": amg, "jacobi": "jacobi", "chebyshev16": tb.ChebyshevPrecBuilder(16)}
    gmg_first_s = None
    if gh is not None:
        t0 = time.perf_counter()
        gmg = tb.MultigridHierarchy(pattern, gh, args.degree, args.ratio, ch)
        gmg.setup(A)
        dev.synchronize()
        gmg_first_s = time.perf_counter() - t0
        gmg.reuse_setup = True
        candidates["gmg"] = gmg
    x, z = dev.zeros(dh.ndofs), dev.zeros(dh.ndofs)
    preroll(dev, lambda: amg.apply(db, z))

    def timed(fn):
        e0, e1 = dev.event(), dev.event()
        e0.record()
        out = fn()
        e1.record()
        dev.synchronize()
        return e0.elapsed_ms(e1), out

    def solve(precond):
        x.fill_zero()
        return tb.pcg_solve(pattern, A, db, x, rtol=args.rtol, atol=0.0, maxiter=args.jacobi_maxiter, precond=precond)

    amg.reuse_setup = True                                          # the set-ups are timed on their own below
    for p in candidates.values():                                   # warm every shape
        solve(p)
    setup_ms, setup_wall_ms, gmg_setup_ms, cycle_ms, solve_ms, iters, converged = [], [], [], [], {k: [] for k in candidates}, {}, {}
    for _ in range(args.reps):
        t0 = time.perf_counter()
        setup_ms.append(timed(lambda: amg.setup(A))[0])
        setup_wall_ms.append(1e3 * (time.perf_counter() - t0))
        if gh is not None:
            gmg_setup_ms.append(timed(lambda: gmg.setup(A))[0])
        cycle_ms.append(timed(lambda: [amg.apply(db, z) for _ in range(10)])[0] / 10)
        for name, p in candidates.items():
            ms_, (its, res) = timed(lambda: solve(p))
            solve_ms[name].append(ms_)
            iters[name], converged[name] = its, bool(tb.solve_converged(pattern, res))
    med = lambda v: float(np.median(v)) if len(v) else None         # noqa: E731
    nl = amg.n_levels
    out = {"problem": args.problem, "n": n, "cells": int(g.n_cells), "dofs": dh.ndofs, "nnz": sp.nnz, "dt": args.dt, "rtol": args.rtol, "theta": args.theta,
           "degree": args.degree, "interval_ratio": args.ratio, "max_coarse": args.max_coarse, "levels": [amg.level_size(l) for l in range(nl)],
           "lambda_max": [amg.lambda_max(l) for l in range(nl - 1)], "amg_first_setup_host_s": first_setup_s, "amg_numeric_setup_ms": med(setup_ms),
           "amg_numeric_setup_wall_ms": med(setup_wall_ms), "amg_cycle_ms": med(cycle_ms), "gmg_first_setup_host_s": gmg_first_s, "gmg_numeric_setup_ms": med(gmg_setup_ms),
           "solve_ms": {k: med(v) for k, v in solve_ms.items()}, "iterations": iters, "converged": converged, "device": dev.info()["name"]}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
