#!/usr/bin/env python3
"""Times the smoothed-aggregation multigrid with rigid-body modes (AMGPrecon(near_nullspace="rigid_body")) against the other preconditioners on one
elasticity tangent, in one process:
  --problem beam       the Holzapfel–Ogden tangent at a small random displacement on a Q1 bar of 4n × n × n cells on 4 × 1 × 1, x = 0 clamped; with
                       --coarse the geometric multigrid of a (4·coarse, coarse, coarse) bar refined to n runs beside it
  --problem ventricle  the same tangent on the generated ideal left ventricle (n cells around, n / 4 through the wall, n along), the base clamped
  --problem q2         the second-order tangent on the bar; the AMGs sit below the p-level: ChainedMGPrecon(PMGPrecon(), AMGPrecon(…))
Candidates: Jacobi, Chebyshev(16), AMGPrecon() (translations only), the rigid-body recipe, and GMGPrecon where a hierarchy exists.  Reported per
candidate: iterations and milliseconds of the solve to --rtol; per AMG: host seconds of the first set-up, milliseconds of the numeric set-up a Newton
iteration repeats, milliseconds per cycle, the levels and the operator complexity Σ nnz_l / nnz_0 (the 6 × 6 coarse blocks make the coarse levels
denser: this is the cost to show).  The candidates alternate inside each repetition, medians over --reps, HIP events around enqueued work, a
pre-roll.  Prints one JSON line and, with --out, writes it to a file."""
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
    ap.add_argument("--problem", default="beam", choices=["beam", "ventricle", "q2"])
    ap.add_argument("--n", type=int, default=8, help="beam, q2: cells across (4n along); ventricle: cells around, a multiple of 4")
    ap.add_argument("--coarse", type=int, default=0, help="beam: cells across of the coarsest grid of the geometric multigrid run beside the AMGs (0: none)")
    ap.add_argument("--rtol", type=float, default=1e-8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--theta", type=float, default=0.25)
    ap.add_argument("--max-coarse", type=int, default=1024)
    ap.add_argument("--maxiter", type=int, default=20000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import thunderbolt_jl_amd as tb
    dev = tb.MI355XDevice(0)
    n, gh = args.n, None
    if args.problem == "ventricle":
        g = tb.generate_ideal_lv_mesh_hex(n, max(n // 4, 1), n)
    elif args.problem == "beam" and args.coarse:
        refinements = int(round(np.log2(n / args.coarse)))
        assert args.coarse * 2 ** refinements == n and refinements >= 1, "n / coarse must be a power of two"
        gh = tb.GridHierarchy(tb.generate_mesh(tb.Hexahedron, (4 * args.coarse, args.coarse, args.coarse), (0, 0, 0), (4, 1, 1)), refinements)
        g = gh.grids[-1]
    else:
        g = tb.generate_mesh(tb.Hexahedron, (4 * n, n, n), (0, 0, 0), (4, 1, 1))
    q2 = args.problem == "q2"
    dh = tb.DofHandler(g, tb.LagrangeCollection(2 if q2 else 1) ** 3)
    sp = tb.allocate_matrix(dh)
    X = tb.dof_coordinates(dh)
    fixed = np.flatnonzero(X[:, 2] >= X[:, 2].max() - 1e-9) if args.problem == "ventricle" else np.flatnonzero(np.abs(X[:, 0]) < 1e-12)
    ch = tb.ConstraintHandler(dh, fixed)
    model = tb.QuasiStaticModel("d", tb.PK1Model(tb.HolzapfelOgden2009Model(), tb.ConstantCoefficient(tb.OrthotropicMicrostructure(*np.eye(3)))), [])
    op = tb.setup_operator(tb.ElementAssemblyStrategy(dev), model, dh, sp)
    u = np.random.default_rng(5).uniform(-1e-3, 1e-3, dh.ndofs)
    u[fixed] = 0.0
    tb.update_linearization(op, dev.to_device(u), 0.0, residual=dev.zeros(dh.ndofs))
    pattern = op.pattern
    A = dev.to_device(op.J.to_host())
    tb.apply_zero(A, None, ch, pattern=pattern)
    b = np.random.default_rng(0).uniform(0.0, 1.0, dh.ndofs)
    b[ch.prescribed_dofs] = 0.0
    db = dev.to_device(b)
    dev.synchronize()

    def recipe(**kw):
        r = tb.AMGPrecon(theta=args.theta, max_coarse=args.max_coarse, **kw)
        return tb.ChainedMGPrecon(tb.PMGPrecon(), r) if q2 else r

    first_s, amgs = {}, {}
    for name, kw in (("amg", {}), ("amg_rigid_body", {"near_nullspace": "rigid_body"})):
        t0 = time.perf_counter()
        amgs[name] = recipe(**kw).materialize(pattern, ch)
        amgs[name].setup(A)
        dev.synchronize()
        first_s[name] = time.perf_counter() - t0
    candidates = {"jacobi": "jacobi", "chebyshev16": tb.ChebyshevPrecBuilder(16), **amgs}
    if gh is not None:
        candidates["gmg"] = tb.MultigridHierarchy(pattern, gh, 2, 4.0, ch).setup(A)
    for p in candidates.values():
        if hasattr(p, "reuse_setup"):
            p.reuse_setup = True                                    # the set-ups are timed on their own below
    x, z = dev.zeros(dh.ndofs), dev.zeros(dh.ndofs)
    preroll(dev, lambda: amgs["amg_rigid_body"].apply(db, z))

    def timed(fn):
        e0, e1 = dev.event(), dev.event()
        e0.record()
        out = fn()
        e1.record()
        dev.synchronize()
        return e0.elapsed_ms(e1), out

    def solve(precond):
        x.fill_zero()
        return tb.pcg_solve(pattern, A, db, x, rtol=args.rtol, atol=0.0, maxiter=args.maxiter, precond=precond)

    for p in candidates.values():                                   # warm every shape
        solve(p)
    setup_ms, cycle_ms = {k: [] for k in amgs}, {k: [] for k in amgs}
    solve_ms, iters, converged = {k: [] for k in candidates}, {}, {}
    for _ in range(args.reps):
        for name, h in amgs.items():
            t0 = time.perf_counter()
            h.setup(A)
            dev.synchronize()
            setup_ms[name].append(1e3 * (time.perf_counter() - t0))   # wall: the numeric set-up reads λ back
            cycle_ms[name].append(timed(lambda: [h.apply(db, z) for _ in range(10)])[0] / 10)
        for name, p in candidates.items():
            ms_, (its, res) = timed(lambda: solve(p))
            solve_ms[name].append(ms_)
            iters[name], converged[name] = its, bool(tb.solve_converged(pattern, res))
    med = lambda v: float(np.median(v)) if len(v) else None         # noqa: E731

    def levels_of(h):
        inner = h.coarse_hierarchy() if q2 else h
        sizes = [inner.level_size(l) for l in range(inner.n_levels)]
        return sizes, sum(s[1] for s in sizes) / sizes[0][1]

    out = {"problem": args.problem, "n": n, "cells": int(g.n_cells), "dofs": dh.ndofs, "nnz": sp.nnz, "rtol": args.rtol, "theta": args.theta, "max_coarse": args.max_coarse,
           "levels": {k: levels_of(h)[0] for k, h in amgs.items()}, "operator_complexity": {k: levels_of(h)[1] for k, h in amgs.items()},
           "first_setup_host_s": first_s, "numeric_setup_wall_ms": {k: med(v) for k, v in setup_ms.items()}, "cycle_ms": {k: med(v) for k, v in cycle_ms.items()},
           "solve_ms": {k: med(v) for k, v in solve_ms.items()}, "iterations": iters, "converged": converged, "device": dev.info()["name"]}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
