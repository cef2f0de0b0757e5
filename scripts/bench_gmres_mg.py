#!/usr/bin/env python3
"""Times multigrid-preconditioned GMRES against Jacobi-GMRES(200) on one non-symmetric tangent under a follower pressure, in one process:
  --problem q1    Holzapfel–Ogden Q1 beam of 4n × n × n cells on 4 × 1 × 1, x = 0 clamped, pressure on the bottom face;
                  AMGPrecon(near_nullspace="rigid_body")
  --problem q2    the same beam with a second-order field; ChainedMGPrecon(PMGPrecon(), AMGPrecon(near_nullspace="rigid_body"))
  --problem ring  the Guccione ring of the multigrid how-to (16 × 1 × 1 cells refined --refinements times), "Myocardium" clamped, pressure on the
                  endocardium; GMGPrecon(gh)
The tangent is taken at the displacement a few Newton steps under the load reach (Jacobi-GMRES, loose tolerance), so the follower term is in it.
Candidates: Jacobi-GMRES(200), multigrid-GMRES(--restart) with the hierarchy in its default mode (general = 0: symmetrised coarsest inverse) and in
general mode (general = 1: pivoted, unsymmetrised).  Reported per candidate: Arnoldi steps, wall milliseconds per solve (the loop reads the host
once per step, so wall time is the figure), converged.  Host-read share of the multigrid solve, two estimates: `round_trip_share` = steps × the wall
time of one scalar read-back on an idle queue (tb.dot on 64 doubles: a launch, an 8-byte copy, a stream synchronisation) / wall time of the solve;
`outside_cycle_and_product_share` = 1 − steps × (event-timed cycle + product enqueued back to back) / wall time: everything a step spends outside
its two large pieces — Gram–Schmidt kernels, the host read, the host's Givens update and the launch gaps.  The candidates alternate inside each
repetition, medians over --reps, a pre-roll.  Prints one JSON line and, with --out, writes it to a file."""
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
    ap.add_argument("--problem", default="q1", choices=["q1", "q2", "ring"])
    ap.add_argument("--n", type=int, default=8, help="q1, q2: cells across (4n along)")
    ap.add_argument("--refinements", type=int, default=2, help="ring: uniform refinements of the 16 x 1 x 1 ring")
    ap.add_argument("--pressure", type=float, default=None, help="follower pressure (default: 0.001 on the beam, 0.01 on the ring)")
    ap.add_argument("--rtol", type=float, default=1e-8)
    ap.add_argument("--restart", type=int, default=50)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--max-coarse", type=int, default=1024)
    ap.add_argument("--maxiter", type=int, default=20000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import thunderbolt_jl_amd as tb
    dev = tb.MI355XDevice(0)
    ms = tb.ConstantCoefficient(tb.OrthotropicMicrostructure(*np.eye(3)))
    if args.problem == "ring":
        gh = tb.GridHierarchy(tb.generate_ring_mesh(16, 1, 1), args.refinements)
        g = gh.grids[-1]
        dh = tb.DofHandler(g, tb.LagrangeCollection(1) ** 3)
        fs = g.facetset("Myocardium")
        nodes = np.unique(g.conn[fs[:, 0][:, None], np.asarray(tb.Grid.HEX_FACETS)[fs[:, 1]]])
        node_dof0 = np.empty(g.n_nodes, dtype=np.int64)
        node_dof0[g.conn.ravel()] = dh.cell_dofs[:, 0::3].ravel()
        fixed = (node_dof0[nodes][:, None] + np.arange(3)).ravel()
        p = 0.01 if args.pressure is None else args.pressure
        model = tb.QuasiStaticModel("d", tb.PK1Model(tb.Guccione1991PassiveModel(), ms), [tb.PressureFieldBC(tb.ConstantCoefficient(p), "Endocardium")])
        recipe = tb.GMGPrecon(gh)
    else:
        n = args.n
        g = tb.generate_mesh(tb.Hexahedron, (4 * n, n, n), (0, 0, 0), (4, 1, 1))
        dh = tb.DofHandler(g, tb.LagrangeCollection(2 if args.problem == "q2" else 1) ** 3)
        fixed = np.flatnonzero(np.abs(tb.dof_coordinates(dh)[:, 0]) < 1e-12)
        p = 0.001 if args.pressure is None else args.pressure
        model = tb.QuasiStaticModel("d", tb.PK1Model(tb.HolzapfelOgden2009Model(a=1.0, b=1.0, af=0.0, as_=0.0, afs=0.0, beta=1.0), ms),
                                    [tb.PressureFieldBC(tb.ConstantCoefficient(p), "bottom")])
        amg = tb.AMGPrecon(max_coarse=args.max_coarse, near_nullspace="rigid_body")
        recipe = tb.ChainedMGPrecon(tb.PMGPrecon(), amg) if args.problem == "q2" else amg
    sp = tb.allocate_matrix(dh)
    ch = tb.ConstraintHandler(dh, fixed)
    op = tb.setup_operator(tb.ElementAssemblyStrategy(dev), model, dh, sp)
    # the state the tangent is taken at: a few loosely solved Newton steps under the load
    u = dev.zeros(dh.ndofs)
    newton = tb.NewtonRaphsonSolver(max_iter=3, tol=1e-6, inner_rtol=1e-4, inner_solver="gmres", gmres_restart=200, inner_maxiter=4000, strict_inner_solve=False,
                                    enforce_monotonic_convergence=False)
    tb.nlsolve(u, op, ch, newton)
    res = dev.zeros(dh.ndofs)
    tb.update_linearization(op, u, 0.0, residual=res)
    pattern = op.pattern
    A = dev.to_device(op.J.to_host())
    tb.apply_zero(A, res, ch, pattern=pattern)
    hA = A.to_host()
    rows = np.repeat(np.arange(dh.ndofs), np.diff(sp.rowptr))
    diag_positive = bool((hA[rows == sp.colidx] > 0).all())
    import scipy.sparse as sparse
    M = sparse.csr_matrix((hA, sp.colidx.astype(np.int32), sp.rowptr.astype(np.int64)), shape=(dh.ndofs, dh.ndofs))
    skew_share = float(abs(M - M.T).max() / abs(M).max())      # 2 × the largest entry of the skew part over the largest entry
    b = np.random.default_rng(0).uniform(0.0, 1.0, dh.ndofs)
    b[ch.prescribed_dofs] = 0.0
    db = dev.to_device(b)
    mg = recipe.materialize(pattern, ch)
    x, z = dev.zeros(dh.ndofs), dev.zeros(dh.ndofs)
    dev.synchronize()

    def jacobi():
        x.fill_zero()
        return tb.gmres_solve(pattern, A, db, x, rtol=args.rtol, atol=0.0, maxiter=args.maxiter, restart=200)

    def multigrid(general):
        def run():
            x.fill_zero()
            return mg.solve_gmres(A, db, x, rtol=args.rtol, atol=0.0, maxiter=args.maxiter, restart=args.restart, setup=False, general=general)
        return run

    candidates = {"jacobi_gmres200": jacobi, "mg_gmres_general0": multigrid(False), "mg_gmres_general1": multigrid(True)}
    mg.set_general(True).setup(A)
    preroll(dev, lambda: mg.apply(db, z))

    def wall(fn):
        dev.synchronize()
        t0 = time.perf_counter()
        out = fn()
        dev.synchronize()
        return 1e3 * (time.perf_counter() - t0), out

    def events(fn, reps):
        e0, e1 = dev.event(), dev.event()
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        dev.synchronize()
        return e0.elapsed_ms(e1) / reps

    setup_ms = {}
    for general in (False, True):                                   # the numeric set-up a Newton iteration repeats, per mode (wall: it reads λ back)
        mg.set_general(general)
        mg.setup(A)
        setup_ms["general%d" % general] = float(np.median([wall(lambda: mg.setup(A))[0] for _ in range(3)]))
    for fn in candidates.values():                                  # warm every shape (each multigrid candidate sets up when it flips the mode: untimed here)
        fn()
    solve_ms, iters, converged = {k: [] for k in candidates}, {}, {}
    tiny = dev.zeros(64)
    trip_ms, step_ms = [], []
    for _ in range(args.reps):
        for name, fn in candidates.items():
            if name.startswith("mg"):
                fn()                                                # the flip's set-up stays outside the timed solve
            ms_, (its, r) = wall(fn)
            solve_ms[name].append(ms_)
            iters[name], converged[name] = its, bool(tb.solve_converged(pattern, r))
        t0 = time.perf_counter()
        for _ in range(200):
            tb.dot(tiny, tiny)
        trip_ms.append(1e3 * (time.perf_counter() - t0) / 200)
        step_ms.append(events(lambda: (mg.apply(db, z), tb.check(tb.lib().tb_spmv_csr(pattern.h, A.ptr, z.ptr, 1.0, 0.0, x.ptr))), 20))
    med = lambda v: float(np.median(v))                             # noqa: E731
    t_mg, k_mg = med(solve_ms["mg_gmres_general1"]), iters["mg_gmres_general1"]
    out = {"problem": args.problem, "cells": int(g.n_cells), "dofs": dh.ndofs, "nnz": sp.nnz, "rtol": args.rtol, "restart": args.restart, "pressure": p,
           "diagonal_positive": diag_positive, "skew_share_of_largest_entry": skew_share, "levels": mg.n_levels,
           "iterations": iters, "converged": converged, "solve_wall_ms": {k: med(v) for k, v in solve_ms.items()}, "numeric_setup_wall_ms": setup_ms,
           "scalar_round_trip_ms": med(trip_ms), "cycle_plus_product_ms": med(step_ms),
           "round_trip_share": k_mg * med(trip_ms) / t_mg, "outside_cycle_and_product_share": 1.0 - k_mg * med(step_ms) / t_mg,
           "device": dev.info()["name"]}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
