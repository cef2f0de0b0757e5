#!/usr/bin/env python3
"""Times the geometric multigrid preconditioner (GMGPrecon, tb_mg_*) against the one-level preconditioners on the same system, in one process:
  --problem heat      M − Δt·K of the Q1 diffusion operator (tensor diag(9, 4, 4)) on an n³ box, Dirichlet on x = 0 (Δt = 0: −K, the Laplace solve)
  --problem guccione  the Q1 Guccione tangent at a small seeded displacement on an n³ box, the face x = 0 clamped
The hierarchy is a --coarse³ box refined until it has n cells per side.  Reported: host seconds of the plans (first tb_mg_setup), milliseconds of the
numeric set-up a Newton iteration repeats, milliseconds per cycle, and for every preconditioner the iterations and milliseconds of the solve to
--rtol; the candidates alternate inside each repetition so that a drift of the clocks meets all of them alike, medians over --reps.  The base of
any comparison is the fastest one-level preconditioner on this system.  HIP events around enqueued work, a device synchronise at the end, a
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
    ap.add_argument("--problem", default="heat", choices=["heat", "guccione"])
    ap.add_argument("--n", type=int, default=64, help="cells per side of the fine box")
    ap.add_argument("--coarse", type=int, default=4, help="cells per side of the coarsest box (n / coarse must be a power of two)")
    ap.add_argument("--dt", type=float, default=0.0, help="heat: A = M − Δt·K; 0: A = −K")
    ap.add_argument("--rtol", type=float, default=1e-8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--degree", type=int, default=2)
    ap.add_argument("--ratio", type=float, default=4.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import thunderbolt_jl_amd as tb
    refinements = int(round(np.log2(args.n / args.coarse)))
    assert args.coarse * 2 ** refinements == args.n and refinements >= 1, "n / coarse must be a power of two"
    dev = tb.MI355XDevice(0)
    t0 = time.perf_counter()
    c = args.coarse
    gh = tb.GridHierarchy(tb.generate_mesh(tb.Hexahedron, (c, c, c), (0, 0, 0), (1, 1, 1)), refinements)
    hierarchy_s = time.perf_counter() - t0
    g = gh.grids[-1]
    ncomp = 3 if args.problem == "guccione" else 1
    dh = tb.DofHandler(g, tb.LagrangeCollection(1, ncomp))
    sp = tb.allocate_matrix(dh)
    node_dofs = np.empty((g.n_nodes, ncomp), dtype=np.int64)
    for k in range(ncomp):
        node_dofs[g.conn.ravel(), k] = dh.cell_dofs[:, k::ncomp].ravel()
    ch = tb.ConstraintHandler(dh, node_dofs[g.xyz[:, 0] == 0.0].ravel())
    rng = np.random.default_rng(0)
    if args.problem == "heat":
        st = tb.PatchAssemblyStrategy(dev)
        D = tb.ConductivityToDiffusivityCoefficient(tb.ConstantCoefficient(np.diag([9.0, 4.0, 4.0])), tb.ConstantCoefficient(1.0), tb.ConstantCoefficient(1.0))
        K = tb.update_operator(tb.setup_operator(st, tb.BilinearDiffusionIntegrator(D), dh, sp), 0.0)
        pattern = K.pattern
        vals = -K.A.to_host()
        if args.dt > 0:
            M = tb.update_operator(tb.setup_operator(st, tb.BilinearMassIntegrator(tb.ConstantCoefficient(1.0)), dh, sp), 0.0)
            vals = M.A.to_host() + args.dt * vals
        A = dev.to_device(vals)
    else:
        ms = tb.ConstantCoefficient(tb.OrthotropicMicrostructure([1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0]))
        op = tb.setup_operator(tb.ElementAssemblyStrategy(dev), tb.QuasiStaticModel("d", tb.PK1Model(tb.Guccione1991PassiveModel(), ms)), dh, sp)
        X = tb.dof_coordinates(dh)                                   # a smooth 1 % stretch along x with lateral contraction: strains stay small at any h
        u = np.zeros(dh.ndofs)
        for k, s in enumerate((0.01, -0.003, -0.003)):
            u[node_dofs[:, k]] = s * X[node_dofs[:, k], k]
        u[ch.prescribed_dofs] = 0.0
        tb.update_linearization(op, dev.to_device(u), 0.0, residual=dev.zeros(dh.ndofs))
        pattern, A = op.pattern, op.J
    tb.apply_zero(A, None, ch, pattern=pattern)
    b = rng.uniform(0.0, 1.0, dh.ndofs)
    b[ch.prescribed_dofs] = 0.0
    db = dev.to_device(b)
    t0 = time.perf_counter()
    mg = tb.MultigridHierarchy(pattern, gh, args.degree, args.ratio, ch)
    mg.setup(A)
    dev.synchronize()
    plan_s = time.perf_counter() - t0
    x, z = dev.zeros(dh.ndofs), dev.zeros(dh.ndofs)
    preroll(dev, lambda: mg.apply(db, z))

    def timed(fn):
        e0, e1 = dev.event(), dev.event()
        e0.record()
        out = fn()
        e1.record()
        dev.synchronize()
        return e0.elapsed_ms(e1), out

    def solve(precond):
        x.fill_zero()
        return tb.pcg_solve(pattern, A, db, x, rtol=args.rtol, atol=0.0, maxiter=20000, precond=precond)

    candidates = {"multigrid": mg, "jacobi": "jacobi", "l1gs64": tb.L1GSPrecBuilder(64), "chebyshev16": tb.ChebyshevPrecBuilder(16)}
    mg.reuse_setup = True                                           # the set-up is timed on its own below
    for p in candidates.values():                                   # warm every shape
        solve(p)
    setup_ms, cycle_ms, solve_ms, iters, converged = [], [], {k: [] for k in candidates}, {}, {}
    for _ in range(args.reps):
        setup_ms.append(timed(lambda: mg.setup(A))[0])
        cycle_ms.append(timed(lambda: [mg.apply(db, z) for _ in range(10)])[0] / 10)
        for name, p in candidates.items():
            ms_, (its, res) = timed(lambda: solve(p))
            solve_ms[name].append(ms_)
            iters[name], converged[name] = its, bool(tb.solve_converged(pattern, res))
    med = lambda v: float(np.median(v))                             # noqa: E731
    one_level = {k: med(v) for k, v in solve_ms.items() if k != "multigrid"}
    base = min(one_level, key=one_level.get)
    mg_iter_ms = med(solve_ms["multigrid"]) / max(iters["multigrid"], 1)
    out = {"problem": args.problem, "n": args.n, "coarse": args.coarse, "levels": len(gh.grids), "dofs": dh.ndofs, "nnz": sp.nnz, "dt": args.dt, "rtol": args.rtol,
           "degree": args.degree, "interval_ratio": args.ratio, "hierarchy_host_s": hierarchy_s, "plans_and_first_setup_host_s": plan_s,
           "setup_ms": med(setup_ms), "cycle_ms": med(cycle_ms), "lambda_max": [mg.lambda_max(l) for l in range(1, mg.n_levels)],
           "solve_ms": {k: med(v) for k, v in solve_ms.items()}, "iterations": iters, "converged": converged,
           "base": base, "multigrid_plus_setup_over_base": (med(solve_ms["multigrid"]) + med(setup_ms)) / one_level[base],
           "setup_in_multigrid_pcg_iterations": med(setup_ms) / mg_iter_ms, "device": dev.info()["name"]}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
