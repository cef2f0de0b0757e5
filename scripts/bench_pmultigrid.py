#!/usr/bin/env python3
"""Times the p-multigrid preconditioner (ChainedMGPrecon(PMGPrecon(), GMGPrecon(gh)), tb_mg_*) on the second-order tangent of a hyperelastic box against
the one-level preconditioners on the same matrix, in one process:
  --material guccione | ho   the Q2 tangent (3 components) at a smooth 1 % stretch on an n³ box, the face x = 0 clamped
The hierarchy is a --coarse³ box refined until it has n cells per side; the Q2 field sits on top of the first-order levels.  Reported: host seconds of
the plans (first tb_mg_setup), per transfer which Galerkin plan it took, its terms and device bytes (tb_mg_level_plan), milliseconds of the numeric
set-up a Newton iteration repeats and of the Galerkin chain inside it (tb_mg_galerkin, level by level; the rest is the λmax estimates and the
coarsest inverse), milliseconds per cycle, and for multigrid, Jacobi and Chebyshev(16) the iterations and milliseconds of the solve to --rtol; the
candidates alternate inside each repetition, medians over --reps.  HIP events around enqueued work, a device synchronise at the end, a pre-roll.

--galerkin-compare times k_mg_galerkin_b3 against k_mg_galerkin on the same p-level: a second hierarchy of the same pattern is planned per dof
(TB_MG_GALERKIN=dof, a switch of the profiling build only: run with TB_LIBTBHIP pointing at libtbhip_ablation.so), the two products alternate, and
each time is set against the bytes the kernel has to move (fine values once, terms, pointers, block-row table, coarse values) and the rate of a
device-to-device copy of the fine matrix measured in the same process.  Prints one JSON line and, with --out, writes it to a file."""
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
    ap.add_argument("--material", default="guccione", choices=["guccione", "ho"])
    ap.add_argument("--n", type=int, default=16, help="cells per side of the fine box")
    ap.add_argument("--coarse", type=int, default=2, help="cells per side of the coarsest box (n / coarse must be a power of two)")
    ap.add_argument("--rtol", type=float, default=1e-8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--degree", type=int, default=2)
    ap.add_argument("--ratio", type=float, default=4.0)
    ap.add_argument("--maxiter", type=int, default=20000)
    ap.add_argument("--skip", default="", help="comma-separated one-level candidates to leave out (jacobi, chebyshev16)")
    ap.add_argument("--galerkin-compare", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import thunderbolt_jl_amd as tb
    from thunderbolt_jl_amd._lib import check, lib
    refinements = int(round(np.log2(args.n / args.coarse)))
    assert args.coarse * 2 ** refinements == args.n and refinements >= 0, "n / coarse must be a power of two"
    dev = tb.MI355XDevice(0)
    start = time.perf_counter()

    def stage(what):                                                # progress on stderr: the large sizes spend minutes on the host before the first kernel
        print("[%7.1f s] %s" % (time.perf_counter() - start, what), file=sys.stderr, flush=True)

    t0 = time.perf_counter()
    c = args.coarse
    gh = tb.GridHierarchy(tb.generate_mesh(tb.Hexahedron, (c, c, c), (0, 0, 0), (1, 1, 1)), refinements)
    hierarchy_s = time.perf_counter() - t0
    dh = tb.DofHandler(gh.grids[-1], tb.LagrangeCollection(2) ** 3)
    sp = tb.allocate_matrix(dh)
    stage("grid hierarchy, dof handler and pattern: %d dofs, %d non-zeros" % (dh.ndofs, sp.nnz))
    X = tb.dof_coordinates(dh)
    comp = np.empty(dh.ndofs, dtype=np.int64)
    for k in range(3):
        comp[dh.cell_dofs[:, k::3].ravel()] = k
    ch = tb.ConstraintHandler(dh, np.flatnonzero(X[:, 0] == 0.0))
    if args.material == "guccione":
        pk1 = tb.PK1Model(tb.Guccione1991PassiveModel(), tb.ConstantCoefficient(tb.OrthotropicMicrostructure([1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0])))
    else:
        f, s, n = np.array([1, 1, 0.0]) / np.sqrt(2), np.array([-1, 1, 0.0]) / np.sqrt(2), np.array([0, 0, 1.0])
        pk1 = tb.PK1Model(tb.HolzapfelOgden2009Model(), tb.ConstantCoefficient(tb.OrthotropicMicrostructure(f, s, n)))
    op = tb.setup_operator(tb.ElementAssemblyStrategy(dev), tb.QuasiStaticModel("d", pk1), dh, sp)
    u = np.array([0.01, -0.003, -0.003])[comp] * X[np.arange(dh.ndofs), comp]   # a smooth 1 % stretch along x with lateral contraction
    u[ch.prescribed_dofs] = 0.0
    tb.update_linearization(op, dev.to_device(u), 0.0, residual=dev.zeros(dh.ndofs))
    pattern, A = op.pattern, op.J
    tb.apply_zero(A, None, ch, pattern=pattern)
    b = np.random.default_rng(0).uniform(0.0, 1.0, dh.ndofs)
    b[ch.prescribed_dofs] = 0.0
    db = dev.to_device(b)
    stage("tangent assembled and eliminated")
    t0 = time.perf_counter()
    mg = tb.ChainedMGPrecon(tb.PMGPrecon(degree=args.degree, interval_ratio=args.ratio), tb.GMGPrecon(gh, args.degree, args.ratio)).materialize(pattern, ch)
    mg.setup(A)
    dev.synchronize()
    plan_s = time.perf_counter() - t0
    stage("plans and first set-up")
    top = mg.n_levels - 1
    plans = [{"fine_level": l, "fine_dofs": mg.dhs[l].ndofs, "fine_nnz": mg.sps[l].nnz, "blocked": mg.plan(l)[0], "terms": mg.plan(l)[1], "plan_bytes": mg.plan_bytes(l)}
             for l in range(top, 0, -1)]
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
        return tb.pcg_solve(pattern, A, db, x, rtol=args.rtol, atol=0.0, maxiter=args.maxiter, precond=precond)

    skip = set(args.skip.split(",")) if args.skip else set()
    candidates = {k: v for k, v in {"multigrid": mg, "jacobi": "jacobi", "chebyshev16": tb.ChebyshevPrecBuilder(16)}.items() if k not in skip}
    mg.reuse_setup = True                                           # the set-up is timed on its own below
    for name, p in candidates.items():                              # warm every shape
        solve(p)
        stage("warm-up solve: " + name)
    setup_ms, chain_ms, cycle_ms, solve_ms, iters, converged = [], [], [], {k: [] for k in candidates}, {}, {}
    for _ in range(args.reps):
        setup_ms.append(timed(lambda: mg.setup(A))[0])
        chain_ms.append(timed(lambda: [mg.galerkin(l) for l in range(top, 0, -1)])[0])
        cycle_ms.append(timed(lambda: [mg.apply(db, z) for _ in range(10)])[0] / 10)
        for name, p in candidates.items():
            ms_, (its, res) = timed(lambda: solve(p))
            solve_ms[name].append(ms_)
            iters[name], converged[name] = its, bool(tb.solve_converged(pattern, res))
        stage("repetition %d" % (len(setup_ms)))
    med = lambda v: float(np.median(v))                             # noqa: E731
    out = {"material": args.material, "n": args.n, "coarse": args.coarse, "levels": mg.n_levels, "dofs": dh.ndofs, "nnz": sp.nnz, "rtol": args.rtol,
           "degree": args.degree, "interval_ratio": args.ratio, "hierarchy_host_s": hierarchy_s, "plans_and_first_setup_host_s": plan_s, "plans": plans,
           "setup_ms": med(setup_ms), "galerkin_chain_ms": med(chain_ms), "lambda_max_and_coarsest_inverse_ms": med(setup_ms) - med(chain_ms),
           "cycle_ms": med(cycle_ms), "lambda_max": [mg.lambda_max(l) for l in range(1, mg.n_levels)],
           "solve_ms": {k: med(v) for k, v in solve_ms.items()}, "iterations": iters, "converged": converged,
           "multigrid_solve_plus_setup_ms": med(solve_ms["multigrid"]) + med(setup_ms), "device": dev.info()["name"]}

    if args.galerkin_compare:
        os.environ["TB_MG_GALERKIN"] = "dof"
        mgd = tb.MultigridHierarchy(pattern, gh, args.degree, args.ratio, ch, p_level=True).setup(A)
        del os.environ["TB_MG_GALERKIN"]
        if mg.plan(top)[0] is not True or mgd.plan(top)[0] is not False:
            sys.exit("--galerkin-compare: the p-level must take the blocked plan by default and the per-dof plan under TB_MG_GALERKIN=dof "
                     "(the profiling build reads the switch: TB_LIBTBHIP=…/libtbhip_ablation.so); got blocked = %s / %s" % (mg.plan(top)[0], mgd.plan(top)[0]))
        a, d = mg.level_matrix(top - 1), mgd.level_matrix(top - 1)
        scratch = dev.zeros(sp.nnz)
        copy = lambda: check(lib().tb_memcpy_d2d(dev.h, scratch.ptr, A.ptr, 8 * sp.nnz))   # noqa: E731
        preroll(dev, lambda: mg.galerkin(top))
        k = 5
        t = {"blocked": [], "dof": [], "copy": []}
        for _ in range(max(args.reps, 7)):
            t["blocked"].append(timed(lambda: [mg.galerkin(top) for _ in range(k)])[0] / k)
            t["dof"].append(timed(lambda: [mgd.galerkin(top) for _ in range(k)])[0] / k)
            t["copy"].append(timed(lambda: [copy() for _ in range(k)])[0] / k)
        nnz_f, nnz_c = mg.sps[top].nnz, mg.sps[top - 1].nnz
        bytes_ = {"blocked": 8 * nnz_f + 4 * mg.plan(top)[1] + 4 * (nnz_f // 9) + 8 * (nnz_c // 9 + 1) + 8 * nnz_c,
                  "dof": 8 * nnz_f + 4 * mgd.plan(top)[1] + 8 * (nnz_c + 1) + 8 * nnz_c}
        copy_gbs = 2 * 8 * sp.nnz / med(t["copy"]) * 1e-6
        out["galerkin"] = {"results_differ_by": float(np.abs(a - d).max() / np.abs(d).max()), "copy_GBps": copy_gbs,
                           **{name: {"ms": med(t[name]), "min_ms": float(np.min(t[name])), "max_ms": float(np.max(t[name])), "bytes": bytes_[name],
                                     "GBps": bytes_[name] / med(t[name]) * 1e-6, "share_of_copy_rate": bytes_[name] / med(t[name]) * 1e-6 / copy_gbs,
                                     "terms": (mg if name == "blocked" else mgd).plan(top)[1], "plan_bytes": (mg if name == "blocked" else mgd).plan_bytes(top)}
                              for name in ("blocked", "dof")}}
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
