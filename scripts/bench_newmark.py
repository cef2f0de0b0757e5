#!/usr/bin/env python3
"""Times the fused Newmark inertia stage tb_newmark_stage (r += c·M(u − ũ), Jnz += c·Mnz in one pass over M) against the composition of entries that
predate it, on the same buffers: one vector kernel for d = u − ũ (tb_heat_matrix with Δt = 1 on the two vectors), tb_spmv_csr(M, d) into r, tb_axpy
over the non-zeros into J.  The stage is timed twice: what the entry point ships for the pattern (the block kernel on node-major numberings, the
composition itself elsewhere) and, on a second device pattern created under TB_NEWMARK_STAGE=rows, its fused general kernel.  The
three candidates alternate inside one loop, so a drift of the clocks meets all of them alike; the line carries the median and the quartiles of each.
Beside the times: the streaming bound (Mnz read once, Jnz read and written, u, ũ and r) at the HBM3E peak of 8.0 TB/s and at the 6.29 TB/s a copy
kernel reaches, and the share of one Newton iteration (linearise + stage + eliminate + inner solve) the stage takes.
HIP events, a pre-roll, the median of --reps alternations.  Prints one JSON line."""
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
    ap.add_argument("--n", type=int, default=80, help="cells per side of the box")
    ap.add_argument("--order", type=int, default=1, choices=[1, 2])
    ap.add_argument("--mesh", default="box", choices=["box", "shuffled"], help="shuffled: the same box with its cells and nodes randomly renumbered")
    ap.add_argument("--numbering", default="natural", choices=["natural", "separated"],
                    help="separated: the dofs renumbered component by component (no 3x3 blocks: the general path of the stage and the CSR kernels of tb_spmv_csr)")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--newton", type=int, default=1, help="1: also time the parts of one Newton iteration of a Newmark step")
    args = ap.parse_args()
    import thunderbolt_jl_amd as tb
    from thunderbolt_jl_amd._lib import check
    lib = tb.lib()
    dev = tb.MI355XDevice(0)
    t0 = time.perf_counter()
    n = args.n
    g = tb.generate_mesh(tb.Hexahedron, (n, n, n), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    if args.mesh == "shuffled":
        rng = np.random.default_rng(1)
        pn, pc = rng.permutation(g.n_nodes), rng.permutation(g.n_cells)
        inv = np.empty_like(pn); inv[pn] = np.arange(g.n_nodes)
        g = tb.Grid(tb.Hexahedron, g.xyz[pn], inv[g.conn[pc]].astype(np.int32))
    dh = tb.DofHandler(g, tb.LagrangeCollection(args.order) ** 3)
    if args.numbering == "separated":
        dofs = np.arange(dh.ndofs)
        dh = tb.renumber_dofs(dh, ((dofs % 3) * (dh.ndofs // 3) + dofs // 3).astype(np.int32))
    sp = tb.allocate_matrix(dh)
    strategy = tb.ElementAssemblyStrategy(dev)
    Mop = tb.setup_operator(strategy, tb.BilinearMassIntegrator(tb.ConstantCoefficient(1.0e3)), dh, sp)
    dev.synchronize()
    ta = time.perf_counter()
    tb.update_operator(Mop, 0.0)
    dev.synchronize()
    mass_assembly_s = time.perf_counter() - ta
    setup_s = time.perf_counter() - t0
    pat, M = Mop.pattern, Mop.A
    nd, nnz = dh.ndofs, sp.nnz
    rng = np.random.default_rng(0)
    u, ut, r, d = (dev.to_device(rng.standard_normal(nd)) for _ in range(4))
    J = dev.to_device(rng.standard_normal(nnz))
    c = 1.0 / (0.25 * 5e-3 ** 2)

    def fused():
        check(lib.tb_newmark_stage(pat.h, M.ptr, c, u.ptr, ut.ptr, J.ptr, r.ptr))

    pat_rows = []

    def fused_rows():
        if not pat_rows:                                      # the switch is read at a pattern's first stage call: a second device pattern of the same arrays
            os.environ["TB_NEWMARK_STAGE"] = "rows"
            try:
                pat_rows.append(type(pat)(Mop.dmesh, sp))
                check(lib.tb_newmark_stage(pat_rows[0].h, M.ptr, c, u.ptr, ut.ptr, J.ptr, r.ptr))
            finally:
                del os.environ["TB_NEWMARK_STAGE"]
            assert lib.tb_last_kernel_name().decode() == "k_newmark_stage_csr"
            return
        check(lib.tb_newmark_stage(pat_rows[0].h, M.ptr, c, u.ptr, ut.ptr, J.ptr, r.ptr))

    def composition():
        check(lib.tb_heat_matrix(dev.h, nd, u.ptr, ut.ptr, 1.0, d.ptr))       # d = u − 1·ũ: one vector kernel
        check(lib.tb_spmv_csr(pat.h, M.ptr, d.ptr, c, 1.0, r.ptr))
        check(lib.tb_axpy(dev.h, nnz, c, M.ptr, J.ptr))

    fused()
    default_kernel = lib.tb_last_kernel_name().decode()
    candidates = {"fused": fused, "composition": composition}
    if default_kernel != "k_newmark_stage_csr":             # what the entry ships is not the fused general kernel: time that one too
        candidates["fused_general_path"] = fused_rows
    for fn in candidates.values():
        fn()
    preroll(dev, composition)
    samples = {k: [] for k in candidates}
    for _ in range(args.reps):
        for k, fn in candidates.items():
            e0, e1 = dev.event(), dev.event()
            e0.record(); fn(); e1.record()
            dev.synchronize()
            samples[k].append(e0.elapsed_ms(e1))
    stats = {k: {"median_ms": float(np.median(v)), "q25_ms": float(np.percentile(v, 25)), "q75_ms": float(np.percentile(v, 75)), "min_ms": float(np.min(v))}
             for k, v in samples.items()}
    bound_bytes = 24 * nnz + 32 * nd                                          # Mnz once, Jnz read + written, u, ũ, r read + written
    t_f = stats["fused"]["median_ms"]
    out = {"workload": "Newmark inertia stage, %s hex Q%d %d^3, %s numbering" % (args.mesh, args.order, n, args.numbering), "ndofs": int(nd), "nnz": int(nnz), "stage_kernel": default_kernel,
           "times": stats, "fused_over_composition": t_f / stats["composition"]["median_ms"],
           "streaming_bound_bytes": int(bound_bytes), "bound_ms_at_8.0TBs": bound_bytes / 8.0e9, "bound_ms_at_6.29TBs": bound_bytes / 6.29e9,
           "fraction_of_bound_8.0TBs": bound_bytes / 8.0e9 / t_f, "fraction_of_bound_6.29TBs": bound_bytes / 6.29e9 / t_f,
           "setup_s": setup_s, "mass_assembly_s": mass_assembly_s}
    if "fused_general_path" in stats:
        out["block_over_general_path"] = t_f / stats["fused_general_path"]["median_ms"]
    if args.newton and args.numbering == "natural":       # the mechanics kernels need a node's three dofs side by side
        # one Newton iteration of a Newmark step: the box clamped at x = 0, a small random displacement, Δt = 5 ms
        ms = tb.ConstantCoefficient(tb.OrthotropicMicrostructure([1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0]))
        op = tb.setup_operator(strategy, tb.QuasiStaticModel("d", tb.PK1Model(tb.Guccione1991PassiveModel(), ms)), dh, sp)
        X = tb.dof_coordinates(dh)
        ch = tb.ConstraintHandler(dh, np.flatnonzero(X[:, 0] < 1e-12))
        uu = rng.uniform(-1e-4, 1e-4, nd)
        uu[ch.prescribed_dofs] = 0.0
        uu = dev.to_device(uu)
        res, du = dev.zeros(nd), dev.zeros(nd)
        newton = tb.NewtonRaphsonSolver(inner_solver="cg", inner_rtol=1e-8, inner_maxiter=20000)

        def timed(fn, reps=3):
            ts = []
            for _ in range(reps):
                dev.synchronize()
                t = time.perf_counter()
                v = fn()
                dev.synchronize()
                ts.append(time.perf_counter() - t)
            return float(np.median(ts)) * 1e3, v

        def stage():
            check(lib.tb_newmark_stage(op.pattern.h, M.ptr, c, uu.ptr, ut.ptr, op.J.ptr, res.ptr))

        def solve():
            du.fill_zero()
            return tb.inner_linear_solve(newton, op.pattern, op.J, res, du, newton.inner_rtol)[0]

        tb.update_linearization(op, uu, 0.0, residual=res)                    # plans
        t_lin, _ = timed(lambda: tb.update_linearization(op, uu, 0.0, residual=res))
        t_stage, _ = timed(stage)
        tb.update_linearization(op, uu, 0.0, residual=res)
        stage()
        t_elim, _ = timed(lambda: tb.apply_zero(op.J, res, ch, pattern=op.pattern), reps=1)
        t_solve, its = timed(solve)
        total = t_lin + t_stage + t_elim + t_solve
        out["newton_iteration"] = {"linearise_ms": t_lin, "stage_ms": t_stage, "eliminate_ms": t_elim, "inner_solve_ms": t_solve, "cg_iterations": int(its),
                                   "stage_share": t_stage / total}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
