#!/usr/bin/env python3
"""Times tb_chamber_assemble (all outputs) on the endocardium of the all-hex ideal ventricle at the size scripts/bench_electromechanics.py uses,
against tb_facet_assemble(TB_BC_PRESSURE) on the same facets (the baseline: the follower-load terms without the coupling blocks), and splits one
coupled Newton iteration into the volume pass, the chamber pass, the 1 + n_chambers inner solves and what is left (host work and the small kernels
of the constraint elimination and the increment).  The baseline is the k_facets of the tree the script runs in; --baseline-only times that call
alone, which also runs on a tree from before the chamber coupling.
HIP events, a pre-roll, the median of --reps launches.  Prints one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def median_ms(dev, fn, reps, preroll=5):
    for _ in range(preroll):
        fn()
    dev.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = dev.event(), dev.event()
        e0.record(); fn(); e1.record()
        dev.synchronize()
        out.append(e0.elapsed_ms(e1))
    return float(np.median(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nc", type=int, default=128); ap.add_argument("--nr", type=int, default=8); ap.add_argument("--nl", type=int, default=100)
    ap.add_argument("--order", type=int, default=1)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--newton", type=int, default=1, help="1: also time the parts of one coupled Newton iteration")
    ap.add_argument("--baseline-only", action="store_true", help="time tb_facet_assemble(TB_BC_PRESSURE) alone")
    args = ap.parse_args()
    import thunderbolt_jl_amd as tb
    L = tb._lib
    dev = tb.MI355XDevice(0)
    g = tb.generate_ideal_lv_mesh_hex(args.nc, args.nr, args.nl)
    f, s, n = tb.ideal_lv_microstructure(g)
    dh = tb.DofHandler(g, tb.LagrangeCollection(args.order) ** 3)
    sp = tb.allocate_matrix(dh)
    cm = tb.PK1Model(tb.Guccione1991PassiveModel(), tb.OrthotropicMicrostructureModel(f, s, n))
    op = tb.setup_operator(tb.ElementAssemblyStrategy(dev), tb.QuasiStaticModel("d", cm), dh, sp)
    facets = np.ascontiguousarray(g.facetset("Endocardium"), dtype=np.int32)
    rng = np.random.default_rng(0)
    u = dev.to_device(rng.uniform(-1e-3, 1e-3, dh.ndofs))
    res, col, row, vol = dev.zeros(dh.ndofs), dev.zeros(dh.ndofs), dev.zeros(dh.ndofs), dev.zeros(1)
    p = 0.7
    dev.defer_status(True)                                    # time the launches, not the status read-back after each call
    h = C.c_void_p()
    L.check(tb.lib().tb_facet_form_create(op.dmesh.h, L.TB_BC_PRESSURE, p, 0, facets.ctypes.data_as(L.c_i32p), len(facets), 0, C.byref(h)))
    t_base = median_ms(dev, lambda: L.check(tb.lib().tb_facet_assemble(h, op.pattern.h, u.ptr, 0.0, op.J.ptr, res.ptr)), args.reps)
    if args.baseline_only:
        dev.poll_status()
        print(json.dumps({"mesh": "ideal LV hex (%d, %d, %d), Q%d" % (args.nc, args.nr, args.nl, args.order), "ndofs": int(dh.ndofs), "facets": int(len(facets)),
                          "facet_pressure_ms": t_base}))
        return
    form = tb.ChamberForm(op.dmesh, facets, tb.RSAFDQ2022SurrogateVolume())
    t_new = median_ms(dev, lambda: form.assemble(u, p, pattern=op.pattern, nzval=op.J, r=res, col=col, row=row, volume=vol), args.reps)
    t_vol = median_ms(dev, lambda: form.assemble(u, p, volume=vol), args.reps)
    dev.poll_status()
    dev.defer_status(False)
    tb.lib().tb_form_destroy(h)
    out = {"mesh": "ideal LV hex (%d, %d, %d), Q%d" % (args.nc, args.nr, args.nl, args.order), "ndofs": int(dh.ndofs), "facets": int(len(facets)),
           "facet_pressure_ms": t_base, "chamber_all_outputs_ms": t_new, "chamber_volume_only_ms": t_vol, "ratio": t_new / t_base}
    if args.newton:
        # one coupled Newton iteration at a small load: base clamped, the chamber held 1 % below its reference volume
        base_nodes = np.unique(g.conn[g.facetset("Base")[:, 0]][:, list(g.HEX_FACETS[5])])
        nd0 = np.empty(g.n_nodes, dtype=np.int64)
        nd0[g.conn.ravel()] = dh.cell_dofs[:, : 3 * 8: 3].ravel()
        ch = tb.ConstraintHandler(dh, (nd0[base_nodes][:, None] + np.arange(3)).ravel())
        V0 = tb.compute_chamber_volume(dh, dev.zeros(dh.ndofs), "Endocardium", tb.RSAFDQ2022SurrogateVolume())
        system = tb.BlockedChamberSystem(op, ch, [tb.ChamberTying(form, None, "Endocardium", 0.99 * V0)])
        uu = dev.zeros(dh.ndofs)
        ev = [dev.event() for _ in range(3)]
        tb.update_linearization(op, uu, 0.0, residual=res)    # pre-roll: the first linearisation allocates its work arrays
        dev.synchronize()
        ev[0].record(); tb.update_linearization(op, uu, 0.0, residual=res); ev[1].record()
        system.vols.fill_zero(); system.cols[0].fill_zero(); system.rows[0].fill_zero()
        form.assemble(uu, 0.0, pattern=op.pattern, nzval=op.J, r=res, col=system.cols[0], row=system.rows[0], volume=system.vols.view(0, 1)); ev[2].record()
        dev.synchronize()
        t_lin, t_ch = ev[0].elapsed_ms(ev[1]), ev[1].elapsed_ms(ev[2])
        # the iteration as nlsolve runs it, on the wall clock: linearise (both passes, the eliminations, the volume read back), solve, apply
        ls = tb.SchurComplementLinearSolver("gmres", rtol=1e-8, maxiter=20000, gmres_restart=100)
        solver = tb.NewtonRaphsonSolver(inner_solver=ls, inner_rtol=1e-8, inner_maxiter=20000, gmres_restart=100)
        du = dev.zeros(dh.ndofs)
        dev.synchronize()
        t0 = time.perf_counter()
        system.linearize(uu, res, 0.0, True)
        rnorm = system.residual_norm(res)
        t1 = time.perf_counter()
        its, lres, ok = system.solve_increment(solver, res, du, solver.inner_rtol)
        dev.synchronize()
        t2 = time.perf_counter()
        if ok:
            system.apply_increment(uu, du)
        dev.synchronize()
        t3 = time.perf_counter()
        wall, t_solve = (t3 - t0) * 1e3, (t2 - t1) * 1e3
        out["newton_iteration"] = {"volume_pass_ms": t_lin, "chamber_pass_ms": t_ch, "inner_solves_ms": t_solve, "inner_iterations": ls.inner_iters, "schur_ok": bool(ok),
                                   "linearize_wall_ms": (t1 - t0) * 1e3, "apply_increment_ms": (t3 - t2) * 1e3, "iteration_wall_ms": wall,
                                   "host_and_small_kernels_ms": wall - t_lin - t_ch - t_solve, "residual_norm": rnorm, "dp": float(system.dp[0]) if ok else None}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
