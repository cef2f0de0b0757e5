#!/usr/bin/env python3
"""Times point location (tb_locator_create: bins + search, and tb_locator_relocate: search alone) and the per-step evaluation (tb_locator_evaluate
with the scatter map, i.e. transfer) between box meshes: an n³ hexahedral source (Q1 field) to an (n/2)³ hexahedral and a 6·(3n/8)³ tetrahedral target,
and a Q2 source field to a Q1 target.  Beside each transfer, the host path examples/electromechanics_lv.py uses for the same field size — to_host, a
NumPy index, upload — and a device copy of the field as the rate yardstick.  HIP events for device work, perf_counter for the host path, every timed loop
behind an untimed pre-roll; the median of --reps.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from _preroll import preroll  # noqa: E402


def event_ms(dev, fn, reps):
    out = []
    for _ in range(reps):
        e0, e1 = dev.event(), dev.event()
        e0.record(); fn(); e1.record()
        dev.synchronize()
        out.append(e0.elapsed_ms(e1))
    return float(np.median(out))


def wall_ms(dev, fn, reps):
    out = []
    for _ in range(reps):
        dev.synchronize()
        t0 = time.perf_counter()
        fn()
        dev.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out))


def case(tb, dev, name, dh_from, dh_to, reps):
    L = tb._lib
    u = dev.to_device(np.random.default_rng(0).uniform(-1.0, 1.0, dh_from.ndofs))
    t0 = time.perf_counter()
    op = tb.NodalIntergridInterpolation(dev, dh_from, dh_to)
    dev.synchronize()
    create_ms = (time.perf_counter() - t0) * 1e3                              # host dof set + upload + bins + search
    npts, nb = op.ph.n_points, dh_from.ndofs_per_cell
    pts = dev.to_device(op.nodes.ravel())
    relocate = lambda: L.check(tb.lib().tb_locator_relocate(op.ph.h, npts, pts.ptr))
    u_to = dev.zeros(dh_to.ndofs)
    xfer = lambda: tb.transfer(u_to, op, u)
    preroll(dev, xfer)
    locate_ms = wall_ms(dev, relocate, max(reps // 4, 3))                     # includes its one read-back
    evaluate_ms = event_ms(dev, xfer, reps)
    # algorithmic bytes of the evaluation: (cell, ξ) 28 B, nb dof ids and nb field values, the scatter index and the stored value, per point
    ev_bytes = npts * (28 + nb * 4 + nb * 8 + 4 + 8)
    # the host path of examples/electromechanics_lv.py:80-83 at this field size: download, index, upload
    idx = np.random.default_rng(1).integers(0, dh_from.ndofs, dh_to.ndofs)

    def host_path():
        u_to.copy_from_host(u.to_host()[idx])

    host_ms = wall_ms(dev, host_path, max(reps // 4, 3))
    copy = dev.zeros(dh_from.ndofs)
    d2d = lambda: L.check(tb.lib().tb_memcpy_d2d(dev.h, copy.ptr, u.ptr, u.nbytes))
    preroll(dev, d2d, 50.0)
    copy_ms = event_ms(dev, d2d, reps)
    return {"case": name, "source_dofs": dh_from.ndofs, "points": npts, "n_missing": op.n_missing, "create_ms_incl_host_dof_set": create_ms,
            "locate_ms": locate_ms, "locate_ns_per_point": locate_ms * 1e6 / npts, "evaluate_ms": evaluate_ms, "evaluate_algorithmic_GBps": ev_bytes / evaluate_ms * 1e-6,
            "host_path_ms": host_ms, "device_copy_of_source_GBps": 2 * u.nbytes / copy_ms * 1e-6}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=128, help="source: n³ hexahedra")
    ap.add_argument("--q2-n", type=int, default=48, help="source of the Q2 case: n³ hexahedra (27 dofs per cell)")
    ap.add_argument("--reps", type=int, default=30)
    args = ap.parse_args()
    import thunderbolt_jl_amd as tb
    dev = tb.MI355XDevice(0)
    n = args.n
    box = ((0, 0, 0), (1, 1, 1))
    src = tb.DofHandler(tb.generate_mesh(tb.Hexahedron, (n,) * 3, *box))
    out = [case(tb, dev, "hex8 %d^3 -> hex8 %d^3" % (n, n // 2), src, tb.DofHandler(tb.generate_mesh(tb.Hexahedron, (n // 2,) * 3, *box)), args.reps),
           case(tb, dev, "hex8 %d^3 -> tet4 6x%d^3" % (n, 3 * n // 8), src, tb.DofHandler(tb.generate_mesh(tb.Tetrahedron, (3 * n // 8,) * 3, *box)), args.reps)]
    del src
    m = args.q2_n
    src2 = tb.DofHandler(tb.generate_mesh(tb.Hexahedron, (m,) * 3, *box), tb.LagrangeCollection(2))
    out.append(case(tb, dev, "hex27 %d^3 -> hex8 %d^3" % (m, m), src2, tb.DofHandler(tb.generate_mesh(tb.Hexahedron, (m,) * 3, *box)), args.reps))
    print(json.dumps({"device": dev.info()["name"], "cases": out}))


if __name__ == "__main__":
    main()
