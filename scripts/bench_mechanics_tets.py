#!/usr/bin/env python3
"""K + r assembly of the quasi-static mechanics operator on tetrahedra (P1 and P2 displacement) — one JSON line per configuration:
the 6·n³ Kuhn split of an n³ lattice, every strategy code, kernel name, element integrations per second, algorithmic bytes and their share of the
HBM roofline; and, on the same lattice, the Q2-hexahedron figure (the P2 tetrahedral field has the same dofs: lattice vertices + edge / face /
cell centres are exactly the P2 nodes of the split), to be read side by side at equal dof count.
Pre-roll, `--passes` passes of `--steps` assemblies each, min and median over the passes (event times)."""
import argparse, json, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=24)
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--passes", type=int, default=5)
ap.add_argument("--energy", default="ho", choices=["ho", "guccione"])
ap.add_argument("--hbm-tbps", type=float, default=8.0, help="peak HBM bandwidth of the box (MI355X: 8 TB/s)")
args = ap.parse_args()
import thunderbolt_jl_amd as tb
from _preroll import preroll
dev = tb.MI355XDevice(0)
n = args.n
ms = tb.ConstantCoefficient(tb.OrthotropicMicrostructure([1, 0, 0], [0, 1, 0], [0, 0, 1]))
energy = tb.HolzapfelOgden2009Model() if args.energy == "ho" else tb.Guccione1991PassiveModel()
model = tb.QuasiStaticModel("u", tb.PK1Model(energy, ms))
STRATEGIES = (("patch (default)", tb.PatchAssemblyStrategy), ("atomic", tb.AtomicAssemblyStrategy), ("color", tb.PerColorAssemblyStrategy), ("element", tb.ElementAssemblyStrategy))


def measure(label, cell, order, strategies):
    g = tb.generate_mesh(cell, (n, n, n), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    dh = tb.DofHandler(g, tb.LagrangeCollection(order) ** 3)
    sp = tb.allocate_matrix(dh)
    u = dev.to_device(1e-2 * np.sin(np.pi * np.arange(dh.ndofs) / dh.ndofs))
    res = dev.zeros(dh.ndofs)
    # bytes an assembly cannot avoid: nz written once, r written once, u read once, and per cell its dof table, connectivity, vertex coordinates
    # and block positions (2 B per node pair)
    nb = dh.ndofs_per_cell // 3
    nbytes = 8 * sp.nnz + 16 * dh.ndofs + g.n_cells * (4 * dh.ndofs_per_cell + 4 * g.conn.shape[1] + 24 * g.conn.shape[1] + 2 * nb * nb)
    fastest = None
    rows = []
    for sname, S in strategies:
        op = tb.setup_operator(S(dev), model, dh, sp)
        run = lambda: tb.update_linearization(op, u, 0.0, residual=res)
        run()
        preroll(dev, run)
        times = []
        for _ in range(args.passes):
            e0, e1 = dev.event(), dev.event()
            e0.record()
            for _ in range(args.steps):
                run()
            e1.record(); dev.synchronize()
            times.append(e0.elapsed_ms(e1) / args.steps)
        tmin, tmed = float(np.min(times)), float(np.median(times))
        rows.append({"workload": "%s, %s quasi-static K + r, %s, %d^3 lattice (%d cells, %d dofs, nnz %d)" % (label, args.energy, sname, n, g.n_cells, dh.ndofs, sp.nnz),
                     "strategy": sname, "kernel": tb.lib().tb_last_kernel_name().decode() if cell == tb.Tetrahedron else "k_mech_points + k_mech_contract + k_gather_node_rows_lds", "linearize_ms_min": tmin, "linearize_ms_median": tmed,
                     "element_integrations_per_s": g.n_cells / (tmin * 1e-3), "dofs": dh.ndofs, "algorithmic_bytes": int(nbytes),
                     "hbm_roofline_fraction": nbytes / (tmin * 1e-3) / (args.hbm_tbps * 1e12)})
        fastest = tmin if fastest is None else min(fastest, tmin)
    for r in rows:
        r["slowdown_vs_fastest_strategy"] = r["linearize_ms_min"] / fastest
        print(json.dumps(r), flush=True)


measure("P1 tetrahedra", tb.Tetrahedron, 1, STRATEGIES)
measure("P2 tetrahedra", tb.Tetrahedron, 2, STRATEGIES)
measure("Q2 hexahedra (same lattice, same dofs as P2 tetrahedra)", tb.Hexahedron, 2, (("element (default)", tb.ElementAssemblyStrategy),))
