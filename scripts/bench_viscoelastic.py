#!/usr/bin/env python3
"""tb_linearize (K + r) of the viscoelastic form (LinearMaxwellMaterial, k_viscoelastic) per strategy, beside the Holzapfel–Ogden fast path on the
same mesh and pattern, in one process — one JSON line per (mesh, strategy): both times, their ratio, the bytes per cell the viscoelastic kernel must
move (its Kₑ, the state read and written, u) and the fraction of the HBM rate they imply at the measured time.
Meshes: 40³ Q1 and 24³ Q2 hexahedra (the sizes of bench_mechanics.py) and the 24³ lattice cut into tetrahedra for P1 / P2.
Pre-roll, `--passes` passes of `--steps` assemblies each, min and median over the passes (event times)."""
import argparse, json, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--n1", type=int, default=40, help="Q1 lattice")
ap.add_argument("--n2", type=int, default=24, help="Q2 / P1 / P2 lattice")
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--passes", type=int, default=5)
ap.add_argument("--only", default="", help="comma-separated subset of Q1,Q2,P1,P2")
ap.add_argument("--hbm-tbps", type=float, default=8.0, help="peak HBM bandwidth of the box (MI355X: 8 TB/s)")
args = ap.parse_args()
import thunderbolt_jl_amd as tb
from _preroll import preroll
dev = tb.MI355XDevice(0)
ms = tb.ConstantCoefficient(tb.OrthotropicMicrostructure([1, 0, 0], [0, 1, 0], [0, 0, 1]))
MODELS = (("viscoelastic", tb.QuasiStaticModel("d", tb.LinearMaxwellMaterial())), ("holzapfel-ogden", tb.QuasiStaticModel("d", tb.PK1Model(tb.HolzapfelOgden2009Model(), ms))))
STRATEGIES = (("element", tb.ElementAssemblyStrategy), ("patch", tb.PatchAssemblyStrategy), ("color", tb.PerColorAssemblyStrategy), ("atomic", tb.AtomicAssemblyStrategy))


def timed(run):
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
    return float(np.min(times)), float(np.median(times))


def measure(label, cell, order, n, nq):
    g = tb.generate_mesh(cell, (n, n, n), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    dh = tb.DofHandler(g, tb.LagrangeCollection(order) ** 3)
    sp = tb.allocate_matrix(dh)
    u = dev.to_device(1e-2 * np.sin(np.pi * np.arange(dh.ndofs) / dh.ndofs))
    res = dev.zeros(dh.ndofs)
    nd = dh.ndofs_per_cell
    # what the viscoelastic kernel must move per cell: its element matrix (written), the state (six per point, read and written) and u (read)
    cell_bytes = 8 * (nd * nd + 2 * 6 * nq + nd)
    for sname, S in STRATEGIES:
        row = {"mesh": "%s, %d^3 lattice (%d cells, %d dofs, nnz %d)" % (label, n, g.n_cells, dh.ndofs, sp.nnz), "strategy": sname}
        for mname, model in MODELS:
            op = tb.setup_operator(S(dev), model, dh, sp)
            if op.internal is not None:
                tb.set_timestep(op, 0.1)
            tmin, tmed = timed(lambda: tb.update_linearization(op, u, 0.0, residual=res))
            # (the hexahedral hyperelastic launchers do not name their kernels through tb_last_kernel_name)
            kname = tb.lib().tb_last_kernel_name().decode() if mname == "viscoelastic" or cell == tb.Tetrahedron else "k_hyperelastic / k_mech_points + k_mech_contract"
            row[mname + "_ms_min"], row[mname + "_ms_median"], row[mname + "_kernel"] = tmin, tmed, kname
        row["ratio_viscoelastic_over_holzapfel_ogden"] = row["viscoelastic_ms_min"] / row["holzapfel-ogden_ms_min"]
        row["viscoelastic_bytes_per_cell"] = cell_bytes
        row["viscoelastic_hbm_fraction"] = cell_bytes * g.n_cells / (row["viscoelastic_ms_min"] * 1e-3) / (args.hbm_tbps * 1e12)
        print(json.dumps(row), flush=True)


only = set(x for x in args.only.split(",") if x)
for key, spec in (("Q1", ("Q1 hexahedra", tb.Hexahedron, 1, args.n1, 8)), ("Q2", ("Q2 hexahedra", tb.Hexahedron, 2, args.n2, 27)),
                  ("P1", ("P1 tetrahedra", tb.Tetrahedron, 1, args.n2, 4)), ("P2", ("P2 tetrahedra", tb.Tetrahedron, 2, args.n2, 8))):
    if not only or key in only:
        measure(*spec)
