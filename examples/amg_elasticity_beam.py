#!/usr/bin/env python3
"""Rigid-body modes in the algebraic multigrid on one MI355X, at toy size: a slender bar of first-order hexahedra (16 × 2 × 2 cells on 8 × 1 × 1), a
Holzapfel–Ogden material, the left face clamped, the right face pushed sideways.  Newton–Raphson whose linear solves are CG preconditioned by one
V(2, 2) cycle of the smoothed-aggregation multigrid — once with AMGPrecon(), whose prolongator carries the three translations, once with
AMGPrecon(near_nullspace="rigid_body"), which aggregates node by node and carries the three rotations as well.  Bending is what the translations miss:
the linear iteration counts show it.  Prints both Newton histories, the levels of both hierarchies and one JSON summary line."""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("--cells", type=int, nargs=3, default=(16, 2, 2), help="cells along x, y, z")
ap.add_argument("--length", type=float, default=8.0)
ap.add_argument("--push", type=float, default=0.1, help="prescribed sideways displacement of the free end")
ap.add_argument("--max-coarse", type=int, default=32)
args = ap.parse_args()
import thunderbolt_jl_amd as tb
dev = tb.MI355XDevice(0)
dh = tb.DofHandler(tb.generate_mesh(tb.Hexahedron, tuple(args.cells), (0, 0, 0), (args.length, 1.0, 1.0)), tb.LagrangeCollection(1) ** 3)
sp = tb.allocate_matrix(dh)
x, comp = tb.dof_coordinates(dh)[:, 0], tb.amg.component_labels(dh)
pres = {int(d): 0.0 for d in np.flatnonzero(np.abs(x) < 1e-12)}
pres.update({int(d): args.push for d in np.flatnonzero((np.abs(x - args.length) < 1e-12) & (comp == 2))})
dofs = np.array(sorted(pres))
model = tb.QuasiStaticModel("d", tb.PK1Model(tb.HolzapfelOgden2009Model(), tb.ConstantCoefficient(tb.OrthotropicMicrostructure(*np.eye(3)))))
history, fields = {}, {}
t0 = time.perf_counter()
for name, precond in (("translations", tb.AMGPrecon(max_coarse=args.max_coarse)), ("rigid_body", tb.AMGPrecon(max_coarse=args.max_coarse, near_nullspace="rigid_body"))):
    ch = tb.ConstraintHandler(dh, dofs, np.array([pres[d] for d in dofs]))
    op = tb.setup_operator(tb.ElementAssemblyStrategy(dev), model, dh, sp)
    u = dev.zeros(dh.ndofs)
    tb.apply(u, ch)
    solver = tb.NewtonRaphsonSolver(max_iter=20, tol=1e-9, inner_rtol=1e-8, inner_solver="cg", inner_precond=precond, inner_maxiter=2000)
    ok = tb.nlsolve(u, op, ch, solver)
    mg = precond.materialize(op.pattern, ch)
    sizes = [mg.level_size(l) for l in range(mg.n_levels)]
    fields[name] = u.to_host()
    history[name] = {"converged": bool(ok), "newton_iterations": int(solver.iter), "linear_iterations": [int(k) for k in solver.linear_iters],
                     "levels": [int(s[0]) for s in sizes], "operator_complexity": sum(s[1] for s in sizes) / sizes[0][1],
                     "dead_coarse_dofs": [int(mg.dead(l).sum()) for l in range(mg.n_levels - 1)] if name == "rigid_body" else None}
    print("%-13s Newton %2d iterations, linear iterations %s, levels %s, operator complexity %.2f" % (
        name, solver.iter, solver.linear_iters, history[name]["levels"], history[name]["operator_complexity"]))
dev.synchronize()
ok = all(h["converged"] for h in history.values())
diff = float(np.abs(fields["translations"] - fields["rigid_body"]).max() / np.abs(fields["translations"]).max())
print(json.dumps({"workload": "Holzapfel-Ogden Q1 bar %dx%dx%d, %d dofs, Newton with AMG-preconditioned CG, translations against rigid-body modes" % (tuple(args.cells) + (dh.ndofs,)),
                  "converged": ok, "max_relative_difference": diff, "solve_s": time.perf_counter() - t0, **history}))
sys.exit(0 if ok else 1)
