#!/usr/bin/env python3
"""p-multigrid as the preconditioner of a Newton solve on one MI355X — second-order hexahedra, the element the reference recommends for mechanics
(LagrangeCollection{2}()^3), at toy size: a bar of 4 × 1 × 1 hexahedra refined once (GridHierarchy), a Holzapfel–Ogden material, the left face
clamped, the right face pulled along the bar.  Newton–Raphson whose linear solves are CG preconditioned by one V(2, 2) cycle of
ChainedMGPrecon(PMGPrecon(), GMGPrecon(gh)): the Q2 tangent on top, the Q1 field on the same grid below it (the p-level), the Q1 field on the
coarse grid at the bottom (the h-level); Galerkin coarse operators rebuilt from every Jacobian.  Prints the Newton history beside the same solve
with the Chebyshev polynomial preconditioner, and one JSON summary line."""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("--cells", type=int, nargs=3, default=(4, 1, 1), help="cells of the coarse bar along x, y, z")
ap.add_argument("--refinements", type=int, default=1)
ap.add_argument("--pull", type=float, default=0.004, help="prescribed axial displacement of the free end")
args = ap.parse_args()
import thunderbolt_jl_amd as tb
dev = tb.MI355XDevice(0)
length = float(args.cells[0])
gh = tb.GridHierarchy(tb.generate_mesh(tb.Hexahedron, tuple(args.cells), (0, 0, 0), (length, float(args.cells[1]), float(args.cells[2]))), args.refinements)
dh = tb.DofHandler(gh.grids[-1], tb.LagrangeCollection(2) ** 3)
sp = tb.allocate_matrix(dh)
x = tb.dof_coordinates(dh)[:, 0]
comp = np.empty(dh.ndofs, dtype=np.int64)
for k in range(3):
    comp[dh.cell_dofs[:, k::3].ravel()] = k
pres = {int(d): 0.0 for d in np.flatnonzero(np.abs(x) < 1e-12)}
pres.update({int(d): args.pull for d in np.flatnonzero((np.abs(x - length) < 1e-12) & (comp == 0))})
dofs = np.array(sorted(pres))
f, s, n = np.array([1, 1, 0.0]) / np.sqrt(2), np.array([-1, 1, 0.0]) / np.sqrt(2), np.array([0, 0, 1.0])
model = tb.QuasiStaticModel("d", tb.PK1Model(tb.HolzapfelOgden2009Model(), tb.ConstantCoefficient(tb.OrthotropicMicrostructure(f, s, n))))
history, plan = {}, None
t0 = time.perf_counter()
for name, precond in (("multigrid", tb.ChainedMGPrecon(tb.PMGPrecon(), tb.GMGPrecon(gh))), ("chebyshev(8)", tb.ChebyshevPrecBuilder(8))):
    ch = tb.ConstraintHandler(dh, dofs, np.array([pres[d] for d in dofs]))
    op = tb.setup_operator(tb.ElementAssemblyStrategy(dev), model, dh, sp)
    u = dev.zeros(dh.ndofs)
    tb.apply(u, ch)
    solver = tb.NewtonRaphsonSolver(max_iter=20, tol=1e-9, inner_rtol=1e-8, inner_solver="cg", inner_precond=precond)
    ok = tb.nlsolve(u, op, ch, solver)
    history[name] = {"converged": bool(ok), "newton_iterations": int(solver.iter), "linear_iterations": [int(k) for k in solver.linear_iters],
                     "residual_norms": [float(r) for r in solver.residual_norms], "max_displacement": float(np.abs(u.to_host()).max())}
    print("%-13s Newton %2d iterations, linear iterations %s, final residual %.2e" % (name, solver.iter, solver.linear_iters, solver.residual_norms[-1]))
    if name == "multigrid":
        mg = precond.materialize(op.pattern, ch)
        blocked, terms = mg.plan(mg.n_levels - 1)
        plan = {"levels": mg.n_levels, "p_level_blocked": blocked, "p_level_terms": terms, "p_level_plan_bytes": mg.plan_bytes(mg.n_levels - 1)}
dev.synchronize()
ok = all(h["converged"] for h in history.values())
print(json.dumps({"workload": "Holzapfel-Ogden Q2 bar %dx%dx%d refined %d times, %d dofs, Newton with p-multigrid-preconditioned CG" % (tuple(args.cells) + (args.refinements, dh.ndofs)),
                  **plan, "converged": ok, "solve_s": time.perf_counter() - t0, **{k.split("(")[0]: v for k, v in history.items()}}))
sys.exit(0 if ok else 1)
