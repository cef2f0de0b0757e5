#!/usr/bin/env python3
"""Geometric multigrid as the preconditioner of a Newton solve on one MI355X — the multigrid how-to of the reference
(docs/src/literate-howto/multigrid.jl) at toy size on first-order elements: a ring of 16 × 1 × 1 hexahedra refined once (GridHierarchy), a Guccione
wall on a Robin bed at the epicardium, its bottom clamped and its base lifted; Newton–Raphson whose linear solves are CG preconditioned by one
V(2, 2) cycle (GMGPrecon: Galerkin coarse operators rebuilt from every Jacobian).  Prints the Newton history beside the same solve with the
Chebyshev polynomial preconditioner, and one JSON summary line."""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("--cells", type=int, nargs=3, default=(16, 1, 1), help="circumferential, radial, longitudinal cells of the coarse ring")
ap.add_argument("--refinements", type=int, default=1)
ap.add_argument("--lift", type=float, default=0.005, help="prescribed axial displacement of the base")
args = ap.parse_args()
import thunderbolt_jl_amd as tb
dev = tb.MI355XDevice(0)
gh = tb.GridHierarchy(tb.generate_ring_mesh(*args.cells), args.refinements)
g = gh.grids[-1]                                                     # the sets of the coarse ring were transferred to it
dh = tb.DofHandler(g, tb.LagrangeCollection(1) ** 3)
sp = tb.allocate_matrix(dh)
node_dof0 = np.empty(g.n_nodes, dtype=np.int64)
node_dof0[g.conn.ravel()] = dh.cell_dofs[:, 0::3].ravel()


def facet_nodes(name):
    fs = g.facetset(name)
    return np.unique(g.conn[fs[:, 0][:, None], np.asarray(tb.Grid.HEX_FACETS)[fs[:, 1]]])


bottom, base = facet_nodes("Myocardium"), facet_nodes("Base")
pres = {int(d): 0.0 for d in (node_dof0[bottom][:, None] + np.arange(3)).ravel()}
pres.update({int(d): 0.0 for d in (node_dof0[base][:, None] + np.arange(2)).ravel()})
pres.update({int(d): np.sign(g.xyz[base[0], 2]) * args.lift for d in node_dof0[base] + 2})
dofs = np.array(sorted(pres))
ms = tb.ConstantCoefficient(tb.OrthotropicMicrostructure([1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0]))
model = tb.QuasiStaticModel("d", tb.PK1Model(tb.Guccione1991PassiveModel(), ms), [tb.RobinBC(0.1, "Epicardium")])
history = {}
t0 = time.perf_counter()
for name, precond in (("multigrid", tb.GMGPrecon(gh)), ("chebyshev(8)", tb.ChebyshevPrecBuilder(8))):
    ch = tb.ConstraintHandler(dh, dofs, np.array([pres[d] for d in dofs]))
    op = tb.setup_operator(tb.ElementAssemblyStrategy(dev), model, dh, sp)
    u = dev.zeros(dh.ndofs)
    tb.apply(u, ch)
    solver = tb.NewtonRaphsonSolver(max_iter=20, tol=1e-9, inner_rtol=1e-8, inner_solver="cg", inner_precond=precond)
    ok = tb.nlsolve(u, op, ch, solver)
    history[name] = {"converged": bool(ok), "newton_iterations": int(solver.iter), "linear_iterations": [int(k) for k in solver.linear_iters],
                     "residual_norms": [float(r) for r in solver.residual_norms], "max_displacement": float(np.abs(u.to_host()).max())}
    print("%-13s Newton %2d iterations, linear iterations %s, final residual %.2e" % (name, solver.iter, solver.linear_iters, solver.residual_norms[-1]))
dev.synchronize()
ok = all(h["converged"] for h in history.values())
print(json.dumps({"workload": "Guccione ring %dx%dx%d refined %d times, %d dofs, Newton with multigrid-preconditioned CG" % (tuple(args.cells) + (args.refinements, dh.ndofs)),
                  "levels": len(gh.grids), "converged": ok, "solve_s": time.perf_counter() - t0, **{k.split("(")[0]: v for k, v in history.items()}}))
sys.exit(0 if ok else 1)
