#!/usr/bin/env python3
"""Multigrid-preconditioned GMRES under a follower load on one MI355X, at toy size: a beam of first-order hexahedra (16 × 4 × 4 cells on 4 × 1 × 1 over a
4 × 1 × 1-cell coarse grid), a Holzapfel–Ogden material, the left face clamped, a pressure on the bottom face (PressureFieldBC).  The follower load
makes the tangent non-symmetric, so CG is not the method; the reference pairs KrylovJL_GMRES with GMGPrecon for it (src/solver/linear/multigrid.jl:
101-159).  Newton–Raphson twice: with Jacobi-GMRES and with GMRES whose right preconditioner is one V(2, 2) cycle of the geometric multigrid in general
mode (pivoted, unsymmetrised coarsest inverse).  Prints both Newton histories with their Arnoldi step counts and one JSON summary line.
The multigrid is for MILDLY non-symmetric tangents with a positive diagonal: the point-Jacobi Chebyshev smoother breaks down when the skew part is as
large as the symmetric one."""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("--refinements", type=int, default=2, help="uniform refinements of the 4 x 1 x 1-cell coarse grid")
ap.add_argument("--pressure", type=float, default=0.001)
ap.add_argument("--restart", type=int, default=100)
args = ap.parse_args()
import thunderbolt_jl_amd as tb
dev = tb.MI355XDevice(0)
gh = tb.GridHierarchy(tb.generate_mesh(tb.Hexahedron, (4, 1, 1), (0, 0, 0), (4.0, 1.0, 1.0)), args.refinements)
dh = tb.DofHandler(gh.grids[-1], tb.LagrangeCollection(1) ** 3)
sp = tb.allocate_matrix(dh)
clamped = np.flatnonzero(np.abs(tb.dof_coordinates(dh)[:, 0]) < 1e-12)
model = tb.QuasiStaticModel("d", tb.PK1Model(tb.HolzapfelOgden2009Model(a=1.0, b=1.0, af=0.0, as_=0.0, afs=0.0, beta=1.0), tb.ConstantCoefficient(tb.OrthotropicMicrostructure(*np.eye(3)))),
                            [tb.PressureFieldBC(tb.ConstantCoefficient(args.pressure), "bottom")])
history, fields = {}, {}
t0 = time.perf_counter()
for name, precond in (("jacobi", None), ("multigrid", tb.GMGPrecon(gh))):
    ch = tb.ConstraintHandler(dh, clamped)
    op = tb.setup_operator(tb.ElementAssemblyStrategy(dev), model, dh, sp)
    u = dev.zeros(dh.ndofs)
    solver = tb.NewtonRaphsonSolver(max_iter=20, tol=1e-9, inner_rtol=1e-8, inner_solver="gmres", inner_precond=precond, inner_maxiter=20000,
                                    gmres_restart=args.restart, strict_inner_solve=False)
    ok = tb.nlsolve(u, op, ch, solver)
    fields[name] = u.to_host()
    history[name] = {"converged": bool(ok), "newton_iterations": int(solver.iter), "arnoldi_steps": [int(k) for k in solver.linear_iters],
                     "arnoldi_steps_total": int(sum(solver.linear_iters)), "max_displacement": float(np.abs(fields[name]).max())}
    print("%-9s GMRES(%d): Newton %2d iterations, Arnoldi steps %s = %d" % (name, args.restart, solver.iter, list(solver.linear_iters), sum(solver.linear_iters)))
dev.synchronize()
ok = all(h["converged"] for h in history.values())
diff = float(np.abs(fields["jacobi"] - fields["multigrid"]).max() / np.abs(fields["jacobi"]).max())
print(json.dumps({"workload": "Holzapfel-Ogden Q1 beam under a follower pressure, %d cells, %d dofs, %d multigrid levels, Newton with GMRES(%d): Jacobi against multigrid"
                  % (gh.grids[-1].n_cells, dh.ndofs, len(gh.grids), args.restart), "converged": ok, "max_relative_difference": diff,
                  "solve_s": time.perf_counter() - t0, **history}))
sys.exit(0 if ok else 1)
