#!/usr/bin/env python3
"""Elastodynamics on one MI355X: a Guccione bar (1 × 0.2 × 0.2, clamped at x = 0) released with a transverse velocity that grows along its axis —
the bar of the reference's test/integration/test_elastodynamics.jl — integrated by fixed-step Newmark-β (average acceleration by default: γ = 1/2,
β = 1/4; --gamma above 1/2 adds numerical dissipation).  Prints the tip deflection over time and one JSON summary line.  Toy size by default."""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("--cells", type=int, nargs=3, default=(4, 1, 1))
ap.add_argument("--order", type=int, default=1, choices=[1, 2])
ap.add_argument("--cell", default="hex", choices=["hex", "tet"])
ap.add_argument("--rho", type=float, default=1.0e-2)
ap.add_argument("--amplitude", type=float, default=0.2)
ap.add_argument("--dt", type=float, default=2.5e-2)
ap.add_argument("--tend", type=float, default=1.0)
ap.add_argument("--gamma", type=float, default=0.5)
args = ap.parse_args()
import thunderbolt_jl_amd as tb
dev = tb.MI355XDevice(0)
g = tb.generate_mesh(tb.Tetrahedron if args.cell == "tet" else tb.Hexahedron, tuple(args.cells), (0.0, 0.0, 0.0), (1.0, 0.2, 0.2))
dh = tb.DofHandler(g, tb.LagrangeCollection(args.order) ** 3)
sp = tb.allocate_matrix(dh)
ms = tb.ConstantCoefficient(tb.OrthotropicMicrostructure([1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0]))
model = tb.ElastodynamicsModel("d", "v", tb.PK1Model(tb.Guccione1991PassiveModel(), ms), tb.ConstantCoefficient(args.rho))
X = tb.dof_coordinates(dh)
left = np.flatnonzero(X[:, 0] < 1e-12)
ydofs = np.unique(dh.cell_dofs[:, 1::3])
v0 = np.zeros(dh.ndofs)
v0[ydofs] = args.amplitude * X[ydofs, 0]          # transverse velocity, fastest at the free end
v0[left] = 0.0
gamma = args.gamma
solver = tb.NewmarkSolver(beta=(gamma + 0.5) ** 2 / 4, gamma=gamma)
integrator = tb.NewmarkIntegrator(model, dh, sp, [tb.Dirichlet("d", left)], tb.ElementAssemblyStrategy(dev), None, v0, (0.0, args.tend), args.dt, solver=solver)
tip = [d for d in ydofs if abs(X[d, 0] - 1.0) < 1e-12 and abs(X[d, 1] - 0.2) < 1e-12 and abs(X[d, 2] - 0.2) < 1e-12][0]
print("   t      tip deflection (y)   tip velocity   Newton iterations")
t0 = time.perf_counter()
ok, newton_its, peak = True, 0, 0.0
while ok and integrator.t < args.tend - 1e-12:
    ok = integrator.step(min(args.dt, args.tend - integrator.t))
    newton_its += integrator.solver.inner_solver.iter
    uy, vy = integrator.u.to_host()[tip], integrator.velocity().to_host()[tip]
    peak = max(peak, abs(uy))
    print("%7.4f  %+.6e       %+.6e   %d" % (integrator.t, uy, vy, integrator.solver.inner_solver.iter))
dev.synchronize()
print(json.dumps({"workload": "elastodynamics bar, %s order %d, %dx%dx%d, %d dofs, Newmark beta %.4g gamma %.4g, dt %g" % ((args.cell, args.order) + tuple(args.cells) + (dh.ndofs, solver.beta, solver.gamma, args.dt)),
                  "converged": bool(ok), "steps": integrator.nsteps, "newton_iterations": int(newton_its), "peak_tip_deflection": float(peak), "solve_s": time.perf_counter() - t0}))
sys.exit(0 if ok else 1)
