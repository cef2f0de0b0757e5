#!/usr/bin/env python3
"""Quasi-static viscoelasticity on one MI355X: the creep test of the reference's "Viscoelasticity" test set (test/integration/test_solid_mechanics.jl:768-807).
A block of LinearMaxwellMaterial on [-1, 1]³ is clamped on its left face and its right face is moved by (0.1, 0, 0) and held: the strain is fixed, the
Maxwell branch relaxes, and the viscous strain εᵛ₁₁ creeps towards ε₁₁ = 0.05 with the time constant η₁(1+ν)/E₁ of its deviatoric part.

How the pieces fit: the material goes into a QuasiStaticModel like any other; the operator allocates the viscous strain (six values per quadrature
point) as `op.internal` / `op.internal_known`; perform_mechanics_step does one backward-Euler step — Newton on u (one iteration: the problem is
linear) with the local problem re-solved inside every assembly from the accepted state — and accepts the state; internal_variables(op) returns the
state on the host as [cell][q][6], components (11, 21, 31, 22, 32, 33).  Prints the εᵛ₁₁ history and one JSON summary line.  Toy size by default."""
import argparse, json, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("--cells", type=int, nargs=3, default=(2, 1, 1))
ap.add_argument("--order", type=int, default=1, choices=[1, 2])
ap.add_argument("--cell", default="hex", choices=["hex", "tet"])
ap.add_argument("--dt", type=float, default=0.1)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--eta1", type=float, default=1e3)
args = ap.parse_args()
import thunderbolt_jl_amd as tb
dev = tb.MI355XDevice(0)
g = tb.generate_mesh(tb.Tetrahedron if args.cell == "tet" else tb.Hexahedron, tuple(args.cells), (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
dh = tb.DofHandler(g, tb.LagrangeCollection(args.order) ** 3)
sp = tb.allocate_matrix(dh)
material = tb.LinearMaxwellMaterial(E0=70e3, E1=20e3, mu=1e3, eta1=args.eta1, nu=0.3)
op = tb.setup_operator(tb.ElementAssemblyStrategy(dev), tb.QuasiStaticModel("d", material, ()), dh, sp)
# Dirichlet conditions: left face clamped, right face at (0.1, 0, 0)
X = tb.dof_coordinates(dh)
xdofs = np.unique(dh.cell_dofs[:, 0::3])
left, right = np.flatnonzero(X[:, 0] < -1 + 1e-12), np.flatnonzero(X[:, 0] > 1 - 1e-12)
prescribed = np.unique(np.concatenate([left, right]))      # the handler keeps its dofs sorted; the values go with that order
target = np.zeros(dh.ndofs)
target[np.intersect1d(right, xdofs)] = 0.1
ch = tb.ConstraintHandler(dh, prescribed, target[prescribed])
solver = tb.NewtonRaphsonSolver(max_iter=10, tol=1e-8, inner_solver="cg", inner_rtol=1e-12)
u = dev.zeros(dh.ndofs)
tb.apply(u, ch)
print("solution size: %d displacement dofs + %d internal variables" % (dh.ndofs, tb.solution_size(op) - dh.ndofs))
print("   t      viscous strain 11 (first point)   mean over the points   Newton iterations")
hist, accepted, its = [tb.internal_variables(op)[0, 0, 0]], [], []
for k in range(args.steps):
    ok = tb.perform_mechanics_step(u, op, ch, solver, k * args.dt, args.dt)
    accepted.append(bool(ok))
    its.append(solver.iter)
    Q = tb.internal_variables(op)
    hist.append(float(Q[0, 0, 0]))
    print("%7.4f  %.15e             %.15e  %d" % ((k + 1) * args.dt, Q[0, 0, 0], Q[:, :, 0].mean(), solver.iter))
    if not ok:
        break
dev.synchronize()
print(json.dumps({"workload": "viscoelastic creep, %s order %d, %dx%dx%d, %d dofs, dt %g" % ((args.cell, args.order) + tuple(args.cells) + (dh.ndofs, args.dt)),
                  "all_accepted": all(accepted) and len(accepted) == args.steps, "newton_iterations_per_step": int(max(its)), "monotone": bool((np.diff(hist) >= 0).all()),
                  "viscous_strain_11": [float(h) for h in hist]}))
sys.exit(0 if all(accepted) else 1)
