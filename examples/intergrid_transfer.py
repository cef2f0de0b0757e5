#!/usr/bin/env python3
"""Two meshes, one field: monodomain + FitzHugh–Nagumo on a fine hexahedral box (a few steps of LieTrotterGodunov((BackwardEuler(CG),
ForwardEulerCellSolver()))), then φₘ moved to a coarse tetrahedral box of the same extent by NodalIntergridInterpolation / transfer
(src/ferrite-addons/transfer_operators.jl:20-161) — on the device: the electrophysiology mesh of an electromechanics run is several times
finer than its mechanics mesh, and the field crosses without a host trip.  Prints one JSON line."""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=64, help="fine mesh: n³ hexahedra")
ap.add_argument("--m", type=int, default=16, help="coarse mesh: 6·m³ tetrahedra")
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--dt", type=float, default=1.0)
ap.add_argument("--reps", type=int, default=20, help="transfers timed (after one untimed)")
args = ap.parse_args()
import thunderbolt_jl_amd as tb
dev = tb.MI355XDevice(0)
L = 2.5
fine = tb.generate_mesh(tb.Hexahedron, (args.n,) * 3, (0, 0, 0), (L, L, L))
coarse = tb.generate_mesh(tb.Tetrahedron, (args.m,) * 3, (0, 0, 0), (L, L, L))
dh_ep, dh_mech = tb.DofHandler(fine), tb.DofHandler(coarse)
sp = tb.allocate_matrix(dh_ep)
kap = np.diag([4.5e-5, 2.0e-5, 2.0e-5])                   # ep01_spiral-wave.jl:39-41
D = tb.ConductivityToDiffusivityCoefficient(tb.ConstantCoefficient(kap), tb.ConstantCoefficient(1.0), tb.ConstantCoefficient(1.0))
heat = tb.BackwardEulerStage(tb.BackwardEulerSolver(rtol=1e-5, atol=1e-6), tb.PatchAssemblyStrategy(dev), dh_ep, D, None, sp)
n = dh_ep.ndofs
X = tb.dof_coordinates(dh_ep)
u0 = np.zeros((2, n))
u0[0] = ((X[:, 0] <= L / 2) & (X[:, 1] <= L / 2)).astype(float)   # ep01:113-118
u0[1] = 0.1 * (X[:, 1] >= L / 2)
f = tb.PointwiseODEFunction(n, tb.FHNModel())
cache = tb.setup_solver_cache(f, tb.ForwardEulerCellSolver(dev), u=dev.to_device(np.ascontiguousarray(u0).ravel()), keep_du=False)
ltg = tb.LieTrotterGodunov(heat, f, cache)
for s in range(args.steps):
    assert ltg.step(s * args.dt, args.dt)
phi = cache.un.view(0, n)                                  # the φₘ block of the state-blocked solution
dev.synchronize()
t0 = time.perf_counter()
op = tb.NodalIntergridInterpolation(dev, dh_ep, dh_mech)   # locate the coarse nodes in the fine mesh: once per pair of meshes
dev.synchronize()
t_locate = time.perf_counter() - t0
phi_mech = dev.zeros(dh_mech.ndofs)
tb.transfer(phi_mech, op, phi)
dev.synchronize()
t0 = time.perf_counter()
for _ in range(args.reps):
    tb.transfer(phi_mech, op, phi)                         # what a coupled time step pays
dev.synchronize()
t_transfer = (time.perf_counter() - t0) / args.reps
src, out = phi.to_host(), phi_mech.to_host()
print(json.dumps({"workload": "FHN monodomain on %d^3 hexahedra (%d dofs), %d steps; phi_m -> %d tetrahedra (%d dofs)" % (args.n, n, args.steps, coarse.n_cells, dh_mech.ndofs),
                  "n_missing": op.n_missing, "source_range": [float(src.min()), float(src.max())],
                  "transferred_range": [float(np.nanmin(out)), float(np.nanmax(out))], "locate_ms": t_locate * 1e3, "transfer_ms": t_transfer * 1e3}))
