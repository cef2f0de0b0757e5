#!/usr/bin/env python3
"""The reference's "Pacemaker subdomain" integration test as a how-to (test/integration/test_electrophysiology.jl:124-195) on one MI355X:
a square of quadrilaterals on [−2.5, 2.5]², the cells with ‖x‖∞ ≤ 0.75 a pacemaker region with its own FitzHugh–Nagumo parameters, the rest
myocardium with the defaults; insert_interfaces duplicates the nodes between the two, an InterfaceDiffusionModel with conductance G couples them
again; LieTrotterGodunov((BackwardEulerSolver(), ForwardEulerCellSolver())), Δt = 1, φ₀ = max(1 − ‖x‖, 0).  Prints one JSON line."""
import argparse, json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=64)
ap.add_argument("--tend", type=float, default=10.0)
ap.add_argument("--G", type=float, default=1.0)
args = ap.parse_args()
import thunderbolt_jl_amd as tb
dev = tb.MI355XDevice(0)
grid = tb.generate_mesh(tb.Quadrilateral, (args.n, args.n), (-2.5, -2.5), (2.5, 2.5))
pacemaker = grid.addcellset("Pacemaker", lambda x: np.abs(x).max() <= 0.75)
grid.addcellset("Myocardium", np.setdiff1d(np.arange(grid.n_cells), pacemaker))
grid2 = tb.insert_interfaces(grid, ["Pacemaker", "Myocardium"])       # one record per shared edge in grid2.interfaces
one, kappa = tb.ConstantCoefficient(1.0), tb.ConstantCoefficient(np.array([[4.5e-4, 0.0], [0.0, 2.0e-4]]))
models = {
    "Pacemaker": tb.MonodomainModel(one, one, kappa, tb.NoStimulationProtocol(), tb.FHNModel(a=-0.5, b=1.0, c=-0.6, d=0.0, e=0.001, f=50 * 0.001), "φₘ", "s1"),
    "Myocardium": tb.MonodomainModel(one, one, kappa, tb.NoStimulationProtocol(), tb.FHNModel(), "φₘ", "s2"),
    "interfaces": tb.InterfaceDiffusionModel(tb.ConstantCoefficient(args.G), "φₘ", "φₘi"),
}
fun = tb.semidiscretize_ep(tb.ReactionDiffusionSplit(models), tb.PatchAssemblyStrategy(dev), grid2)
u0 = np.zeros(tb.solution_size(fun.functions))
u0[fun.heat_dofrange] = np.maximum(1.0 - np.linalg.norm(tb.dof_coordinates(fun.dh), axis=1), 0.0)   # φₘ sits where heat_dofrange says
cache = tb.setup_solver_cache(fun.functions, tb.ForwardEulerCellSolver(dev), u=dev.to_device(u0))
ltg = tb.MultiDomainLieTrotterGodunov(fun.heat_stage(tb.BackwardEulerSolver()), fun.functions, cache)
dt, t, steps, its = 1.0, 0.0, 0, 0
t0 = time.perf_counter()
while t < args.tend - 1e-9:
    assert ltg.step(t, dt)
    its += ltg.heat.last_iters
    t += dt; steps += 1
dev.synchronize()
el = time.perf_counter() - t0
u = cache.u.to_host()
phi = u[fun.heat_dofrange]
on_pm = np.zeros(fun.dh.ndofs, dtype=bool); on_pm[fun.subdofs[0]] = True
print(json.dumps({"workload": "pacemaker subdomain, %d² quadrilaterals, FHN | FHN, G=%g, LTG(BE+CG, FE), dt=1, t_end=%g" % (args.n, args.G, args.tend),
                  "interface_elements": len(grid2.interfaces), "dofs": fun.dh.ndofs, "solution_size": len(u), "time_steps": steps,
                  "ms_per_time_step": el / steps * 1e3, "cg_iterations_per_step": its / steps, "moved": bool(not np.allclose(u, u0)),
                  "phi_range_pacemaker": [float(phi[on_pm].min()), float(phi[on_pm].max())],
                  "phi_range_myocardium": [float(phi[~on_pm].min()), float(phi[~on_pm].max())]}))
