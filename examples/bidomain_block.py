#!/usr/bin/env python3
"""Parabolic–elliptic bidomain on a slab: fibres along x, κₑ not proportional to κᵢ (unequal anisotropy ratios), FitzHugh–Nagumo, a stimulus in one
corner, φₑ read at two nodes as a lead.  The extracellular potential is an unknown of the step (BidomainBackwardEulerStage), not a reconstruction;
the stage goes into the unchanged LieTrotterGodunov.  Toy size; prints one JSON line."""
import argparse, json, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("--nx", type=int, default=24, help="cells along the fibre (a quarter as many across)")
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--dt", type=float, default=0.5)
args = ap.parse_args()
import thunderbolt_jl_amd as tb
dev = tb.MI355XDevice(0)
ny = max(2, args.nx // 4)
L = 0.25 * args.nx
g = tb.generate_mesh(tb.Hexahedron, (args.nx, ny, ny), (0, 0, 0), (L, 0.25 * ny, 0.25 * ny))
dh = tb.DofHandler(g)
sp = tb.allocate_matrix(dh)
model = tb.ParabolicEllipticBidomainModel(tb.ConstantCoefficient(1.0), tb.ConstantCoefficient(1.0),
                                          tb.ConstantCoefficient(np.diag([3.0, 1.0, 1.0]) * 1e-2),      # κᵢ: 3 : 1
                                          tb.ConstantCoefficient(np.diag([2.0, 1.5, 1.5]) * 1e-2),      # κₑ: 4 : 3
                                          tb.NoStimulationProtocol(), tb.FHNModel())
Di, De = model.diffusivities()
# the stage adds `source` as BackwardEulerStage does, per step and not per unit of time: 0.3 a step for three steps lifts the corner over the threshold
stim = tb.LinearIntegrator(tb.AnalyticalCoefficient(lambda x, t: 0.3 * (t <= 1.75) * (x[0] <= 0.5 and x[1] <= 0.5 and x[2] <= 0.5)))
ground = [tb.get_closest_vertex((L, 0.0, 0.0), g)]                                                     # φₑ = 0 at the far corner
heat = tb.BidomainBackwardEulerStage(tb.BackwardEulerSolver(rtol=1e-6, atol=1e-8, maxiter=20000), tb.PerColorAssemblyStrategy(dev), dh, Di, De, ground, source=stim, pattern=sp)
n = dh.ndofs
u0 = np.zeros((2, n))
f = tb.PointwiseODEFunction(n, model.ion)
cache = tb.setup_solver_cache(f, tb.ForwardEulerCellSolver(dev), u=dev.to_device(u0.ravel()))
ltg = tb.LieTrotterGodunov(heat, f, cache)
n2d = tb.vertex_dofs(dh)
a, b = n2d[tb.get_closest_vertex((0.25 * L, 0.0, 0.0), g)], n2d[tb.get_closest_vertex((0.75 * L, 0.0, 0.0), g)]
ok, its, lead = True, 0, []
for s in range(args.steps):
    ok = ltg.step(s * args.dt, args.dt) and ok
    its += heat.last_iters
    pe = heat.phi_e.to_host()
    lead.append(float(pe[a] - pe[b]))
u = cache.un.to_host()
pe = heat.phi_e.to_host()
print(json.dumps({"workload": "bidomain + FHN, %dx%dx%d hex Q1 (%d dofs, %d unknowns), LTG(BE + block-Jacobi PCG, forward Euler), dt=%g" % (args.nx, ny, ny, n, 2 * n, args.dt),
                  "all_converged": bool(ok), "cg_iterations_per_step": its / args.steps, "phi_m_range": [float(u[:n].min()), float(u[:n].max())],
                  "phi_e_range": [float(pe.min()), float(pe.max())], "phi_e_at_ground": float(pe[n2d[ground[0]]]), "lead": lead[-1], "lead_trace": lead}))
