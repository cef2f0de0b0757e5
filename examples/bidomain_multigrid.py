#!/usr/bin/env python3
"""The slab of bidomain_block.py with the block system preconditioned by geometric multigrid: the grid is the finest of a GridHierarchy (a coarse slab
refined `--refinements` times), and `precond=GMGPrecon(gh)` gives the stage one V(2, 2) cycle on the node pairs (φₘ, φₑ) per CG iteration instead of the
inverse 2 × 2 diagonal blocks.  The same run without `precond` is made beside it: the two potentials agree to the solver's tolerance, the multigrid count
is the smaller one and does not grow with the refinements.  Toy size; prints one JSON line."""
import argparse, json, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("--nx", type=int, default=6, help="cells of the coarsest grid along the fibre (a third as many across)")
ap.add_argument("--refinements", type=int, default=2)
ap.add_argument("--steps", type=int, default=10)
ap.add_argument("--dt", type=float, default=0.5)
args = ap.parse_args()
import thunderbolt_jl_amd as tb
dev = tb.MI355XDevice(0)
ny = max(1, args.nx // 3)
cell = 0.25 * 2 ** args.refinements                                                                      # coarse cells of the size that refines to 0.25
L = cell * args.nx
gh = tb.GridHierarchy(tb.generate_mesh(tb.Hexahedron, (args.nx, ny, ny), (0, 0, 0), (L, cell * ny, cell * ny)), args.refinements)
g = gh.finest
dh = tb.DofHandler(g)
sp = tb.allocate_matrix(dh)
model = tb.ParabolicEllipticBidomainModel(tb.ConstantCoefficient(1.0), tb.ConstantCoefficient(1.0),
                                          tb.ConstantCoefficient(np.diag([3.0, 1.0, 1.0]) * 1e-2),      # κᵢ: 3 : 1
                                          tb.ConstantCoefficient(np.diag([2.0, 1.5, 1.5]) * 1e-2),      # κₑ: 4 : 3
                                          tb.NoStimulationProtocol(), tb.FHNModel())
Di, De = model.diffusivities()
stim = tb.LinearIntegrator(tb.AnalyticalCoefficient(lambda x, t: 0.3 * (t <= 1.75) * (x[0] <= 0.5 and x[1] <= 0.5 and x[2] <= 0.5)))
ground = [tb.get_closest_vertex((L, 0.0, 0.0), g)]                                                     # φₑ = 0 at the far corner
n = dh.ndofs


def run(precond):
    heat = tb.BidomainBackwardEulerStage(tb.BackwardEulerSolver(rtol=1e-6, atol=1e-8, maxiter=20000), tb.PerColorAssemblyStrategy(dev), dh, Di, De, ground, source=stim,
                                         pattern=sp, precond=precond)
    f = tb.PointwiseODEFunction(n, model.ion)
    cache = tb.setup_solver_cache(f, tb.ForwardEulerCellSolver(dev), u=dev.to_device(np.zeros(2 * n)))
    ltg = tb.LieTrotterGodunov(heat, f, cache)
    ok, its = True, 0
    for s in range(args.steps):
        ok = ltg.step(s * args.dt, args.dt) and ok
        its += heat.last_iters
    return ok, its / args.steps, cache.un.to_host()[:n], heat.phi_e.to_host(), heat


ok_mg, its_mg, pm_mg, pe_mg, heat = run(tb.GMGPrecon(gh))
ok_bj, its_bj, pm_bj, pe_bj, _ = run(None)
print(json.dumps({"workload": "bidomain + FHN, %d nodes (%d unknowns), %d multigrid levels, LTG(BE + multigrid PCG, forward Euler), dt=%g" % (n, 2 * n, heat.multigrid.n_levels, args.dt),
                  "all_converged": bool(ok_mg and ok_bj), "cg_iterations_per_step": its_mg, "block_jacobi_iterations_per_step": its_bj,
                  "lambda_max": [heat.multigrid.lambda_max(l) for l in range(1, heat.multigrid.n_levels)],
                  "phi_m_range": [float(pm_mg.min()), float(pm_mg.max())], "phi_e_range": [float(pe_mg.min()), float(pe_mg.max())],
                  "phi_e_at_ground": float(pe_mg[tb.vertex_dofs(dh)[ground[0]]]),
                  "max_difference_to_block_jacobi": [float(np.abs(pm_mg - pm_bj).max()), float(np.abs(pe_mg - pe_bj).max())]}))
