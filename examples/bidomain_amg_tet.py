#!/usr/bin/env python3
"""A bidomain wave on a box of linear tetrahedra at toy size: unequal anisotropy ratios (κᵢ 3 : 1, κₑ 4 : 3), FitzHugh–Nagumo cells, φₑ grounded at the
far corner.  The stimulus is the bidomain's own: a balanced extracellular current between two electrodes (nodal currents, `source_e`) on top of a
depolarised corner.  A tetrahedral mesh has no GridHierarchy, so the geometric block multigrid does not apply;
`precond=BidomainAMGPrecon()` builds one smoothed-aggregation V(2, 2) cycle on the node pairs (φₘ, φₑ) from the matrix alone.  The same run with the
block-Jacobi preconditioner is made beside it: the two potentials agree to the solver's tolerance and the algebraic multigrid takes the fewer
iterations.  Prints one JSON line: the levels, iterations per step of both, and the largest difference of the two φₘ and φₑ fields."""
import argparse, json, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=8, help="lattice cells per edge (six tetrahedra each)")
ap.add_argument("--steps", type=int, default=6)
ap.add_argument("--dt", type=float, default=0.5)
ap.add_argument("--max-coarse", type=int, default=64)
args = ap.parse_args()
import thunderbolt_jl_amd as tb
dev = tb.MI355XDevice(0)
L = 0.25 * args.n
g = tb.generate_mesh(tb.Tetrahedron, (args.n, args.n, args.n), (0, 0, 0), (L, L, L))
dh = tb.DofHandler(g)
sp = tb.allocate_matrix(dh)
model = tb.ParabolicEllipticBidomainModel(tb.ConstantCoefficient(1.0), tb.ConstantCoefficient(1.0),
                                          tb.ConstantCoefficient(np.diag([3.0, 1.0, 1.0]) * 1e-2),      # κᵢ: 3 : 1
                                          tb.ConstantCoefficient(np.diag([2.0, 1.5, 1.5]) * 1e-2),      # κₑ: 4 : 3
                                          tb.NoStimulationProtocol(), tb.FHNModel())
Di, De = model.diffusivities()
X = tb.dof_coordinates(dh)
anode, cathode = np.flatnonzero((X <= 0.5).all(axis=1)), np.flatnonzero((X[:, 0] >= L - 0.5) & (X[:, 1:] <= 0.5).all(axis=1))
current = np.zeros(dh.ndofs)
current[anode], current[cathode] = 0.02 / len(anode), -0.02 / len(cathode)                              # sums to zero: the boundary is sealed
ground = [tb.get_closest_vertex((L, L, L), g)]                                                         # φₑ = 0 at the far corner
n = dh.ndofs


def run(precond):
    heat = tb.BidomainBackwardEulerStage(tb.BackwardEulerSolver(rtol=1e-6, atol=1e-8, maxiter=20000), tb.PerColorAssemblyStrategy(dev), dh, Di, De, ground, source_e=current,
                                         pattern=sp, precond=precond)
    f = tb.PointwiseODEFunction(n, model.ion)
    cache = tb.setup_solver_cache(f, tb.ForwardEulerCellSolver(dev), u=dev.to_device(np.concatenate([1.0 * (X <= 0.75).all(axis=1), np.zeros(n)])))
    ltg = tb.LieTrotterGodunov(heat, f, cache)
    ok, its = True, []
    for s in range(args.steps):
        ok = ltg.step(s * args.dt, args.dt) and ok
        its.append(heat.last_iters)
    return ok, its, cache.un.to_host()[:n], heat.phi_e.to_host(), heat


ok_mg, its_mg, pm_mg, pe_mg, heat = run(tb.BidomainAMGPrecon(max_coarse=args.max_coarse))
ok_bj, its_bj, pm_bj, pe_bj, _ = run(None)
mg = heat.multigrid
print(json.dumps({"workload": "bidomain + FHN on tetrahedra, %d nodes (%d unknowns), %d cells, LTG(BE + AMG PCG, forward Euler), dt=%g" % (n, 2 * n, g.n_cells, args.dt),
                  "levels": [mg.level_size(l)[0] for l in range(mg.n_levels)], "all_converged": bool(ok_mg and ok_bj),
                  "iterations_amg": its_mg, "iterations_block_jacobi": its_bj, "setups": mg.setups, "aggregations": mg.aggregations,
                  "lambda_max": [mg.lambda_max(l) for l in range(mg.n_levels - 1)],
                  "phi_m_range": [float(pm_mg.min()), float(pm_mg.max())], "phi_e_range": [float(pe_mg.min()), float(pe_mg.max())],
                  "phi_e_at_ground": float(pe_mg[tb.vertex_dofs(dh)[ground[0]]]),
                  "max_difference_phi_m": float(np.abs(pm_mg - pm_bj).max()), "max_difference_phi_e": float(np.abs(pe_mg - pe_bj).max())}))
