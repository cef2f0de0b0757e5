#!/usr/bin/env python3
"""The pseudo-ECG tutorial (docs/src/literate-tutorials/ep04_geselowitz-ecg.jl) at toy size: monodomain + FitzHugh–Nagumo on a 12³ heart block
[−1,1]³ inside a 16³ torso [−2,2]³, all three ECGs sampled every time step on the device —
  Plonsey1964ECGGaussCache        the volume integral over the heart, at the six face centres of the torso,
  PoissonECGReconstructionCache   ∇·κ∇φₑ = −∇·κᵢ∇φₘ on the torso, grounded at a torso corner,
  Geselowitz1989ECGLeadCache      one lead field per pair (corner, face centre).
Everything of a step that only enqueues — the reaction step, the Plonsey update and integral, the heart → torso transfers, the source products,
the lead products — is captured ONCE in one DeviceGraph and replayed with one launch per step; its samples land in fixed slots and are copied to
row k of the traces on the device.  The two CG solves (heat step, Poisson) look at their residual from the host and stay outside the graph.
Prints the extrema of the three traces and the Poisson / lead-field agreement, then one JSON line."""
import argparse, json, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=40)
ap.add_argument("--dt", type=float, default=1.0)
args = ap.parse_args()
import thunderbolt_jl_amd as tb
dev = tb.MI355XDevice(0)
heart = tb.generate_mesh(tb.Hexahedron, (12, 12, 12))
torso = tb.generate_mesh(tb.Hexahedron, (16, 16, 16), (-2, -2, -2), (2, 2, 2))
torso.addcellset("heart", lambda x: np.abs(x).max() <= 1.0)
hdh, tdh = tb.DofHandler(heart), tb.DofHandler(torso)
kappa_i, kappa = 2.0e-3, 6.0e-3                                    # intracellular and bulk conductivity (isotropic); Cₘ = χ = 1
n = hdh.ndofs

# monodomain: LieTrotterGodunov((BackwardEulerSolver(CG), ForwardEulerCellSolver()))
D = tb.ConductivityToDiffusivityCoefficient(tb.ConstantCoefficient(kappa_i), tb.ConstantCoefficient(1.0), tb.ConstantCoefficient(1.0))
heat = tb.BackwardEulerStage(tb.BackwardEulerSolver(rtol=1e-8, atol=1e-10), tb.PerColorAssemblyStrategy(dev), hdh, D)
X = tb.dof_coordinates(hdh)
u0 = np.zeros((2, n))
u0[0] = ((X[:, 0] <= -0.4) & (X[:, 1] <= 0.2)).astype(float)      # an excited corner, off the symmetry planes
u0[1] = 0.1 * (X[:, 1] >= 0.5)
f = tb.PointwiseODEFunction(n, tb.FHNModel())
cell = tb.setup_solver_cache(f, tb.ForwardEulerCellSolver(dev), u=dev.to_device(u0.ravel()), keep_du=False)
ltg = tb.LieTrotterGodunov(heat, f, cell)
phi = ltg.phi                                                      # φₘ: the first block of the state

# the three ECGs
faces = np.array([[-2.0, 0, 0], [2.0, 0, 0], [0, -2.0, 0], [0, 2.0, 0], [0, 0, -2.0], [0, 0, 2.0]])
corner = np.array([-2.0, -2.0, -2.0])
ground = [tb.get_closest_vertex(corner, torso)]
ki_torso = tb.cellset_coefficient(torso, "heart", inside=kappa_i)  # κᵢ in the heart cells, 0 outside
op_i = tb.setup_operator(tb.PerColorAssemblyStrategy(dev), tb.BilinearDiffusionIntegrator(tb.ConstantCoefficient(kappa_i)), hdh, heat.sp)
plonsey = tb.Plonsey1964ECGGaussCache(op_i, phi)
poisson = tb.PoissonECGReconstructionCache(dev, hdh, tdh, ki_torso, tb.ConstantCoefficient(kappa), np.vstack([corner, faces]), ground, torso_heart_domain="heart")
leads = tb.Geselowitz1989ECGLeadCache(dev, hdh, tdh, ki_torso, tb.ConstantCoefficient(kappa), [[corner, e] for e in faces], ground, torso_heart_domain="heart")

x_el = dev.to_device(faces.ravel())
s_pl, s_po, s_le = dev.zeros(6), dev.zeros(7), dev.zeros(6)        # the sample slots the graph writes
tr_pl, tr_po, tr_le = dev.zeros(6 * args.steps), dev.zeros(7 * args.steps), dev.zeros(6 * args.steps)
state = {"t": 0.0}


def enqueue_only_part():
    tb.perform_step(f, cell, state["t"], args.dt)                  # reaction
    tb.update_ecg(plonsey, phi)
    tb.evaluate_ecg(plonsey, x_el, kappa, out=s_pl)
    tb.update_ecg(leads, phi)
    tb.evaluate_ecg(leads, out=s_le)
    poisson.right_hand_side(phi)


def copy_row(dst, k, src):
    tb.check(tb.lib().tb_memcpy_d2d(dev.h, dst.view(k * src.n, src.n).ptr, src.ptr, src.nbytes))


saved = cell.un.to_host()
enqueue_only_part()                                                # once uncaptured: plans and workspaces exist before the capture
cell.un.copy_from_host(saved)
graph = dev.capture(enqueue_only_part)
its = 0
for k in range(args.steps):
    t = k * args.dt
    assert heat.perform_step(phi, t, args.dt)
    graph.launch(t)
    poisson.solve()
    tb.evaluate_ecg(poisson, out=s_po)
    for dst, src in ((tr_pl, s_pl), (tr_po, s_po), (tr_le, s_le)):
        copy_row(dst, k, src)
    its += poisson.last_iters
dev.synchronize()
pl, po, le = tr_pl.to_host().reshape(-1, 6), tr_po.to_host().reshape(-1, 7), tr_le.to_host().reshape(-1, 6)
agree = np.abs(le - (po[:, 1:] - po[:, :1])).max() / np.abs(po).max()
print("graph nodes per step: %d; Poisson CG iterations per step: %.1f; lead-field solves: %s iterations" % (graph.nodes, its / args.steps, leads.lead_iters))
for name, tr in (("Plonsey", pl), ("Poisson", po[:, 1:]), ("lead field", le)):
    print("%-10s min %+.6e  max %+.6e" % (name, tr.min(), tr.max()))
print("Poisson / lead-field agreement (max difference / max|φₑ|): %.3e" % agree)
phi_h = phi.to_host()
print(json.dumps({"workload": "monodomain + FHN, 12^3 heart in 16^3 torso, three ECGs per step", "steps": args.steps, "graph_nodes": graph.nodes,
                  "plonsey_range": [float(pl.min()), float(pl.max())], "poisson_range": [float(po.min()), float(po.max())],
                  "leadfield_range": [float(le.min()), float(le.max())], "poisson_leadfield_agreement": float(agree),
                  "phi_range": [float(phi_h.min()), float(phi_h.max())]}))
