#!/usr/bin/env python3
"""The reaction-eikonal ECG (the tutorial the reference plans as docs/src/literate-tutorials/ep05_eikonal.jl and has not written) at toy size:
  1. an idealised left ventricle with a rule-based fibre field (helix angle +80° … −65° across the wall),
  2. G = squared conduction velocity, a SpectralTensorCoefficient over that field (fast along the fibre),
  3. activation times from √(∇Tᵀ G ∇T) = 1 started at a few endocardial nodes with staggered onsets (solve_activation: the fast iterative method on
     the device),
  4. an action-potential template from one FitzHugh–Nagumo cell (ActionPotentialTemplate.from_cell_model),
  5. φₘ(x, t) = U(t − T(x)) on a time grid into the Plonsey pseudo-ECG of the package — no reaction–diffusion step is taken.
The potential recovery, the flux update and the volume integral of a sample only enqueue; they are captured once in one DeviceGraph and replayed per
sample.  Prints the activation summary and the trace at four electrodes, then one JSON line."""
import argparse, json, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("--nc", type=int, default=16)
ap.add_argument("--nr", type=int, default=3)
ap.add_argument("--nl", type=int, default=8)
ap.add_argument("--samples", type=int, default=40)
ap.add_argument("--velocity", type=float, nargs=3, default=[0.06, 0.03, 0.02], help="conduction velocity along fibre, sheet, normal (length / time)")
args = ap.parse_args()
import thunderbolt_jl_amd as tb
dev = tb.MI355XDevice(0)
grid = tb.generate_ideal_lv_mesh_hex(args.nc, args.nr, args.nl)
dh = tb.DofHandler(grid)
f, s, n = tb.ideal_lv_microstructure(grid)
G = tb.SpectralTensorCoefficient(tb.OrthotropicMicrostructureModel(f, s, n), tb.ConstantCoefficient(np.square(args.velocity)))

# activation: three endocardial nodes (transmural fraction 0) spread over the cavity surface, 0, 2 and 4 time units apart
endo = np.flatnonzero(grid.parametric[:, 2] == 0.0)
sources = endo[np.linspace(0, len(endo) - 1, 5).astype(int)[1:4]]
cache = tb.EikonalActivationCache(dev, tb.EikonalModel(G), dh)
T = tb.solve_activation(cache, sources, times=[0.0, 2.0, 4.0])
Th = T.to_host()
res = np.abs(cache.residual().to_host())
print("activation: %d nodes, %d sweeps, converged %s, last activation at t = %.3f, max |residual| / T = %.2e"
      % (dh.ndofs, cache.sweeps, cache.converged, Th.max(), (res / np.maximum(Th, 1e-300)).max()))

# template: one FHN cell pushed over its threshold, sampled every 0.5 time units
template = tb.ActionPotentialTemplate.from_cell_model(tb.FHNModel(), 0.5, 400.0, 0.5, device=dev, substeps=10)

# ECG: φₘ(t) → Plonsey integral at four electrodes around the ventricle
kappa_i, kappa_t = 2.0e-3, 6.0e-3
op = tb.setup_operator(tb.PerColorAssemblyStrategy(dev), tb.BilinearDiffusionIntegrator(tb.ConstantCoefficient(kappa_i)), dh, tb.allocate_matrix(dh))
phi = tb.activation_potential(cache, 0.0, template)
plonsey = tb.Plonsey1964ECGGaussCache(op, phi)
electrodes = np.array([[3.0, 0, 0], [-3.0, 0, 0], [0, 3.0, 0], [0, 0, -3.0]])
x_el = dev.to_device(electrodes.ravel())
sample = dev.zeros(len(electrodes))
trace = dev.zeros(len(electrodes) * args.samples)
times = np.linspace(0.0, Th.max() + 300.0, args.samples)


def one_sample():
    tb.activation_potential(cache, 0.0, template, out=phi)       # inside the graph the time comes from DeviceGraph.launch(t)
    tb.update_ecg(plonsey, phi)
    tb.evaluate_ecg(plonsey, x_el, kappa_t, out=sample)


one_sample()                                                      # once uncaptured: the reduction workspace exists before the capture
graph = dev.capture(one_sample)
for k, t in enumerate(times):
    graph.launch(float(t))
    tb.check(tb.lib().tb_memcpy_d2d(dev.h, trace.view(k * sample.n, sample.n).ptr, sample.ptr, sample.nbytes))
dev.synchronize()
ecg = trace.to_host().reshape(args.samples, -1)
print("   t      " + "  ".join("electrode %d  " % e for e in range(len(electrodes))))
for t, row in zip(times, ecg):
    print("%7.2f  " % t + "  ".join("%+.6e" % v for v in row))
print(json.dumps({"workload": "eikonal activation + template potential + Plonsey ECG, ideal LV %dx%dx%d" % (args.nc, args.nr, args.nl),
                  "nodes": int(dh.ndofs), "sweeps": int(cache.sweeps), "converged": bool(cache.converged), "activation_end": float(Th.max()),
                  "graph_nodes": graph.nodes, "ecg_finite": bool(np.isfinite(ecg).all()), "ecg_range": [float(ecg.min()), float(ecg.max())]}))
