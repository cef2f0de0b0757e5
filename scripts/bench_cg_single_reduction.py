"""Classic against single-reduction (Chronopoulos–Gear) Jacobi-CG of DistributedCG at one rank, on the heat matrix A = M − Δt·K of the 216³ box and
of its 108 / 54 / 27-layer slabs (the 2 / 4 / 8-GPU shares), products on the mirrored SpMV.  Prints ONE JSON line.

Per mesh and variant: the iteration time (tb_cgd_iteration / tb_cg1_iteration through DistributedCG.device_step / device_step1, after the _preroll
pre-roll, ≥ 50 iterations, the better of two loops, no profiler), the same iteration replayed as a HIP graph, the bytes one iteration moves and their
fraction of the HBM peak.  Bytes: 8 B per stored non-zero (the mirror streams values only) plus 8 B per dof and vector pass — classic 12 passes, as
bench.py counts them; single-reduction 14 (update: u, p, w, s, x, r, D⁻¹ read, p, s, x, r, u written; product: u read, w written).

The predicted 1 → N speed-up of one CG iteration is t₂₁₆ / (t_slab + k·L), k = 2 (classic) or 1 (single-reduction) blocking all-reduces per
iteration.  L is an ASSUMED all-reduce latency from the grid {10, 20, 40} µs, not a measurement: no multi-GPU node was measured.  If RCCL loads, the
line also carries the world-size-1 tb_comm_allreduce time of 3 doubles — a short-circuit at world size 1, not the latency of N GPUs.

    python scripts/bench_cg_single_reduction.py [--n 216] [--layers 108,54,27] [--iters 200]"""
import argparse
import gc
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import thunderbolt_jl_amd as tb  # noqa: E402
from _preroll import preroll  # noqa: E402

HBM_PEAK_GBS = 8000.0          # MI355X HBM3E spec, as bench.py
PASSES = {"classic": 12, "single_reduction": 14}
LATENCIES_US = (10.0, 20.0, 40.0)


def best_of_two(dev, fn, nit):
    ts = []
    for _ in range(2):
        dev.synchronize()
        t0 = time.perf_counter()
        for _ in range(nit):
            fn()
        dev.synchronize()
        ts.append((time.perf_counter() - t0) / nit)
    return min(ts)


def measure(dev, n, layers, nit):
    g = tb.generate_mesh(tb.Hexahedron, (n, n, layers), (0.0, 0.0, 0.0), (1.0, 1.0, layers / n), perturb=0.2)
    dh = tb.DofHandler(g)
    sp = tb.allocate_matrix(dh)
    st = tb.PatchAssemblyStrategy(dev)
    kap = np.diag([4.5e-5, 2.0e-5, 2.0e-5])
    M = tb.setup_operator(st, tb.BilinearMassIntegrator(tb.ConstantCoefficient(1.0)), dh, sp)
    K = tb.setup_operator(st, tb.BilinearDiffusionIntegrator(tb.ConstantCoefficient(kap)), dh, sp)
    tb.update_operators(M, K, 0.0)
    A = tb.heat_system_matrix(dev, M, K, 0.01)
    npts = dh.ndofs
    diag = torch.empty(npts, dtype=torch.float64, device="cuda")
    tb._lib.check(tb.lib().tb_extract_diagonal(K.pattern.h, A.ptr, diag.data_ptr()))
    mirrored = bool(K.pattern.mirror(A))
    b = torch.from_numpy(np.cos(np.linspace(0.0, 9.0, npts))).cuda()
    out = {"layers": layers, "ndofs": npts, "nnz": int(sp.nnz), "mirrored_spmv": mirrored}
    for variant in ("classic", "single_reduction"):
        cg = tb.distributed.DistributedCG(None, diag, None, None, 0, 1, None, device=dev, operator=(K.pattern, A), variant=variant)
        x = torch.zeros(npts, dtype=torch.float64, device="cuda")
        if variant == "classic":                                      # the state bench.py's time_cg iterates
            r = b.clone()
            p = cg.dinv * r
            Ap = torch.empty_like(x)
            S = torch.zeros(6, dtype=torch.float64, device="cuda")
            tb._lib.check(tb.lib().tb_cgd_dot(dev.h, npts, cg.w.data_ptr(), r.data_ptr(), p.data_ptr(), S[0:1].data_ptr()))
            step = lambda: cg.device_step(x, r, p, Ap, S)  # noqa: E731
        else:
            st1 = cg.device_setup1(b, x)
            step = lambda: cg.device_step1(x, *st1)  # noqa: E731
        preroll(dev, step)
        t_it = best_of_two(dev, step, nit)
        gr = dev.capture(step)
        preroll(dev, lambda: gr.launch(0.0))
        t_graph = best_of_two(dev, lambda: gr.launch(0.0), nit)
        nodes = gr.nodes
        gr.close()
        gc.enable()
        nbytes = 8.0 * sp.nnz + PASSES[variant] * 8.0 * npts
        out[variant] = {"iteration_ms": t_it * 1e3, "graph_iteration_ms": t_graph * 1e3, "graph_nodes": nodes, "bytes_per_iteration": nbytes,
                        "hbm_frac": nbytes / (t_it * HBM_PEAK_GBS * 1e9), "hbm_frac_graph": nbytes / (t_graph * HBM_PEAK_GBS * 1e9)}
    out["ratio_single_reduction_over_classic"] = out["single_reduction"]["iteration_ms"] / out["classic"]["iteration_ms"]
    out["ratio_graph"] = out["single_reduction"]["graph_iteration_ms"] / out["classic"]["graph_iteration_ms"]
    del M, K, A, sp, dh, g
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    return out


def rccl_world1(dev):
    """world-size-1 tb_comm_allreduce of 3 doubles (None when RCCL does not load)"""
    try:
        comm = tb.distributed.RcclComm(dev, 0, 1)
    except Exception as ex:
        return {"error": str(ex)[:200]}
    t = torch.zeros(3, dtype=torch.float64, device="cuda")
    for _ in range(50):
        comm.allreduce(t)
    ms = best_of_two(dev, lambda: comm.allreduce(t), 500) * 1e3
    comm.close()
    return {"allreduce_3_doubles_ms": ms, "world_size": 1, "note": "world size 1: RCCL short-circuits; not the latency of an N-GPU all-reduce"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=216)
    ap.add_argument("--layers", default="108,54,27")
    ap.add_argument("--iters", type=int, default=200)
    args = ap.parse_args()
    nit = max(50, args.iters)
    torch.cuda.set_stream(torch.cuda.Stream())
    dev = tb.MI355XDevice(0)
    dev.set_stream(torch.cuda.current_stream().cuda_stream)
    meshes = {str(args.n): measure(dev, args.n, args.n, nit)}
    for L in [int(v) for v in args.layers.split(",") if v]:
        meshes[str(L)] = measure(dev, args.n, L, nit)
    t_full = {v: meshes[str(args.n)][v]["iteration_ms"] for v in PASSES}
    pred = {}
    for L in [int(v) for v in args.layers.split(",") if v]:
        ngpu = args.n // L
        for v, k in (("classic", 2), ("single_reduction", 1)):
            for lat in LATENCIES_US:
                pred["%d_gpus/%s/L=%gus" % (ngpu, v, lat)] = t_full[v] / (meshes[str(L)][v]["iteration_ms"] + k * lat * 1e-3)
    line = {"what": "CG iteration, classic vs single-reduction, one rank, heat matrix of the %d³ box and its slabs" % args.n,
            "device": dev.info()["name"], "iterations_timed": nit, "meshes": meshes,
            "predicted_speedup_cg": pred,
            "allreduce_latency_assumed_us": list(LATENCIES_US),
            "allreduce_latency_note": "ASSUMED latencies of a blocking all-reduce over N GPUs, not measured (no multi-GPU node); "
                                      "prediction = t_full / (t_slab + k·L), k = 2 classic, 1 single-reduction",
            "rccl": rccl_world1(dev)}
    sys.stdout.flush()
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
