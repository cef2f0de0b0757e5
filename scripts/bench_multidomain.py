"""Times multi-domain electrophysiology on one MI355X against the unchanged single-domain step.  Prints ONE JSON line.

An n³ box of hexahedra (default 128³) is split by the lattice plane in the middle of x into the cell sets "a" and "b"; insert_interfaces duplicates the
n_y·n_z-facet plane between them.  Timed with device events behind the _preroll pre-roll (the better of two loops of `--reps` calls, no profiler):

  interface_assembly   tb_interface_assemble alone (both kernels), into a value array of the widened pattern
  multi_step           MultiDomainLieTrotterGodunov.step, and its parts one by one: gather (tb_gather_indexed), heat (BackwardEulerStage.perform_step
                       on the widened pattern), scatter (tb_scatter_indexed), children (one reaction launch per child)
  single_step          the unchanged LieTrotterGodunov step (StateBlocked state, φₘ a view) of the model of subdomain "b" on the UNSPLIT mesh of the
                       same size, in the same process: the parent commit's code, the yardstick;  ratio = multi_step / single_step.  Its heat and
                       reaction stages are timed one by one as well

for both child layouts, and for `--ionic fhn` (FHN | FHN) or `--ionic tt06` (TT06 | FHN).  Each timed step starts from the same state (copied back
before every loop), so the CG iteration counts of the loops agree; they are reported.

    python scripts/bench_multidomain.py [--n 128] [--ionic fhn|tt06] [--reps 10] [--dt 0.01]

Every timed step is checked: a failed heat solve or a non-finite state ends the run."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import numpy as np  # noqa: E402

import thunderbolt_jl_amd as tb  # noqa: E402
from _preroll import preroll  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=128)
ap.add_argument("--ionic", default="fhn", choices=["fhn", "tt06"])
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--dt", type=float, default=None, help="default 0.01; 0.001 with --ionic tt06 (forward Euler on its gates)")
args = ap.parse_args()

dev = tb.MI355XDevice(0)
lib, check = tb.lib(), tb._lib.check
n, dt = args.n, args.dt or (0.001 if args.ionic == "tt06" else 0.01)


def ok(flag):
    if not flag:
        raise SystemExit("a timed step failed")


def timed(fn, reset=None):
    """ms per call: pre-roll, then the better of two event-timed loops"""
    preroll(dev, fn)
    best = None
    for _ in range(2):
        if reset:
            reset()
        e0, e1 = dev.event(), dev.event()
        e0.record()
        for _ in range(args.reps):
            fn()
        e1.record()
        dev.synchronize()
        ms = e0.elapsed_ms(e1) / args.reps
        best = ms if best is None else min(best, ms)
    return best


# conductivities a thousand times the reference tutorial's: with Δt = 0.01 on h = 2/n the heat step then needs a handful of CG iterations
# (Δt·κ/h² ≈ 2 at n = 128) instead of meeting its tolerance at the initial guess, so the stage that dominates a production step is in the timing
kap = tb.ConstantCoefficient(np.diag([4.5e-2, 2.0e-2, 2.0e-2]))
one = tb.ConstantCoefficient(1.0)
ion_a = tb.TT06() if args.ionic == "tt06" else tb.FHNModel()
ion_b = tb.FHNModel()
strategy = tb.PatchAssemblyStrategy(dev)
res = {"device": dev.info()["name"], "box": "%d^3 hexahedra split by a plane" % n, "ionic": "%s | fhn" % args.ionic, "dt": dt, "reps": args.reps}


def phi0_of(x):
    return np.exp(-8.0 * ((x[:, 0] + 0.1) ** 2 + x[:, 1] ** 2 + x[:, 2] ** 2))


# ---- the yardstick: the single-domain LieTrotterGodunov step on the unsplit mesh
g = tb.generate_mesh(tb.Hexahedron, (n, n, n), (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
dh = tb.DofHandler(g)
D = tb.ConductivityToDiffusivityCoefficient(kap, one, one)
heat = tb.BackwardEulerStage(tb.BackwardEulerSolver(), strategy, dh, D)
f1 = tb.PointwiseODEFunction(dh.ndofs, ion_b)
s0 = np.tile(ion_b.default_initial_state(), (dh.ndofs, 1))
s0[:, ion_b.phi_index] += phi0_of(tb.dof_coordinates(dh))
s0 = np.ascontiguousarray(s0.T).ravel()
u1 = dev.to_device(s0)
keep1 = dev.to_device(s0)
c1 = tb.setup_solver_cache(f1, tb.ForwardEulerCellSolver(dev), u=u1, keep_du=False)
ltg1 = tb.LieTrotterGodunov(heat, f1, c1)
restore1 = lambda: check(lib.tb_memcpy_d2d(dev.h, u1.ptr, keep1.ptr, u1.nbytes))  # noqa: E731
t_single = timed(lambda: ok(ltg1.step(0.0, dt)), restore1)
its1 = heat.last_iters
keep_phi1 = dev.to_device(s0[ion_b.phi_index * dh.ndofs:(ion_b.phi_index + 1) * dh.ndofs])
parts1 = {"heat": timed(lambda: ok(heat.perform_step(ltg1.phi, 0.0, dt)), lambda: check(lib.tb_memcpy_d2d(dev.h, ltg1.phi.ptr, keep_phi1.ptr, ltg1.phi.nbytes))),
          "reaction": timed(lambda: tb.perform_step(f1, c1, 0.0, dt), restore1)}
res["single_step"] = {"ms": round(t_single, 4), "dofs": dh.ndofs, "cg_iterations_last": its1, "parts_ms": {k: round(v, 4) for k, v in parts1.items()}}
del keep_phi1
del ltg1, c1, u1, keep1, heat, f1

# ---- the split mesh
c = np.arange(n ** 3).reshape(n, n, n)
g.addcellset("a", c[:, :, : n // 2].ravel())
g.addcellset("b", c[:, :, n // 2:].ravel())
g2 = tb.insert_interfaces(g, ["a", "b"])
models = {"a": tb.MonodomainModel(one, one, kap, tb.NoStimulationProtocol(), ion_a, "φₘ", "s1"),
          "b": tb.MonodomainModel(one, one, kap, tb.NoStimulationProtocol(), ion_b, "φₘ", "s2"),
          "interfaces": tb.InterfaceDiffusionModel(tb.ConstantCoefficient(1.0e-3), "φₘ", "φₘi")}
res["interface_elements"] = len(g2.interfaces)
for layout in (tb.PointBlockedLayout(), tb.StateBlockedLayout()):
    name = type(layout).__name__
    fun = tb.semidiscretize_ep(tb.ReactionDiffusionSplit(models), strategy, g2, layout=layout)
    if "interface_assembly" not in res:
        nz = dev.zeros(fun.pattern.nnz)
        t_if = timed(lambda: fun.interface_form.assemble(fun.K.pattern, nz))
        res["interface_assembly"] = {"ms": round(t_if, 4), "nnz_widened": fun.pattern.nnz, "nnz_narrow": tb.allocate_matrix(fun.dh).nnz}
        del nz
    u0 = fun.initial_condition()
    amp = np.ones(fun.dh.ndofs)
    amp[fun.subdofs[0]] = 50.0 if args.ionic == "tt06" else 1.0        # TT06 counts millivolts
    u0[fun.heat_dofrange] += amp * phi0_of(tb.dof_coordinates(fun.dh))
    u, keep = dev.to_device(u0), dev.to_device(u0)
    cache = tb.setup_solver_cache(fun.functions, tb.ForwardEulerCellSolver(dev), u=u, keep_du=False)
    ltg = tb.MultiDomainLieTrotterGodunov(fun.heat_stage(tb.BackwardEulerSolver()), fun.functions, cache)
    restore = lambda: check(lib.tb_memcpy_d2d(dev.h, u.ptr, keep.ptr, u.nbytes))  # noqa: E731
    t_multi = timed(lambda: ok(ltg.step(0.0, dt)), restore)
    its = ltg.heat.last_iters
    restore()
    check(lib.tb_gather_indexed(dev.h, ltg.n, u.ptr, ltg.idx.ptr, ltg.phi.ptr))
    keep_phi = dev.to_device(ltg.phi.to_host())
    parts = {"gather": timed(lambda: check(lib.tb_gather_indexed(dev.h, ltg.n, u.ptr, ltg.idx.ptr, ltg.phi.ptr))),
             "heat": timed(lambda: ok(ltg.heat.perform_step(ltg.phi, 0.0, dt)), lambda: check(lib.tb_memcpy_d2d(dev.h, ltg.phi.ptr, keep_phi.ptr, ltg.phi.nbytes))),
             "scatter": timed(lambda: check(lib.tb_scatter_indexed(dev.h, ltg.n, ltg.phi.ptr, ltg.idx.ptr, u.ptr))),
             "children": timed(lambda: ltg.reaction_step(0.0, dt), restore)}
    res["multi_step_" + name] = {"ms": round(t_multi, 4), "ratio_to_single_step": round(t_multi / t_single, 3), "cg_iterations_last": its,
                                 "parts_ms": {k: round(v, 4) for k, v in parts.items()}, "dofs": fun.dh.ndofs, "solution_size": fun.solution_size}
    if not np.isfinite(u.to_host()).all():
        raise SystemExit("non-finite state after the timed steps")
    del ltg, cache, u, keep, keep_phi, fun
print(json.dumps(res))
