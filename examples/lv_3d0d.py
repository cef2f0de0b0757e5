#!/usr/bin/env python3
"""3D-0D coupling of an idealised left ventricle with a closed-loop lumped circulation on one MI355X (Regazzoni et al. 2022), the reference's
tutorial docs/src/literate-tutorials/cm03_3d0d-coupling.jl at the toy size of test/integration/test_fsi.jl: Guccione passive tissue with
SimpleActiveStress driven by the Pelce–Sun–Langeveld model and a piecewise-linear calcium transient, normal springs on the epicardium and the
base, four anchors, and the chamber pressure an unknown tied to the cavity volume the circuit supplies.  Every step: V0D ← circuit, blocked Newton
on [d; p] (device facet integrals, device Krylov solves inside a Schur complement), p → circuit, circuit over Δt (host RK4).
Prints t, p_LV, V3D and V0D per step.  The all-hex generator needs a circumferential count divisible by 4, so the smallest mesh is (8, 1, 2)
where the reference's mixed-cell generator uses (6, 1, 2)."""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def calcium_profile(t_global):
    """test_fsi.jl:96-107: 0 → 1 over 120 ms, back to 0 at 272 ms, period 800 ms"""
    t = t_global % 800.0
    if 0 <= t <= 120.0:
        return t / 120.0
    if t <= 272.0:
        return 1.0 + (t - 120.0) * (0.0 - 1.0) / (272.0 - 120.0)
    return 0.0


def setup(tb, dev, nc=8, nr=1, nl=2, prepace_beats=10, newton_tol=1e-2):
    scaling_factor = 3.9
    g = tb.generate_ideal_lv_mesh_hex(nc, nr, nl, inner_radius=scaling_factor * 0.7, outer_radius=scaling_factor * 1.0, longitudinal_upper=0.4,
                                      apex_inner=scaling_factor * 1.3, apex_outer=scaling_factor * 1.5)
    f, s, n = tb.ideal_lv_microstructure(g, np.deg2rad(80.0), np.deg2rad(-65.0))
    dh = tb.DofHandler(g, tb.LagrangeCollection(1) ** 3)
    sp = tb.allocate_matrix(dh)
    material = tb.ActiveStressModel(tb.Guccione1991PassiveModel(), tb.SimpleActiveStress(),
                                    tb.CaDrivenInternalSarcomereModel(tb.PelceSunLangeveld1995Model(), calcium_profile), tb.OrthotropicMicrostructureModel(f, s, n))
    solid = tb.QuasiStaticModel("d", material, (tb.NormalSpringBC(0.1, "Epicardium"), tb.NormalSpringBC(0.1, "Base")))
    # the circuit alone, every pressure given, over ten beats: a periodic initial state
    u0fluid = tb.prepace_circuit(tb.RSAFDQ2022LumpedCicuitModel(), beats=prepace_beats)
    circuit = tb.RSAFDQ2022LumpedCicuitModel(lv_pressure_given=False)
    coupler = tb.LumpedFluidSolidCoupler([tb.ChamberVolumeCoupling("Endocardium", "lv-volume-control", tb.RSAFDQ2022SurrogateVolume(), "Vₗᵥ", "pₗᵥ", "pₗᵥ")], "d")
    nd0 = np.empty(g.n_nodes, dtype=np.int64)
    nd0[g.conn.ravel()] = dh.cell_dofs[:, 0::3].ravel()
    a = [g.getnodeset("MyocardialAnchor%d" % k)[0] for k in (1, 2, 3, 4)]
    ch = tb.ConstraintHandler(dh, np.concatenate([nd0[a[0]] + np.arange(3), nd0[a[1]] + np.array([1, 2]), [nd0[a[2]] + 2], [nd0[a[3]] + 2]]))
    fun = tb.semidiscretize_rsafdq(tb.RSAFDQ2022Split(tb.RSAFDQ2022Model(solid, circuit, coupler)), tb.ElementAssemblyStrategy(dev), dh, sp, ch)
    fun.circuit_state = u0fluid.copy()
    newton = tb.NewtonRaphsonSolver(max_iter=10, tol=newton_tol, inner_solver=tb.SchurComplementLinearSolver("gmres"), inner_rtol=1e-10, inner_maxiter=20000,
                                    gmres_restart=200)
    integrator = tb.RSAFDQ2022Integrator(fun, tb.HomotopyPathSolver(newton))
    return fun, integrator, u0fluid


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--dt", type=float, default=1.0, help="time step [ms]")
    ap.add_argument("--nc", type=int, default=8)
    ap.add_argument("--nr", type=int, default=1)
    ap.add_argument("--nl", type=int, default=2)
    args = ap.parse_args()
    import thunderbolt_jl_amd as tb
    dev = tb.MI355XDevice(0)
    fun, integrator, _ = setup(tb, dev, args.nc, args.nr, args.nl)
    iv = fun.chambers[0].volume_index
    print("%8s %14s %14s %14s  newton" % ("t [ms]", "p_LV [kPa]", "V3D [mL]", "V0D [mL]"))
    for _ in range(args.steps):
        v0d = float(fun.circuit_state[iv])
        if not integrator.step(args.dt):
            print("step at t = %g failed: %s" % (integrator.t, integrator.chamber_solver.inner_solver.linear_failure))
            return 1
        print("%8.2f %14.6e %14.6e %14.6e  %d" % (integrator.t, fun.pressures[0], fun.V3D[0], v0d, integrator.chamber_solver.inner_solver.iter))
    return 0


if __name__ == "__main__":
    sys.exit(main())
