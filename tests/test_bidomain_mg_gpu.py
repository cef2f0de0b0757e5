"""The multigrid preconditioner of the bidomain block system on the device (csrc/tb_bidomain_mg.hip, BidomainMultigrid) against the NumPy restatement of
tests/bidomain_mg_reference.py: the coarse operators plane by plane, λmax, one V-cycle, symmetry, bit identity, the preconditioned solve, the stage,
refusals and the example.  Meshes A (125 nodes, two levels) and B (1 989 nodes, three levels: the four-plane coarse product runs), each under the three
grounds: one vertex, two fine vertices that are no coarse vertices, a whole face."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bidomain_mg_reference as ref
import bidomain_reference as bref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(m, g) for m in ref.MESHES for g in ref.GROUNDS]
DEGREE, RATIO = 2, 4.0
# test_cycle_is_the_numpy_cycle: the reference's own error, measured on the host by ref.reference_deviation(problem, ground, DEGREE, RATIO) — the float64
# NumPy result against the same computation accumulated in np.longdouble with the coarsest solve refined, three right-hand sides, max |z − z_ld| / max |z_ld|,
# λmax = 1.05 λ*.  "whole": Galerkin chain and cycle both in extended precision (the figure the device is held to against the reference chain);
# "cycle alone": both cycles on the float64 chain (the figure the device is held to when the NumPy cycle runs on the device's own operators).  On mesh B the
# two differ by a decade and more: the float64 chain is off by 5e-16 of a level's largest entry, the coarsest operator's condition is 4.6e4 with the
# nearly constant φₑ as its smallest mode, and the cycle answers that rounding with 4e-14.  The device is allowed ten times the figure of its case
# (different summation orders, fused multiply-adds, the unpivoted Gauss–Jordan inverse in the place of a pivoted solve).  Measured on the device, worst of
# three right-hand sides: against the reference chain A 1.7e-15, 4.8e-16, 2.5e-16 and B 7.7e-14, 2.6e-14, 9.9e-16 (vertex, off_coarse, face); against the
# cycle on its own operators A 4.4e-15, 3.4e-16, 2.5e-16 and B 2.7e-15, 2.8e-15, 4.3e-16.
REFERENCE_DEVIATION = {          # (mesh, ground): (whole, cycle alone)
    ("A", "vertex"): (2.682e-15, 2.533e-15), ("A", "off_coarse"): (2.293e-16, 3.511e-16), ("A", "face"): (1.398e-16, 1.356e-16),
    ("B", "vertex"): (4.126e-14, 3.229e-15), ("B", "off_coarse"): (1.607e-14, 1.204e-15), ("B", "face"): (5.301e-16, 2.700e-16),
}

def strict_solver(tb, n):
    return tb.BackwardEulerSolver(rtol=1e-12, atol=0.0, maxiter=8 * n)


def relerr(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


@pytest.fixture(scope="module")
def setups(tb, device, oracle):
    """per (mesh, ground): the device system with its hierarchy set up, and the reference levels — computed once, never written"""
    cache = {}

    def get(name, kind):
        if name not in cache:
            p = ref.build_problem(tb, oracle, name)
            p["dev"] = tuple(device.to_device(a) for a in p["host"])
            p["pattern"] = p["dhs"][-1].device_mesh(device).pattern(p["sps"][-1])
            cache[name] = p
        p = cache[name]
        if (name, kind) not in cache:
            ground = ref.ground_dofs(p, kind)
            flags = np.zeros(p["n"], dtype=np.uint8)
            flags[ground] = 1
            sp, (M, Ki, Ke) = p["sps"][-1], p["host"]
            gd = bref.ground_diagonal(sp.rowptr, sp.colidx, Ki, Ke, bref.DT)
            system = tb.BidomainSystem(p["pattern"])
            system.set_matrices(*p["dev"], bref.DT, device.to_device(flags), gd)
            mg = tb.BidomainMultigrid(system, p["gh"], DEGREE, RATIO).setup()
            lv = ref.reference_levels(dict(p, dhs=mg.dhs, sps=mg.sps), kind)
            lv.update(system=system, mg=mg, lmax=[None] + [mg.lambda_max(l) for l in range(1, mg.n_levels)])
            cache[name, kind] = lv
        return p, cache[name, kind]
    return get


# ------------------------------------------------------------------------------------------------ 1. coarse operators
@pytest.mark.parametrize("name,kind", CASES)
def test_level_planes_are_the_reference_chain(setups, name, kind):
    p, lv = setups(name, kind)
    mg = lv["mg"]
    assert mg.n_levels == len(p["gh"].grids) == (2 if name == "A" else 3)
    for l in range(mg.n_levels):
        sp, A, g = mg.sps[l], lv["As"][l], lv["gs"][l]
        want, clean = ref.planes(A, sp)
        assert clean                                                          # nothing of 𝒫ᵀ𝒜𝒫 lies outside the level's scalar pattern
        got = mg.level_blocks(l)
        scale = max(np.abs(w).max() for w in want)
        errs = [np.abs(a - w).max() / scale for a, w in zip(got, want)]
        print("%s ground %s level %d: max |plane - reference| / max |entry| = %s" % (name, kind, l, ", ".join("%.2e" % e for e in errs)))
        assert max(errs) <= 1e-12
        rows = np.repeat(np.arange(len(sp.rowptr) - 1), np.diff(sp.rowptr))
        cols = sp.colidx
        gi, gj, diag = g[rows], g[cols], rows == cols
        assert np.all(got[1][gj] == 0.0) and np.all(got[2][gi] == 0.0) and np.all(got[3][(gi | gj) & ~diag] == 0.0)   # eliminated rows and columns: exactly zero
        if g.any():
            n = len(g)
            fill = A[n + np.flatnonzero(g), n + np.flatnonzero(g)]
            assert np.abs(got[3][gi & diag] - fill).max() <= 1e-12 * np.abs(fill).max()
    if kind == "off_coarse":                                                  # the case tests what it claims: a₁₂ ≠ a₂₁ᵀ on the first coarse level
        a12, a21 = mg.level_blocks(mg.n_levels - 2)[1:3]
        sp = mg.sps[-2]
        D12, D21 = bref.dense_of_csr(sp.rowptr, sp.colidx, a12), bref.dense_of_csr(sp.rowptr, sp.colidx, a21)
        assert np.abs(D12 - D12.T).max() > 1e-3 * np.abs(D12).max() and np.abs(D12 - D21.T).max() <= 1e-12 * np.abs(D12).max()


# ------------------------------------------------------------------------------------------------ 2. λmax
@pytest.mark.parametrize("name,kind", CASES)
def test_lambda_max_brackets_the_dense_eigenvalue(setups, name, kind):
    """λ* ≤ estimate ≤ 1.05 λ* (1 + 1e-12): a Ritz value never exceeds λ* and the inflation is 5 %; the lower bound is what the smoother needs"""
    _, lv = setups(name, kind)
    stars = ref.lambda_stars(lv["As"], lv["gs"])
    for l in range(1, len(stars)):
        print("%s ground %s level %d: lambda* %.12e, device %.12e (ratio %.6f)" % (name, kind, l, stars[l], lv["lmax"][l], lv["lmax"][l] / stars[l]))
        assert stars[l] <= lv["lmax"][l] <= 1.05 * stars[l] * (1.0 + 1e-12)


# ------------------------------------------------------------------------------------------------ 3. the cycle
def device_operators(mg, lv):
    """the level operators as the device holds them, dense and blocked (the fine level: the reference's own matrix, which the device stores bit for bit)"""
    out = []
    for l in range(mg.n_levels - 1):
        sp = mg.sps[l]
        d = [bref.dense_of_csr(sp.rowptr, sp.colidx, a) for a in mg.level_blocks(l)]
        out.append(np.block([[d[0], d[1]], [d[2], d[3]]]))
    return out + [lv["A"]]


@pytest.mark.parametrize("name,kind", CASES)
def test_cycle_is_the_numpy_cycle(device, setups, name, kind):
    """Two comparisons, both asserted, the NumPy cycle fed the device's λmax per level as test_multigrid_gpu.test_cycle_is_the_numpy_cycle does.
    (a) against the reference chain: the NumPy cycle on the reference's own coarse operators — independent of the device's set-up; bound: ten times the
    whole reference's deviation from its extended-precision restatement.  (b) the NumPy cycle on the device's level operators: the cycle's arithmetic
    alone, held to ten times the deviation of the NumPy cycle alone, a decade tighter on mesh B."""
    p, lv = setups(name, kind)
    n, mg = p["n"], lv["mg"]
    chain = ref.Cycle(lv["As"], lv["Ps"], lv["gs"], lv["lmax"], DEGREE, RATIO)
    own = ref.Cycle(device_operators(mg, lv), lv["Ps"], lv["gs"], lv["lmax"], DEGREE, RATIO)
    rng = np.random.default_rng(41)
    tol_chain, tol_own = (10.0 * v for v in REFERENCE_DEVIATION[name, kind])
    errs_chain, errs_own = [], []
    for k in range(3):
        r = rng.normal(size=2 * n)
        z = bref.deinterleave(mg.apply(device.to_device(bref.interleave(r)), device.zeros(2 * n)).to_host())
        errs_chain.append(relerr(z, chain(r)))
        errs_own.append(relerr(z, own(r)))
        assert np.all(z[n + lv["ground"]] == 0.0)                                     # r is non-zero there
    print("%s ground %s: max |z - z_numpy| / max |z_numpy| against the reference chain %s (allowed %.2e); with the NumPy cycle on the device's operators %s (allowed %.2e)"
          % (name, kind, ", ".join("%.3e" % e for e in errs_chain), tol_chain, ", ".join("%.3e" % e for e in errs_own), tol_own))
    assert max(errs_chain) <= tol_chain
    assert max(errs_own) <= tol_own


# ------------------------------------------------------------------------------------------------ 4. symmetry and positivity
def test_cycle_is_symmetric_and_positive(device, setups):
    p, lv = setups("B", "off_coarse")
    n, mg = p["n"], lv["mg"]
    rng = np.random.default_rng(42)
    u, v = rng.normal(size=2 * n), rng.normal(size=2 * n)
    mu = mg.apply(device.to_device(u), device.zeros(2 * n)).to_host()
    mv = mg.apply(device.to_device(v), device.zeros(2 * n)).to_host()
    asym = abs(u @ mv - v @ mu) / abs(u @ mv)
    print("u.M^-1 v = %.15e, v.M^-1 u = %.15e, relative difference %.2e, u.M^-1 u = %.3e" % (u @ mv, v @ mu, asym, u @ mu))
    assert asym <= 1e-12 and u @ mu > 0.0 and v @ mv > 0.0


# ------------------------------------------------------------------------------------------------ 5. same bits, capture
def test_two_setups_and_two_applications_give_the_same_bits(tb, setups):
    p, lv = setups("B", "off_coarse")
    dev2 = tb.MI355XDevice(0)                                               # a device of its own: a refused call must not disturb the shared one
    n = p["n"]
    pattern = tb.DeviceMesh(dev2, p["dhs"][-1]).pattern(p["sps"][-1])
    system = tb.BidomainSystem(pattern)
    system.set_matrices(*(dev2.to_device(a) for a in p["host"]), bref.DT, dev2.to_device(lv["flags"].astype(np.uint8)), lv["ground_diag"])
    mg = tb.BidomainMultigrid(system, p["gh"], DEGREE, RATIO).setup()
    first = [mg.level_blocks(l) for l in range(mg.n_levels)]
    lmax = [mg.lambda_max(l) for l in range(1, mg.n_levels)]
    mg.setup()
    for l in range(mg.n_levels):
        for a, b in zip(first[l], mg.level_blocks(l)):
            assert np.array_equal(a, b), "two set-ups differ on level %d" % l
        for a, b in zip(first[l], lv["mg"].level_blocks(l)):
            assert np.array_equal(a, b), "two hierarchies differ on level %d" % l
    assert lmax == [mg.lambda_max(l) for l in range(1, mg.n_levels)]
    r = dev2.to_device(np.random.default_rng(43).normal(size=2 * n))
    z1, z2, z3 = dev2.zeros(2 * n), dev2.zeros(2 * n), dev2.zeros(2 * n)
    mg.apply(r, z1)
    mg.apply(r, z2)
    assert np.array_equal(z1.to_host(), z2.to_host())
    graph = dev2.capture(lambda: mg.apply(r, z3))
    graph.launch()
    dev2.synchronize()
    assert np.array_equal(z1.to_host(), z3.to_host())
    graph.close()
    for call in (lambda: system.solve(r, z2, maxiter=5, precond=mg), mg.setup):
        with pytest.raises(tb.TBError) as e:
            dev2.capture(call)
        assert e.value.code == tb._lib.TB_ERR_BAD_ARG and "capture" in str(e.value)
    mg.apply(r, z2)                                                         # the stream is still usable
    assert np.array_equal(z1.to_host(), z2.to_host())
    mg.close()


# ------------------------------------------------------------------------------------------------ 6. the solve
@pytest.mark.parametrize("name,kind", CASES)
def test_solve_against_the_dense_solution(tb, device, setups, name, kind):
    """the right-hand side and the bound of test_bidomain_gpu.test_solve_against_the_dense_solution: ‖x − x*‖₂ ≤ (‖b − A x‖₂ + 4ε‖ |A||x| ‖₂)/λ_min(A)"""
    p, lv = setups(name, kind)
    n, A, system, mg = p["n"], lv["A"], lv["system"], lv["mg"]
    b = np.random.default_rng(12).uniform(-1.0, 1.0, 2 * n)
    b[n + lv["ground"]] = 0.0
    db = device.to_device(bref.interleave(b))
    runs = []
    for _ in range(2):
        dx = device.zeros(2 * n)
        its, res = system.solve(db, dx, rtol=1e-12, atol=0.0, maxiter=8 * n, precond=mg)
        runs.append((dx.to_host(), its, res))
    (x1, its, res), (x2, its2, res2) = runs
    assert np.array_equal(x1, x2) and (its, res) == (its2, res2)
    tol = C.c_double()
    tb.check(tb.lib().tb_solver_last_tolerance(p["pattern"].h, C.byref(tol)))
    dxj = device.zeros(2 * n)
    its_bj, _ = system.solve(db, dxj, rtol=1e-12, atol=0.0, maxiter=8 * n)
    cyc = ref.Cycle(lv["As"], lv["Ps"], lv["gs"], lv["lmax"], DEGREE, RATIO)
    _, its_ref = ref.pcg(A, b, cyc, 1e-12, 8 * n)
    x, xs = bref.deinterleave(x1), np.linalg.solve(A, b)
    err, bound = np.linalg.norm(x - xs), bref.error_bound(A, b, x)
    print("%s ground %s: %d iterations (NumPy PCG %d, block-Jacobi %d), reported |r| %.3e <= tolerance %.3e, |x - x*| %.3e <= bound %.3e" % (name, kind, its, its_ref, its_bj, res,
                                                                                                                                 tol.value, err, bound))
    assert res <= tol.value
    assert abs(tol.value - 1e-12 * np.linalg.norm(b)) <= 1e-12 * tol.value
    assert tb.solve_converged(p["pattern"], res)
    assert err <= bound
    assert np.all(x[n + lv["ground"]] == 0.0)
    assert its <= its_ref + 2                                                # the margin: rounding at the stopping look
    assert its < its_bj


# ------------------------------------------------------------------------------------------------ 7. the stage
def make_stage(tb, device, p, ground_vertices, **kw):
    one = tb.ConstantCoefficient(1.0)
    Di = tb.ConductivityToDiffusivityCoefficient(tb.ConstantCoefficient(bref.KAPPA_I), one, one)
    De = tb.ConductivityToDiffusivityCoefficient(tb.ConstantCoefficient(bref.KAPPA_E), one, one)
    return tb.BidomainBackwardEulerStage(strict_solver(tb, p["n"]), tb.PerColorAssemblyStrategy(device), p["dhs"][-1], Di, De, list(ground_vertices), pattern=p["sps"][-1], **kw)


def test_stage_with_multigrid_is_the_stage_without(tb, device, setups):
    p, _ = setups("B", "off_coarse")
    n, gh = p["n"], p["gh"]
    ground = ref.ground_nodes(gh, "off_coarse")
    mgs, bjs = make_stage(tb, device, p, ground, precond=tb.GMGPrecon(gh)), make_stage(tb, device, p, ground)
    assert mgs.multigrid.n_levels == 3 and bjs.multigrid is None
    phi0 = np.random.default_rng(44).uniform(-1.0, 1.0, n)
    pm, pj = device.to_device(phi0), device.to_device(phi0)
    sp = mgs.sp

    def dense(stage, dt):
        M, Ki, Ke = stage.M.A.to_host(), stage.Ki.A.to_host(), stage.Ke.A.to_host()
        return bref.block_matrix(sp.rowptr, sp.colidx, M, Ki, Ke, dt, stage.ground_dofs, stage.ground_diag(dt)), bref.dense_of_csr(sp.rowptr, sp.colidx, M)

    assert mgs.generation == 0
    mg = mgs.multigrid
    t, lam, old = 0.0, {}, None
    for step, dt in enumerate((0.1, 0.1, 0.05)):
        # both stages start every step from the same φₘ and the same initial guess φₑ, so the two solutions of one system are compared
        start = pm.to_host()
        pj.copy_from_host(start)
        bjs.phi_e.copy_from_host(mgs.phi_e.to_host())
        assert mgs.perform_step(pm, t, dt) and bjs.perform_step(pj, t, dt)
        assert mgs.generation == bjs.generation == (1 if step < 2 else 2) and mgs.dt_last == dt
        if dt not in lam:
            A, Md = dense(mgs, dt)
            lam[dt] = (A, Md, float(np.linalg.eigvalsh(A)[0]))
        A, Md, lmin = lam[dt]
        b = np.concatenate([Md @ start, np.zeros(n)])
        xm = np.concatenate([pm.to_host(), mgs.phi_e.to_host()])
        xj = np.concatenate([pj.to_host(), bjs.phi_e.to_host()])
        bound_m, bound_j = bref.error_bound(A, b, xm, lmin), bref.error_bound(A, b, xj, lmin)
        diff_m, diff_e = np.linalg.norm(xm[:n] - xj[:n]), np.linalg.norm(xm[n:] - xj[n:])
        print("step %d (dt %g): multigrid %d iterations, block-Jacobi %d, |phi_m difference| %.3e, |phi_e difference| %.3e <= %.3e + %.3e" % (step, dt, mgs.last_iters, bjs.last_iters,
                                                                                                                                 diff_m, diff_e, bound_m, bound_j))
        assert mgs.last_iters < bjs.last_iters and mgs.last_resnorm >= 0.0
        assert diff_m <= bound_m + bound_j and diff_e <= bound_m + bound_j
        if step == 0:
            old = mg.level_blocks(mg.n_levels - 2)
        elif step == 1:
            assert all(np.array_equal(a, c) for a, c in zip(old, mg.level_blocks(mg.n_levels - 2)))      # the same Δt: no new set-up
        t += dt
    # the operators of the new Δt: the first coarse level against the reference chain of the stage's own matrices at Δt = 0.05
    flags = np.zeros(n, dtype=bool)
    flags[mgs.ground_dofs] = True
    As, _, _ = ref.hierarchy(gh, mg.dhs, lam[0.05][0], flags)
    want, _ = ref.planes(As[-2], mg.sps[-2])
    got = mg.level_blocks(mg.n_levels - 2)
    scale = max(np.abs(w).max() for w in want)
    assert max(np.abs(a - w).max() for a, w in zip(got, want)) <= 1e-12 * scale
    assert np.abs(old[0] - got[0]).max() > 1e-3 * scale                                                 # … and not those of the old one


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_refusals(tb, device, setups):
    p, lv = setups("A", "vertex")
    n, gh, lib = p["n"], p["gh"], tb.lib()
    BAD, UNSUP = tb._lib.TB_ERR_BAD_ARG, tb._lib.TB_ERR_UNSUPPORTED
    flags = device.to_device(lv["flags"].astype(np.uint8))
    x, y = device.zeros(2 * n), device.zeros(2 * n)
    # the hierarchy's finest pattern is not the block system's pattern
    other = p["dhs"][-1].device_mesh(device).pattern(tb.allocate_matrix(p["dhs"][-1]))
    good, foreign_system = tb.BidomainMultigrid(tb.BidomainSystem(p["pattern"]), gh), tb.BidomainSystem(other)
    h = C.c_void_p()
    assert lib.tb_bidomain_mg_create(foreign_system.h, good.mg, C.byref(h)) == BAD and not h and b"finest pattern" in lib.tb_last_error_string()
    good.close()
    # setup before set_matrices; apply and solve before setup
    system = tb.BidomainSystem(p["pattern"])
    mg = tb.BidomainMultigrid(system, gh)
    assert lib.tb_bidomain_mg_setup(mg.h, 2, 4.0) == BAD and b"tb_bidomain_set_matrices" in lib.tb_last_error_string()
    system.set_matrices(*p["dev"], bref.DT, flags, lv["ground_diag"])
    assert lib.tb_bidomain_mg_apply(mg.h, x.ptr, y.ptr) == BAD and b"no numeric set-up" in lib.tb_last_error_string()
    it, res = C.c_int(), C.c_double()
    assert lib.tb_bidomain_mg_solve(mg.h, x.ptr, y.ptr, 1e-5, 0.0, 5, C.byref(it), C.byref(res)) == BAD and b"no numeric set-up" in lib.tb_last_error_string()
    for degree, ratio, fragment in ((0, 4.0, b"degree must be in 1..64"), (2, 1.0, b"interval_ratio must be a finite number above 1"),
                                    (2, float("nan"), b"interval_ratio must be a finite number above 1")):
        assert lib.tb_bidomain_mg_setup(mg.h, degree, ratio) == BAD and fragment in lib.tb_last_error_string()
    mg.setup()
    mg.apply(x, y)
    # … or after a later set_matrices without a new setup
    system.set_matrices(*p["dev"], 0.5 * bref.DT, flags, lv["ground_diag"])
    assert lib.tb_bidomain_mg_apply(mg.h, x.ptr, y.ptr) == BAD and b"after the latest set-up" in lib.tb_last_error_string()
    with pytest.raises(tb.TBError, match="after the latest set-up"):
        system.solve(x, y, precond=mg)
    mg.setup()
    # a NULL, aliased or misaligned vector
    assert lib.tb_bidomain_mg_apply(mg.h, None, y.ptr) == BAD and b"NULL argument" in lib.tb_last_error_string()
    assert lib.tb_bidomain_mg_apply(mg.h, x.ptr, x.ptr) == BAD and b"alias" in lib.tb_last_error_string()
    assert lib.tb_bidomain_mg_apply(mg.h, C.c_void_p(x.ptr.value + 8), y.ptr) == BAD and b"16-byte" in lib.tb_last_error_string()
    assert lib.tb_bidomain_mg_solve(mg.h, x.ptr, C.c_void_p(y.ptr.value + 8), 1e-5, 0.0, 5, C.byref(it), C.byref(res)) == BAD and b"16-byte" in lib.tb_last_error_string()
    with pytest.raises(ValueError, match="another block system"):
        lv["system"].solve(x, y, precond=mg)
    mg.close()
    # the coarsest level is too large: 9³ = 729 nodes
    big = tb.GridHierarchy(tb.generate_mesh(tb.Hexahedron, (8, 8, 8)), 1)
    dhb = tb.DofHandler(big.finest)
    with pytest.raises(tb.TBError, match="add a level") as e:
        tb.BidomainMultigrid(tb.BidomainSystem(dhb.device_mesh(device).pattern(tb.allocate_matrix(dhb))), big)
    assert e.value.code == UNSUP
    # the stage: what check_supported refuses, and the recipes out of scope
    D = tb.ConstantCoefficient(bref.KAPPA_I)
    args = (tb.BackwardEulerSolver(), tb.PerColorAssemblyStrategy(device))
    tet = tb.DofHandler(tb.generate_mesh(tb.Tetrahedron, (2, 2, 2)))
    with pytest.raises(NotImplementedError, match="hexahedral"):
        tb.BidomainBackwardEulerStage(*args, tet, D, D, [0], precond=tb.GMGPrecon(gh))
    with pytest.raises(NotImplementedError, match="first-order scalar fields only"):
        tb.BidomainBackwardEulerStage(*args, tb.DofHandler(gh.finest, tb.LagrangeCollection(2)), D, D, [0], precond=tb.GMGPrecon(gh))
    whole = p["dhs"][-1]
    part = tb.DofHandler(gh.finest, cell_dofs=whole.cell_dofs[:whole.cell_dofs.shape[0] // 2], ndofs=whole.ndofs)      # a handler over half of the cells
    with pytest.raises(NotImplementedError, match="subdomain dof handlers are out of scope"):
        tb.BidomainBackwardEulerStage(*args, part, D, D, [0], precond=tb.GMGPrecon(gh))
    foreign = tb.DofHandler(tb.generate_mesh(tb.Hexahedron, (3, 3, 3)))
    with pytest.raises(ValueError, match="finest grid"):
        tb.BidomainBackwardEulerStage(*args, foreign, D, D, [0], precond=tb.GMGPrecon(gh))
    for recipe in (tb.PMGPrecon(), tb.ChainedMGPrecon(tb.PMGPrecon(), tb.GMGPrecon(gh)), "jacobi"):
        with pytest.raises(NotImplementedError, match="out of scope"):
            tb.BidomainBackwardEulerStage(*args, p["dhs"][-1], D, D, [0], precond=recipe)
    for kw, fragment in ((dict(cycle="W"), "V-cycles only"), (dict(cycle="F"), "V-cycles only"), (dict(smoother="l1gs"), "Chebyshev-Jacobi smoother only")):
        with pytest.raises(NotImplementedError, match=fragment):
            tb.GMGPrecon(gh, **kw)


# ------------------------------------------------------------------------------------------------ 9. the example
def test_the_bidomain_multigrid_example_runs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "bidomain_multigrid.py"), "--nx", "3", "--refinements", "2", "--steps", "4"], capture_output=True,
                         text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads(out.stdout.strip().splitlines()[-1])
    assert d["all_converged"] and d["phi_m_range"][1] > 0.1 and d["phi_e_at_ground"] == 0.0
    assert 0 < d["cg_iterations_per_step"] < d["block_jacobi_iterations_per_step"]
    assert max(d["max_difference_to_block_jacobi"]) <= 1e-4
