"""The algebraic multigrid preconditioner of the bidomain block system on the device (csrc/tb_bidomain_amg.hip, BidomainAlgebraicMultigrid) against the
SciPy restatement of tests/bidomain_amg_reference.py: aggregates, P and the four planes level by level, bit identities, λmax, one V-cycle, symmetry, the
preconditioned solve, the stage, refusals and the example.  Meshes: a perturbed hexahedral box of 8³ cells (729 nodes: 11 full slices and a partial one, a
coarse level below 64 nodes), a tetrahedral box (4, 4, 4), each under three grounds (one vertex; an interior vertex and one more; a whole face), and one
hexahedral box of 16³ cells (4 913 nodes, a coarse level of a few hundred nodes with rows far wider than 27).  max_coarse = 32 throughout."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import amg_reference as aref
import bidomain_amg_reference as ref
import bidomain_reference as bref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_COARSE, DEGREE, RATIO, DT = 32, 2, 4.0, 0.1
KAPPA_I, KAPPA_E = np.diag([1.0, 0.2, 0.2]), np.diag([1.0, 0.5, 0.5])
MESHES = {"hex8": ("Hexahedron", 8, 0.1), "tet4": ("Tetrahedron", 4, 0.0), "hex16": ("Hexahedron", 16, 0.1)}
CASES = [(m, g) for m in ("hex8", "tet4") for g in ("vertex", "two", "face")] + [("hex16", "two")]


def ground_vertices(nel, kind):
    """vertex ids on the lattice of (nel + 1)³ nodes, x fastest"""
    m = nel + 1
    if kind == "vertex":
        return [0]
    if kind == "two":
        return [m ** 3 // 2, m ** 3 - 2]                                   # the centre of the box, and one more
    if kind == "face":
        return [int(v) for v in np.flatnonzero(np.arange(m ** 3) % m == 0)]  # x = 0
    raise KeyError(kind)


def relmax(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def coefficients(tb):
    one = tb.ConstantCoefficient(1.0)
    return (tb.ConductivityToDiffusivityCoefficient(tb.ConstantCoefficient(KAPPA_I), one, one),
            tb.ConductivityToDiffusivityCoefficient(tb.ConstantCoefficient(KAPPA_E), one, one))


def make_stage(tb, device, dh, sp, ground, n, **kw):
    Di, De = coefficients(tb)
    return tb.BidomainBackwardEulerStage(tb.BackwardEulerSolver(rtol=1e-12, atol=0.0, maxiter=8 * n), tb.PerColorAssemblyStrategy(device), dh, Di, De, list(ground), pattern=sp, **kw)


class Case:
    """one system: M, Kᵢ, Kₑ assembled on the device and downloaded, the block system with its hierarchy after one set-up, a plain scalar hierarchy on the
    same a₂₂ array, and the restatement fed the device's λ of both kinds — computed once, never written"""

    def __init__(self, tb, device, mesh, kind):
        cell, nel, perturb = MESHES[mesh]
        self.mesh, self.kind, self.nel = mesh, kind, nel
        grid = tb.generate_mesh(getattr(tb, cell), (nel, nel, nel), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), perturb=perturb)
        self.dh = dh = tb.DofHandler(grid)
        self.sp = sp = tb.allocate_matrix(dh)
        self.n = n = dh.ndofs
        self.stage = stage = make_stage(tb, device, dh, sp, ground_vertices(nel, kind), n)       # assembles; its block-Jacobi solve is never run here
        self.pattern, self.dev = stage.M.pattern, (stage.M.A, stage.Ki.A, stage.Ke.A)
        self.host = tuple(a.to_host() for a in self.dev)
        self.ground = stage.ground_dofs
        self.gd = stage.ground_diag(DT)
        self.dflags = stage.ground_flags
        self.system = tb.BidomainSystem(self.pattern)
        self.system.set_matrices(*self.dev, DT, self.dflags, self.gd)
        self.mg = tb.BidomainAlgebraicMultigrid(self.system, 0.25, DEGREE, RATIO, MAX_COARSE).setup()
        self.nl = self.mg.n_levels
        self.lmax = [self.mg.lambda_max(l) for l in range(self.nl - 1)]
        self.A, self.flags, _ = ref.block_system(sp.rowptr, sp.colidx, *self.host, DT, self.ground, self.gd)
        self.pat0 = (sp.rowptr.astype(np.int64), sp.colidx.astype(np.int32))
        # the scalar hierarchy of tb_amg on the same a₂₂ array: its λ(D⁻¹A) per level is what the restatement's P is smoothed with
        self.da22 = device.to_device(self.mg.level_blocks(0)[3])
        self.plain = tb.amg.AlgebraicHierarchy(self.pattern, 0.25, DEGREE, RATIO, MAX_COARSE).setup(self.da22)
        self.lam = [self.plain.lambda_max(l) for l in range(self.plain.n_levels - 1)]
        self.levels = ref.hierarchy(self.A, self.pat0, self.lam, 0.25, MAX_COARSE)
        self.cycle = ref.Cycle(self.levels, self.flags, self.lmax, DEGREE, RATIO)
        self.b = np.random.default_rng(17).normal(size=2 * n)
        self.b[n + self.ground] = 0.0


_cases = {}


@pytest.fixture(params=CASES, ids=["%s-%s" % c for c in CASES])
def case(request, tb, device):
    if request.param not in _cases:
        _cases[request.param] = Case(tb, device, *request.param)
    return _cases[request.param]


def get_case(tb, device, mesh, kind):
    if (mesh, kind) not in _cases:
        _cases[mesh, kind] = Case(tb, device, mesh, kind)
    return _cases[mesh, kind]


def apply(case, device, r_blocked):
    z = case.mg.apply(device.to_device(bref.interleave(r_blocked)), device.zeros(2 * case.n)).to_host()
    return bref.deinterleave(z)


# ------------------------------------------------------------------------------------------------ 1. set-up
def test_the_fine_matrix_is_the_reference_block_matrix(tb, device):
    c = get_case(tb, device, "tet4", "two")
    sp = c.sp
    dense = bref.block_matrix(sp.rowptr, sp.colidx, *c.host, DT, c.ground, c.gd)
    assert np.abs(c.A.toarray() - dense).max() == 0.0
    assert bref.asymmetry(dense) <= bref.EPS


def test_aggregates_patterns_prolongators_and_planes_are_the_restatements(case):
    mg, levels = case.mg, case.levels
    sizes = [mg.level_size(l) for l in range(case.nl)]
    print("%s ground %s: levels (nodes, non-zeros, aggregates) %s" % (case.mesh, case.kind, sizes))
    assert case.nl == len(levels) == case.plain.n_levels and case.nl >= 2
    assert sizes[-1][0] <= MAX_COARSE and sizes[-1][2] == 0
    if case.mesh == "hex8":
        assert sizes[1][0] < 64
    if case.mesh == "hex16":
        assert sizes[1][0] > 128 and np.diff(mg.level_pattern(1)[0]).max() > 27 + 8
    for l in range(case.nl):
        ptr, col = mg.level_pattern(l)
        assert np.array_equal(ptr, levels[l]["pattern"][0]) and np.array_equal(col, levels[l]["pattern"][1]), "pattern of level %d" % l
        want, got = ref.planes_of(levels[l]["A"], levels[l]["pattern"]), mg.level_blocks(l)
        scale = max(np.abs(w).max() for w in want)
        errs = [np.abs(a - w).max() / scale for a, w in zip(got, want)]
        msg = "%s ground %s level %d: max |plane - restatement| / max |entry| = %s" % (case.mesh, case.kind, l, ", ".join("%.2e" % e for e in errs))
        assert max(errs) <= 1e-13, msg
        assert np.array_equal(got[2], got[1]) or l == 0                                    # a₂₁ is bitwise a₁₂ below the finest level
        if l == 0:
            assert all(np.array_equal(a, w) for a, w in zip(got, want))                     # the finest planes: the block system's, bit for bit
        # the φₑφₑ plane is bitwise the level matrix of the plain scalar hierarchy on the same a₂₂ array
        assert np.array_equal(got[3], case.plain.level_matrix(l).data), "a22 of level %d" % l
        if l < case.nl - 1:
            margin = aref.strength_margin(levels[l]["a22"], None, 0.25)
            assert margin > 1e-9, "a strength tie on level %d: the comparison below would be of roundings" % l
            assert np.array_equal(mg.aggregates(l), levels[l]["agg"]), l
            assert sizes[l][2] == levels[l]["plan"]["na"] == sizes[l + 1][0]
            P, wantP = mg.prolongator(l), levels[l]["P"]
            assert np.array_equal(P.indptr, wantP.indptr) and np.array_equal(P.indices, wantP.indices), "pattern of P_%d" % l
            eP = relmax(P.data, wantP.data)
            print(msg + "  P %.2e" % eP)
            assert eP <= 1e-13
            assert np.array_equal(P.data, case.plain.prolongator(l).data)
    assert (mg.aggregates(0)[case.ground] == -1).all()                                       # grounded nodes are outside every aggregate …
    assert np.diff(mg.prolongator(0).indptr)[case.ground].max() == 0                        # … and their rows of P are empty


def test_lambda_max_is_no_less_than_the_exact_eigenvalue(case):
    stars = ref.lambda_stars(case.levels)
    for l, star in enumerate(stars):
        print("%s ground %s level %d: lambda* %.12e, device %.12e (ratio %.6f)" % (case.mesh, case.kind, l, star, case.lmax[l], case.lmax[l] / star))
        assert star <= case.lmax[l] <= 1.05 * star * (1.0 + 1e-12)


# ------------------------------------------------------------------------------------------------ 2. the cycle
def test_cycle_is_the_restatements_cycle(case, device):
    """one cycle against the restatement fed the device's λmax of both kinds: 1e-12 relative to max |z|"""
    z, want = apply(case, device, case.b), case.cycle(case.b)
    err = relmax(z, want)
    print("%s ground %s: one V-cycle, max |z - z_ref| / max |z_ref| = %.3e" % (case.mesh, case.kind, err))
    assert err <= 1e-12
    assert np.all(z[case.n + case.ground] == 0.0)


def test_cycle_is_symmetric_positive_and_zero_at_the_ground(case, device):
    rng = np.random.default_rng(42)
    u, v = rng.normal(size=2 * case.n), rng.normal(size=2 * case.n)                          # non-zero at the grounded φₑ as well
    mu, mv = apply(case, device, u), apply(case, device, v)
    asym = abs(u @ mv - v @ mu) / abs(u @ mv)
    print("%s ground %s: u.M^-1 v = %.15e, v.M^-1 u = %.15e, relative difference %.2e, u.M^-1 u = %.3e" % (case.mesh, case.kind, u @ mv, v @ mu, asym, u @ mu))
    assert asym <= 1e-12 and u @ mu > 0.0 and v @ mv > 0.0
    assert np.all(mu[case.n + case.ground] == 0.0) and np.all(mv[case.n + case.ground] == 0.0)


# ------------------------------------------------------------------------------------------------ 3. same bits
@pytest.mark.parametrize("mesh,kind", [("hex8", "face"), ("tet4", "two")])
def test_same_bits_across_setups_replan_applications_and_a_capture(tb, device, mesh, kind):
    c = get_case(tb, device, mesh, kind)
    dev2 = tb.MI355XDevice(0)                                                # a device of its own: a refused call must not disturb the shared one
    n = c.n
    pattern = tb.DeviceMesh(dev2, c.dh).pattern(c.sp)
    system = tb.BidomainSystem(pattern)
    system.set_matrices(*(dev2.to_device(a) for a in c.host), DT, dev2.to_device(c.flags.astype(np.uint8)), c.gd)
    mg = tb.BidomainAlgebraicMultigrid(system, 0.25, DEGREE, RATIO, MAX_COARSE).setup()

    def snapshot():
        return ([mg.level_blocks(l) for l in range(mg.n_levels)], [mg.prolongator(l).data for l in range(mg.n_levels - 1)],
                [mg.lambda_max(l) for l in range(mg.n_levels - 1)], [mg.aggregates(l) for l in range(mg.n_levels - 1)])

    def same(a, b):
        return (all(np.array_equal(x, y) for la, lb in zip(a[0], b[0]) for x, y in zip(la, lb)) and all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))
                and a[2] == b[2] and all(np.array_equal(x, y) for x, y in zip(a[3], b[3])))

    first = snapshot()
    assert same(first, ([c.mg.level_blocks(l) for l in range(c.nl)], [c.mg.prolongator(l).data for l in range(c.nl - 1)], c.lmax,
                        [c.mg.aggregates(l) for l in range(c.nl - 1)])), "two hierarchies differ"
    r = dev2.to_device(np.random.default_rng(43).normal(size=2 * n))
    z1, z2, z3 = dev2.zeros(2 * n), dev2.zeros(2 * n), dev2.zeros(2 * n)
    mg.apply(r, z1)
    planned = mg.n_levels - 1                                               # one host aggregation per level with a level below
    assert (mg.setups, mg.aggregations) == (1, planned)
    mg.setup()
    assert (mg.setups, mg.aggregations) == (2, planned) and same(first, snapshot()), "two set-ups differ"
    mg.replan().setup()
    assert (mg.setups, mg.aggregations) == (3, 2 * planned) and same(first, snapshot()), "replan + set-up differs"
    mg.apply(r, z2)
    assert np.array_equal(z1.to_host(), z2.to_host()) and np.abs(z1.to_host()).max() > 0.0
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


def test_doubled_matrices_double_every_plane(tb, device):
    """M, Kᵢ, Kₑ and ground_diag × 2: every product and sum of the set-up scales exactly, the plan stays, D⁻¹A and with it P keep their bits"""
    c = get_case(tb, device, "hex8", "two")
    system = tb.BidomainSystem(c.pattern)
    system.set_matrices(*(device.to_device(2.0 * a) for a in c.host), DT, c.dflags, 2.0 * c.gd)
    mg = tb.BidomainAlgebraicMultigrid(system, 0.25, DEGREE, RATIO, MAX_COARSE).setup()
    assert mg.n_levels == c.nl
    for l in range(c.nl):
        for a, w in zip(mg.level_blocks(l), c.mg.level_blocks(l)):
            assert np.array_equal(a, 2.0 * w), l
        if l < c.nl - 1:
            assert np.array_equal(mg.aggregates(l), c.mg.aggregates(l)) and np.array_equal(mg.prolongator(l).data, c.mg.prolongator(l).data)
    mg.close()


def test_fused_products_are_bitwise_the_scalar_product_chain(case):
    """every plane of every coarse level — a₁₁ and a₁₂ included — is bit for bit what three launch pairs of the scalar hierarchy's own product kernel
    (k_amg_spgemm, unchanged) give on the same planes, plans and P; and the fused pair gives them again"""
    mg = case.mg
    for l in range(case.nl - 1):
        before = mg.level_blocks(l + 1)
        assert all(np.abs(a).max() > 0.0 for a in before)
        mg.products(l, False)
        scalar = mg.level_blocks(l + 1)
        mg.products(l, True)
        fused = mg.level_blocks(l + 1)
        for q, name in enumerate(("a11", "a12", "a21", "a22")):
            assert np.array_equal(scalar[q], before[q]), "%s of level %d: three scalar launch pairs differ from the set-up's fused pair" % (name, l + 1)
            assert np.array_equal(fused[q], before[q]), "%s of level %d: the fused pair differs from itself" % (name, l + 1)


# ------------------------------------------------------------------------------------------------ 4. the solve
def test_pcg_count_is_the_restatements_and_below_block_jacobi(tb, case, device):
    n, system = case.n, case.system
    db = device.to_device(bref.interleave(case.b))
    runs = []
    for _ in range(2):
        dx = device.zeros(2 * n)
        its, res = system.solve(db, dx, rtol=1e-8, atol=0.0, maxiter=500, precond=case.mg)
        runs.append((dx.to_host(), its, res))
    (x1, its, res), (x2, its2, res2) = runs
    tol = C.c_double()
    tb.check(tb.lib().tb_solver_last_tolerance(case.pattern.h, C.byref(tol)))
    xj = device.zeros(2 * n)
    its_bj, _ = system.solve(db, xj, rtol=1e-8, atol=0.0, maxiter=5000)
    xr, its_ref = ref.pcg(case.A, case.b, case.cycle, rtol=1e-8)
    x = bref.deinterleave(x1)
    true_res = np.linalg.norm(case.b - case.A @ x)
    print("%s ground %s: %d iterations (restatement %d, block-Jacobi %d), reported |r| %.3e <= tolerance %.3e, true %.3e" % (case.mesh, case.kind, its, its_ref, its_bj, res,
                                                                                                                     tol.value, true_res))
    assert (its, res) == (its2, res2)
    if n <= 16000 // 2:
        assert np.array_equal(x1, x2)                                        # every sum of the solve is ordered up to 64 workgroups
    assert res <= tol.value and abs(tol.value - 1e-8 * np.linalg.norm(case.b)) <= 1e-12 * tol.value
    assert tb.solve_converged(case.pattern, res)
    assert true_res <= 1.01e-8 * np.linalg.norm(case.b)
    assert np.all(x[n + case.ground] == 0.0)
    assert relmax(x, xr) <= 1e-6
    assert its == its_ref
    assert its < its_bj


# ------------------------------------------------------------------------------------------------ 5. the stage
def test_stage_with_the_algebraic_cycle_is_the_stage_without(tb, device):
    c = get_case(tb, device, "tet4", "two")
    n, sp = c.n, c.sp
    ground = ground_vertices(c.nel, "two")
    mgs = make_stage(tb, device, c.dh, sp, ground, n, precond=tb.BidomainAMGPrecon(max_coarse=MAX_COARSE))
    bjs = make_stage(tb, device, c.dh, sp, ground, n)
    mg = mgs.multigrid
    assert isinstance(mg, tb.BidomainAlgebraicMultigrid) and bjs.multigrid is None and (mg.setups, mg.aggregations) == (0, 0)
    phi0 = np.random.default_rng(44).uniform(-1.0, 1.0, n)
    pm, pj = device.to_device(phi0), device.to_device(phi0)
    t, lam, agg, old = 0.0, {}, None, None
    for step, dt in enumerate((0.1, 0.1, 0.05)):
        start = pm.to_host()
        pj.copy_from_host(start)
        bjs.phi_e.copy_from_host(mgs.phi_e.to_host())
        assert mgs.perform_step(pm, t, dt) and bjs.perform_step(pj, t, dt)
        assert mgs.generation == bjs.generation == (1 if step < 2 else 2)
        # the library's own counts: a new Δt is exactly one set-up more and no host aggregation more
        assert (mg.setups, mg.aggregations) == ((1, mg.n_levels - 1) if step < 2 else (2, mg.n_levels - 1))
        if dt not in lam:
            M, Ki, Ke = mgs.M.A.to_host(), mgs.Ki.A.to_host(), mgs.Ke.A.to_host()
            A = bref.block_matrix(sp.rowptr, sp.colidx, M, Ki, Ke, dt, mgs.ground_dofs, mgs.ground_diag(dt))
            lam[dt] = (A, bref.dense_of_csr(sp.rowptr, sp.colidx, M), float(np.linalg.eigvalsh(A)[0]))
        A, Md, lmin = lam[dt]
        b = np.concatenate([Md @ start, np.zeros(n)])
        xm = np.concatenate([pm.to_host(), mgs.phi_e.to_host()])
        xj = np.concatenate([pj.to_host(), bjs.phi_e.to_host()])
        bound_m, bound_j = bref.error_bound(A, b, xm, lmin), bref.error_bound(A, b, xj, lmin)
        diff_m, diff_e = np.linalg.norm(xm[:n] - xj[:n]), np.linalg.norm(xm[n:] - xj[n:])
        print("step %d (dt %g): AMG %d iterations, block-Jacobi %d, |phi_m difference| %.3e, |phi_e difference| %.3e <= %.3e + %.3e" % (step, dt, mgs.last_iters, bjs.last_iters, diff_m,
                                                                                                                          diff_e, bound_m, bound_j))
        assert mgs.last_iters < bjs.last_iters
        assert diff_m <= bound_m + bound_j and diff_e <= bound_m + bound_j
        if step == 0:
            agg, old = mg.aggregates(0), mg.level_blocks(1)
        elif step == 1:
            assert all(np.array_equal(a, w) for a, w in zip(old, mg.level_blocks(1)))        # the same Δt: no new set-up
        t += dt
    assert np.array_equal(agg, mg.aggregates(0))
    assert np.abs(old[0] - mg.level_blocks(1)[0]).max() > 1e-3 * np.abs(old[0]).max()       # the operators are those of the new Δt


# ------------------------------------------------------------------------------------------------ 6. refusals
def test_refusals(tb, device):
    c = get_case(tb, device, "hex8", "vertex")
    n, lib = c.n, tb.lib()
    BAD, UNSUP = tb._lib.TB_ERR_BAD_ARG, tb._lib.TB_ERR_UNSUPPORTED
    x, y = device.zeros(2 * n), device.zeros(2 * n)
    it, res = C.c_int(), C.c_double()
    system = tb.BidomainSystem(c.pattern)
    # the recipe's arguments
    h = C.c_void_p()
    assert lib.tb_bidomain_amg_create(system.h, 0.25, 513, 16, C.byref(h)) == UNSUP and not h and b"at most 512 nodes" in lib.tb_last_error_string()
    for theta, mc, ml, fragment in ((1.5, 32, 16, b"theta must be in 0..1"), (0.25, 0, 16, b"max_coarse must be positive"), (0.25, 32, 0, b"max_levels must be in 1..64")):
        assert lib.tb_bidomain_amg_create(system.h, theta, mc, ml, C.byref(h)) == BAD and fragment in lib.tb_last_error_string()
    with pytest.raises(tb.TBError, match="at most 512 nodes"):
        tb.BidomainAlgebraicMultigrid(system, max_coarse=1024)
    for kw, fragment in ((dict(cycle="W"), "V-cycles only"), (dict(cycle="F"), "V-cycles only"), (dict(smoother="l1gs"), "Chebyshev smoother")):
        with pytest.raises(NotImplementedError, match=fragment):
            tb.BidomainAMGPrecon(**kw)
    # set-up before set_matrices; apply, solve and the inspectors before set-up
    mg = tb.BidomainAlgebraicMultigrid(system, max_coarse=MAX_COARSE)
    assert lib.tb_bidomain_amg_setup(mg.h, 2, 4.0) == BAD and b"tb_bidomain_set_matrices" in lib.tb_last_error_string()
    system.set_matrices(*c.dev, DT, c.dflags, c.gd)
    assert lib.tb_bidomain_amg_apply(mg.h, x.ptr, y.ptr) == BAD and b"no numeric set-up" in lib.tb_last_error_string()
    assert lib.tb_bidomain_amg_solve(mg.h, x.ptr, y.ptr, 1e-5, 0.0, 5, C.byref(it), C.byref(res)) == BAD and b"no numeric set-up" in lib.tb_last_error_string()
    with pytest.raises(tb.TBError, match="no numeric set-up"):
        mg.n_levels
    assert lib.tb_bidomain_amg_products(mg.h, 0, 1) == BAD and b"no numeric set-up" in lib.tb_last_error_string()
    assert (mg.setups, mg.aggregations) == (0, 0)                                           # the counts need no set-up, and a refused set-up counts nothing
    for degree, ratio, fragment in ((0, 4.0, b"degree must be in 1..64"), (2, 1.0, b"interval_ratio must be a finite number above 1")):
        assert lib.tb_bidomain_amg_setup(mg.h, degree, ratio) == BAD and fragment in lib.tb_last_error_string()
    mg.setup()
    mg.apply(x, y)
    # … or after a later set_matrices without a new set-up
    system.set_matrices(*c.dev, 0.5 * DT, c.dflags, c.gd)
    assert lib.tb_bidomain_amg_apply(mg.h, x.ptr, y.ptr) == BAD and b"after the latest set-up" in lib.tb_last_error_string()
    with pytest.raises(tb.TBError, match="after the latest set-up"):
        system.solve(x, y, precond=mg)
    with pytest.raises(tb.TBError, match="after the latest set-up"):
        mg.level_blocks(0)
    for fused in (0, 1):
        assert lib.tb_bidomain_amg_products(mg.h, 0, fused) == BAD and b"after the latest set-up" in lib.tb_last_error_string()
    mg.setup()
    # a NULL, aliased or misaligned vector; a level that does not exist; the last level has no smoother
    assert lib.tb_bidomain_amg_apply(mg.h, None, y.ptr) == BAD and b"NULL argument" in lib.tb_last_error_string()
    assert lib.tb_bidomain_amg_apply(mg.h, x.ptr, x.ptr) == BAD and b"alias" in lib.tb_last_error_string()
    assert lib.tb_bidomain_amg_apply(mg.h, C.c_void_p(x.ptr.value + 8), y.ptr) == BAD and b"16-byte" in lib.tb_last_error_string()
    assert lib.tb_bidomain_amg_solve(mg.h, x.ptr, C.c_void_p(y.ptr.value + 8), 1e-5, 0.0, 5, C.byref(it), C.byref(res)) == BAD and b"16-byte" in lib.tb_last_error_string()
    assert lib.tb_bidomain_amg_solve(mg.h, x.ptr, x.ptr, 1e-5, 0.0, 5, C.byref(it), C.byref(res)) == BAD and b"alias" in lib.tb_last_error_string()
    with pytest.raises(tb.TBError, match="level %d of %d" % (mg.n_levels, mg.n_levels)):
        mg.level_size(mg.n_levels)
    with pytest.raises(tb.TBError, match="last one"):
        mg.lambda_max(mg.n_levels - 1)
    for fused in (False, True):
        with pytest.raises(tb.TBError, match="no level below"):
            mg.products(mg.n_levels - 1, fused)
        with pytest.raises(tb.TBError, match="level -1 of %d" % mg.n_levels):
            mg.products(-1, fused)
    assert lib.tb_bidomain_amg_products(None, 0, 1) == BAD and lib.tb_bidomain_amg_counts(None, None, None) == BAD
    # a hierarchy of another system
    with pytest.raises(ValueError, match="another block system"):
        c.system.solve(x, y, precond=mg)
    with pytest.raises(TypeError):
        c.system.solve(x, y, precond=c.plain)
    mg.close()
    # a last level too large, the reason named: one level on 729 nodes, and max_levels = 2 on the 16³ box wherever its first coarse level exceeds 512 nodes
    one = tb.BidomainAlgebraicMultigrid(system, max_coarse=MAX_COARSE, max_levels=1)
    with pytest.raises(tb.TBError, match="tb_bidomain_amg_setup: the last level .0. has 729 nodes.*at most 512.*max_levels was reached") as e:
        one.setup()
    assert e.value.code == UNSUP
    one.close()
    big = get_case(tb, device, "hex16", "two")
    two = tb.BidomainAlgebraicMultigrid(big.system, max_coarse=MAX_COARSE, max_levels=2)
    n1 = big.mg.level_size(1)[0]
    if n1 > 512:
        with pytest.raises(tb.TBError, match="max_levels was reached") as e:
            two.setup()
        assert e.value.code == UNSUP
    else:
        assert two.setup().n_levels == 2 and two.level_size(1)[0] == n1                     # (a few hundred nodes: the dense inverse takes them)
    two.close()
    # the stage: the scalar recipe stays refused, second-order fields and subdomain handlers too
    D = tb.ConstantCoefficient(KAPPA_I)
    args = (tb.BackwardEulerSolver(), tb.PerColorAssemblyStrategy(device))
    with pytest.raises(NotImplementedError, match="out of scope.*BidomainAMGPrecon"):
        tb.BidomainBackwardEulerStage(*args, c.dh, D, D, [0], precond=tb.AMGPrecon())
    with pytest.raises(NotImplementedError, match="first-order scalar fields only"):
        tb.BidomainBackwardEulerStage(*args, tb.DofHandler(c.dh.grid, tb.LagrangeCollection(2)), D, D, [0], precond=tb.BidomainAMGPrecon())
    part = tb.DofHandler(c.dh.grid, cell_dofs=c.dh.cell_dofs[:c.dh.cell_dofs.shape[0] // 2], ndofs=c.dh.ndofs)
    with pytest.raises(NotImplementedError, match="subdomain dof handlers are out of scope"):
        tb.BidomainBackwardEulerStage(*args, part, D, D, [0], precond=tb.BidomainAMGPrecon())


# ------------------------------------------------------------------------------------------------ 7. the example
def test_the_tetrahedral_bidomain_example_runs():
    """examples/bidomain_amg_tet.py: a bidomain wave on a tetrahedral box at toy size — the AMG takes fewer iterations than block-Jacobi, same fields"""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "bidomain_amg_tet.py")], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    rec = json.loads(out.stdout.strip().splitlines()[-1])
    print(rec)
    assert len(rec["levels"]) >= 2 and rec["levels"][-1] <= 64
    assert max(rec["iterations_amg"]) < min(rec["iterations_block_jacobi"])
    assert rec["all_converged"] and rec["phi_m_range"][1] > 0.1 and rec["phi_e_at_ground"] == 0.0
    assert rec["max_difference_phi_m"] <= 1e-4 and rec["max_difference_phi_e"] <= 1e-4
