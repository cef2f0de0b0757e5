"""The geometric multigrid on the device (tb_multigrid.hip) against the numpy restatement of tests/multigrid_reference.py: transfers, Galerkin level
matrices, one V-cycle, the preconditioned solve on the diffusion problem of the issue's CPU restatement (tensor diag(9, 4, 4), Dirichlet on x = 0,
levels down to 2³ cells) and the Newton solve of a clamped Guccione bar."""
import ctypes as C

import numpy as np
import pytest

import multigrid_reference as ref

pytestmark = pytest.mark.gpu


def box(tb, nel, perturb=0.0):
    return tb.generate_mesh(tb.Hexahedron, nel, (0, 0, 0), (1, 1, 1), perturb=perturb)


def face_dofs(dh, axis=0, value=0.0):
    """every dof of the nodes on the face x_axis = value"""
    return ref.node_dofs(dh)[np.abs(dh.grid.xyz[:, axis] - value) < 1e-12].ravel()


def spd_values(sp):
    """a symmetric, strictly diagonally dominant matrix on the pattern: a_ij = −(0.1 + h(min, max)) off the diagonal"""
    n = len(sp.rowptr) - 1
    rows = np.repeat(np.arange(n), np.diff(sp.rowptr))
    cols = sp.colidx.astype(np.int64)
    lo, hi = np.minimum(rows, cols), np.maximum(rows, cols)
    v = -(0.1 + ((lo * 7919 + hi * 104729) % 1000) / 1000.0)
    v[rows == cols] = 0.0
    rowsum = np.zeros(n)
    np.add.at(rowsum, rows, np.abs(v))
    v[rows == cols] = rowsum + 1.0
    return v


def diffusion_problem(tb, device, gh, tensor=(9.0, 4.0, 4.0), mass_dt=None):
    """−K (or M − Δt·K with mass_dt) of the Q1 diffusion operator on the finest grid → (dh, sp, pattern, values on the host)"""
    dh = tb.DofHandler(gh.grids[-1])
    sp = tb.allocate_matrix(dh)
    st = tb.PatchAssemblyStrategy(device)
    D = tb.ConductivityToDiffusivityCoefficient(tb.ConstantCoefficient(np.diag(tensor)), tb.ConstantCoefficient(1.0), tb.ConstantCoefficient(1.0))
    K = tb.update_operator(tb.setup_operator(st, tb.BilinearDiffusionIntegrator(D), dh, sp), 0.0)
    vals = -K.A.to_host()
    if mass_dt is not None:
        M = tb.update_operator(tb.setup_operator(st, tb.BilinearMassIntegrator(tb.ConstantCoefficient(1.0)), dh, sp), 0.0)
        vals = M.A.to_host() + mass_dt * vals
    return dh, sp, K.pattern, vals


def eliminated(tb, device, pattern, vals, ch):
    """the matrix as apply_zero leaves it, on the device"""
    dA = device.to_device(vals)
    if ch is not None:
        tb.apply_zero(dA, None, ch, pattern=pattern)
    return dA


def flags_of(dh, ch):
    f = np.zeros(dh.ndofs, dtype=bool)
    if ch is not None:
        f[ch.prescribed_dofs] = True
    return f


def relerr(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


# ------------------------------------------------------------------------------------------------ transfers
@pytest.mark.parametrize("prescribed", [False, True])
@pytest.mark.parametrize("ncomp", [1, 3])
def test_transfers_are_P_and_its_transpose(tb, device, ncomp, prescribed):
    gh = tb.GridHierarchy(box(tb, (3, 2, 2)), 2)
    dh = tb.DofHandler(gh.grids[-1], tb.LagrangeCollection(1, ncomp))
    sp = tb.allocate_matrix(dh)
    pattern = dh.device_mesh(device).pattern(sp)
    ch = tb.ConstraintHandler(dh, face_dofs(dh)) if prescribed else None
    mg = tb.MultigridHierarchy(pattern, gh, ch=ch)
    mg.setup(eliminated(tb, device, pattern, spd_values(sp), ch))
    _, Ps, _ = ref.hierarchy(gh, mg.dhs, np.zeros((dh.ndofs, dh.ndofs)), flags_of(dh, ch))
    rng = np.random.default_rng(3)
    for l in (1, 2):
        P = Ps[l]
        x, y = rng.normal(size=P.shape[1]), rng.normal(size=P.shape[0])
        px = mg.prolong(l, device.to_device(x), device.zeros(P.shape[0])).to_host()
        rty = mg.restrict(l, device.to_device(y), device.zeros(P.shape[1])).to_host()
        e1, e2 = relerr(px, P @ x), relerr(rty, P.T @ y)
        adj = abs(px @ y - x @ rty) / abs(px @ y)
        print("level %d (%d -> %d dofs): prolong %.2e restrict %.2e adjoint %.2e" % (l, P.shape[1], P.shape[0], e1, e2, adj))
        assert e1 <= 1e-14 and e2 <= 1e-14 and adj <= 1e-13


# ------------------------------------------------------------------------------------------------ Galerkin products
def check_levels(tb, device, gh, dh, pattern, vals, ch):
    mg = tb.MultigridHierarchy(pattern, gh, ch=ch)
    dA = eliminated(tb, device, pattern, vals, ch)
    mg.setup(dA)
    first = [mg.level_matrix(l) for l in range(mg.n_levels)]
    mg.setup(dA)
    As, _, _ = ref.hierarchy(gh, mg.dhs, ref.csr_to_dense(pattern.sp, dA.to_host()), flags_of(dh, ch))
    for l in range(mg.n_levels):
        assert np.array_equal(first[l], mg.level_matrix(l)), "two setups differ on level %d" % l
        want = ref.dense_to_csr(mg.sps[l], As[l])
        assert np.array_equal(ref.csr_to_dense(mg.sps[l], want) != 0, As[l] != 0)         # nothing of PᵀAP lies outside the level's pattern
        err = np.abs(first[l] - want).max() / np.abs(want).max()
        print("level %d: max |A_c - PtAP| / max |PtAP| = %.3e" % (l, err))
        assert err <= 1e-12
    return mg


def test_galerkin_levels_of_diffusion_and_heat_matrices(tb, device):
    gh = tb.GridHierarchy(box(tb, (4, 3, 2), perturb=0.2), 1)
    dh, sp, pattern, K = diffusion_problem(tb, device, gh)
    check_levels(tb, device, gh, dh, pattern, K, tb.ConstraintHandler(dh, face_dofs(dh)))
    dh, sp, pattern, H = diffusion_problem(tb, device, gh, mass_dt=0.05)
    check_levels(tb, device, gh, dh, pattern, H, None)


def guccione_bar(tb, device, gh, facets=()):
    dh = tb.DofHandler(gh.grids[-1], tb.LagrangeCollection(1) ** 3)
    sp = tb.allocate_matrix(dh)
    ms = tb.ConstantCoefficient(tb.OrthotropicMicrostructure(*np.eye(3)))
    model = tb.QuasiStaticModel("d", tb.PK1Model(tb.Guccione1991PassiveModel(), ms), list(facets))
    op = tb.setup_operator(tb.ElementAssemblyStrategy(device), model, dh, sp)
    return dh, sp, op


def test_galerkin_levels_of_a_guccione_tangent(tb, device):
    gh = tb.GridHierarchy(box(tb, (4, 3, 2), perturb=0.2), 1)
    dh, sp, op = guccione_bar(tb, device, gh, [tb.RobinBC(0.3, "right")])
    ch = tb.ConstraintHandler(dh, face_dofs(dh))
    u = np.random.default_rng(5).uniform(-5e-3, 5e-3, dh.ndofs)
    u[ch.prescribed_dofs] = 0.0
    res = device.zeros(dh.ndofs)
    tb.update_linearization(op, device.to_device(u), 0.0, residual=res)
    check_levels(tb, device, gh, dh, op.pattern, op.J.to_host(), ch)


def test_galerkin_of_nested_affine_grids_is_the_coarse_assembly(tb, device):
    """constant coefficients on an unperturbed box: the Q1 spaces are nested and the quadrature is exact on affine cells, so PᵀAP is the matrix
    tb_assemble_matrix builds on the coarse grid"""
    gh = tb.GridHierarchy(box(tb, (3, 2, 2)), 1)
    dh, sp, pattern, H = diffusion_problem(tb, device, gh, mass_dt=0.05)
    mg = tb.MultigridHierarchy(pattern, gh).setup(device.to_device(H))
    st = tb.PatchAssemblyStrategy(device)
    D = tb.ConductivityToDiffusivityCoefficient(tb.ConstantCoefficient(np.diag([9.0, 4.0, 4.0])), tb.ConstantCoefficient(1.0), tb.ConstantCoefficient(1.0))
    Kc = tb.update_operator(tb.setup_operator(st, tb.BilinearDiffusionIntegrator(D), mg.dhs[0], mg.sps[0]), 0.0).A.to_host()
    Mc = tb.update_operator(tb.setup_operator(st, tb.BilinearMassIntegrator(tb.ConstantCoefficient(1.0)), mg.dhs[0], mg.sps[0]), 0.0).A.to_host()
    err = relerr(mg.level_matrix(0), Mc - 0.05 * Kc)
    print("Galerkin vs coarse assembly: %.3e" % err)
    assert err <= 1e-12


# ------------------------------------------------------------------------------------------------ cycle
@pytest.fixture(scope="module")
def cycle_problem(tb, device):
    gh = tb.GridHierarchy(box(tb, (2, 2, 2)), 2)
    dh, sp, pattern, K = diffusion_problem(tb, device, gh)
    ch = tb.ConstraintHandler(dh, face_dofs(dh))
    dA = eliminated(tb, device, pattern, K, ch)
    mg = tb.MultigridHierarchy(pattern, gh, ch=ch).setup(dA)
    As, Ps, pres = ref.hierarchy(gh, mg.dhs, ref.csr_to_dense(sp, dA.to_host()), flags_of(dh, ch))
    lmax = [None] + [mg.lambda_max(l) for l in range(1, mg.n_levels)]
    return mg, dh, ch, As, Ps, pres, lmax


def test_cycle_is_the_numpy_cycle(tb, device, cycle_problem):
    mg, dh, ch, As, Ps, pres, lmax = cycle_problem
    rng = np.random.default_rng(11)
    for k in range(2):
        r = rng.normal(size=dh.ndofs)
        z = mg.apply(device.to_device(r), device.zeros(dh.ndofs)).to_host()
        want = ref.vcycle(As, Ps, pres, lmax, mg.degree, mg.interval_ratio, r)
        err = relerr(z, want)
        print("rhs %d: lambda_max %s, max |z - z_numpy| / max |z_numpy| = %.3e" % (k, lmax[1:], err))
        assert err <= 1e-10
        assert np.all(z[ch.prescribed_dofs] == 0.0)               # r is non-zero there


def test_cycle_is_symmetric_and_positive(tb, device, cycle_problem):
    mg, dh = cycle_problem[0], cycle_problem[1]
    rng = np.random.default_rng(12)
    x, y = rng.normal(size=dh.ndofs), rng.normal(size=dh.ndofs)
    mx = mg.apply(device.to_device(x), device.zeros(dh.ndofs)).to_host()
    my = mg.apply(device.to_device(y), device.zeros(dh.ndofs)).to_host()
    asym = abs(x @ my - y @ mx) / abs(x @ my)
    print("x.M^-1 y = %.15e, y.M^-1 x = %.15e, relative difference %.2e" % (x @ my, y @ mx, asym))
    assert asym <= 1e-12 and x @ mx > 0.0


def test_cycle_replays_from_a_graph_with_the_same_bits(tb, device, cycle_problem):
    mg, dh = cycle_problem[0], cycle_problem[1]
    r = device.to_device(np.random.default_rng(13).normal(size=dh.ndofs))
    z1, z2 = device.zeros(dh.ndofs), device.zeros(dh.ndofs)
    mg.apply(r, z1)
    graph = device.capture(lambda: mg.apply(r, z2))
    graph.launch()
    device.synchronize()
    assert np.array_equal(z1.to_host(), z2.to_host())
    graph.close()


# ------------------------------------------------------------------------------------------------ solve
def test_preconditioned_solve_is_mesh_independent(tb, device):
    its, jac = {}, {}
    for refinements in (2, 3, 4):                                  # 8³, 16³, 32³ over a coarsest grid of 2³ cells
        gh = tb.GridHierarchy(box(tb, (2, 2, 2)), refinements)
        dh, sp, pattern, K = diffusion_problem(tb, device, gh)
        ch = tb.ConstraintHandler(dh, face_dofs(dh))
        dA = eliminated(tb, device, pattern, K, ch)
        b = np.random.default_rng(21).uniform(0.0, 1.0, dh.ndofs)
        b[ch.prescribed_dofs] = 0.0
        db = device.to_device(b)
        n = 2 ** (refinements + 1)
        x = device.zeros(dh.ndofs)
        its[n], res = tb.pcg_solve(pattern, dA, db, x, rtol=1e-10, atol=0.0, maxiter=200, precond=tb.GMGPrecon(gh).materialize(pattern, ch))
        assert tb.solve_converged(pattern, res), (n, its[n], res)
        xj = device.zeros(dh.ndofs)
        jac[n], resj = tb.pcg_solve(pattern, dA, db, xj, rtol=1e-10, atol=0.0, maxiter=5000, precond="jacobi")
        assert tb.solve_converged(pattern, resj)
        err = relerr(x.to_host(), xj.to_host())
        print("%d^3: multigrid PCG %d iterations, Jacobi PCG %d, solutions differ by %.2e" % (n, its[n], jac[n], err))
        assert err <= 1e-6
    assert its[32] <= its[8] + 2, its
    assert 4 * its[32] <= jac[32], (its, jac)


# ------------------------------------------------------------------------------------------------ Newton
@pytest.mark.parametrize("pressure", [False, True])
def test_newton_with_multigrid_reaches_the_chebyshev_solution(tb, device, pressure):
    gh = tb.GridHierarchy(tb.generate_mesh(tb.Hexahedron, (4, 1, 1), (0, 0, 0), (4.0, 1.0, 1.0)), 1)
    out = {}
    for name, precond in (("multigrid", tb.GMGPrecon(gh)), ("chebyshev", tb.ChebyshevPrecBuilder(8))):
        dh, sp, op = guccione_bar(tb, device, gh, [tb.ConstantPressureBC(0.001, "top")] if pressure else [])
        left, right = face_dofs(dh, 0, 0.0), ref.node_dofs(dh)[np.abs(dh.grid.xyz[:, 0] - 4.0) < 1e-12][:, 0]
        dofs = np.concatenate([left, right])
        ch = tb.ConstraintHandler(dh, dofs)
        order = {d: k for k, d in enumerate(ch.prescribed_dofs)}
        ch.values[[order[d] for d in right]] = 0.004                # the free end is pulled along the bar
        u = device.zeros(dh.ndofs)
        tb.apply(u, ch)
        solver = tb.NewtonRaphsonSolver(max_iter=20, tol=1e-9, inner_rtol=1e-8, inner_solver="cg", inner_precond=precond)
        assert tb.nlsolve(u, op, ch, solver), (name, solver.residual_norms, solver.linear_failure)
        out[name] = (u.to_host(), solver.iter, list(solver.linear_iters))
    print("pressure %s: Newton iterations %d / %d, linear iterations multigrid %s, Chebyshev(8) %s"
          % (pressure, out["multigrid"][1], out["chebyshev"][1], out["multigrid"][2], out["chebyshev"][2]))
    assert relerr(out["multigrid"][0], out["chebyshev"][0]) <= 1e-8
    assert out["multigrid"][1] == out["chebyshev"][1]


def test_the_ring_example_runs():
    """examples/multigrid_ring.py: the how-to at toy size converges with both preconditioners and reports the same Newton history length"""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "examples", "multigrid_ring.py")], capture_output=True, text=True, timeout=300, cwd=root)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-1500:])
    line = json.loads(out.stdout.strip().splitlines()[-1])
    print(out.stdout)
    assert line["converged"] and line["levels"] == 2
    assert line["multigrid"]["newton_iterations"] == line["chebyshev"]["newton_iterations"]
    assert abs(line["multigrid"]["max_displacement"] - line["chebyshev"]["max_displacement"]) <= 1e-8


# ------------------------------------------------------------------------------------------------ errors
def test_errors(tb, device):
    L, lib = tb._lib, tb.lib()
    gh = tb.GridHierarchy(box(tb, (2, 2, 2)), 1)
    dh, sp, pattern, K = diffusion_problem(tb, device, gh)
    ch = tb.ConstraintHandler(dh, face_dofs(dh))
    dA = eliminated(tb, device, pattern, K, ch)
    mg = tb.MultigridHierarchy(pattern, gh, ch=ch)
    r, z = device.zeros(dh.ndofs), device.zeros(dh.ndofs)
    assert lib.tb_mg_apply(mg.h, r.ptr, z.ptr) == L.TB_ERR_BAD_ARG                            # before tb_mg_setup
    # a level pattern that does not match the transfer: the parent lists of another refinement
    other = tb.GridHierarchy(box(tb, (3, 2, 2)), 1)
    pptr, pidx = other.parents[0]
    rc = lib.tb_mg_set_transfer(mg.h, 1, other.grids[1].n_nodes, np.ascontiguousarray(pptr, dtype=np.int64).ctypes.data_as(L.c_i64p),
                                np.ascontiguousarray(pidx, dtype=np.int32).ctypes.data_as(L.c_i32p))
    assert rc == L.TB_ERR_BAD_ARG and b"does not match" in lib.tb_last_error_string()
    # setup inside an open capture refuses, and the capture survives
    tb.check(lib.tb_graph_begin(device.h))
    rc = lib.tb_mg_setup(mg.h, dA.ptr, 2, 4.0)
    h = C.c_void_p()
    tb.check(lib.tb_graph_end(device.h, C.byref(h)))
    if h:
        lib.tb_graph_destroy(h)
    assert rc == L.TB_ERR_BAD_ARG
    # a coarsest level above 1024 dofs
    big = tb.GridHierarchy(box(tb, (10, 10, 10)), 1)
    dhb = tb.DofHandler(big.grids[-1])
    spb = tb.allocate_matrix(dhb)
    pb = dhb.device_mesh(device).pattern(spb)
    mgb = tb.MultigridHierarchy(pb, big)
    assert lib.tb_mg_setup(mgb.h, device.to_device(spd_values(spb)).ptr, 2, 4.0) == L.TB_ERR_UNSUPPORTED
    assert b"add a level" in lib.tb_last_error_string()
    # a NaN in A: the solve returns unconverged, as tb_pcg_solve does
    bad = dA.to_host()
    bad[sp.rowptr[dh.ndofs // 2]] = np.nan
    dbad = device.to_device(bad)
    b = np.ones(dh.ndofs); b[ch.prescribed_dofs] = 0.0
    x = device.zeros(dh.ndofs)
    try:
        its, res = mg.solve(dbad, device.to_device(b), x, rtol=1e-8, atol=0.0, maxiter=50)
        assert its <= 50 and not tb.solve_converged(pattern, res), (its, res)
    except tb.TBError as e:
        assert e.code == L.TB_ERR_BAD_ARG
