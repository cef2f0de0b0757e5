"""The p-level of the multigrid on the device (tb_multigrid.hip: tb_mg_set_p_transfer, k_mg_galerkin_b3) against the numpy restatement of
tests/pmultigrid_reference.py: transfers, Galerkin level matrices under both plans, one V-cycle of a chained hierarchy, the preconditioned solve of
second-order diffusion (tensor diag(9, 4, 4), Dirichlet on x = 0, levels down to 2³ cells) and the Newton solve of a clamped second-order Guccione bar."""
import ctypes as C

import numpy as np
import pytest

import pmultigrid_reference as pref

pytestmark = pytest.mark.gpu

TENSOR = (9.0, 4.0, 4.0)


def box(tb, nel, perturb=0.0):
    return tb.generate_mesh(tb.Hexahedron, nel, (0, 0, 0), (1, 1, 1), perturb=perturb)


def component_of(dh):
    comp, nc = np.empty(dh.ndofs, dtype=np.int64), dh.ip.ncomp
    for k in range(nc):
        comp[dh.cell_dofs[:, k::nc].ravel()] = k
    return comp


def face_dofs(tb, dh, axis=0, value=0.0, components=None):
    """the dofs of the nodes (vertices, edge, face centres) on the face x_axis = value; components: None = all"""
    on = np.abs(tb.dof_coordinates(dh)[:, axis] - value) < 1e-12
    if components is not None:
        on &= np.isin(component_of(dh), components)
    return np.flatnonzero(on)


def spd_values(sp):
    """a symmetric, strictly diagonally dominant matrix on the pattern"""
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


def scalar_forms(tb, device, dh, sp):
    """(M, K) of the field of dh with the constant tensor, host values"""
    st = tb.ElementAssemblyStrategy(device)
    K = tb.update_operator(tb.setup_operator(st, tb.BilinearDiffusionIntegrator(tb.ConstantCoefficient(np.diag(TENSOR))), dh, sp), 0.0)
    M = tb.update_operator(tb.setup_operator(st, tb.BilinearMassIntegrator(tb.ConstantCoefficient(1.0)), dh, sp), 0.0)
    return M.A.to_host(), K.A.to_host(), K.pattern


def eliminated(tb, device, pattern, vals, ch):
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
def test_p_transfers_are_P_and_its_transpose(tb, device, ncomp, prescribed):
    dh = tb.DofHandler(box(tb, (2, 2, 2), perturb=0.2), tb.LagrangeCollection(2, ncomp))
    sp = tb.allocate_matrix(dh)
    pattern = dh.device_mesh(device).pattern(sp)
    ch = tb.ConstraintHandler(dh, face_dofs(tb, dh)) if prescribed else None
    mg = tb.PMGPrecon().materialize(pattern, ch)
    mg.setup(eliminated(tb, device, pattern, spd_values(sp), ch))
    assert mg.n_levels == 2 and mg.dhs[0].ip.order == 1 and mg.dhs[1] is dh
    P, _ = pref.dense_p_level(tb, dh, mg.dhs[0], flags_of(dh, ch) if prescribed else None)
    rng = np.random.default_rng(3)
    x, y = rng.normal(size=P.shape[1]), rng.normal(size=P.shape[0])
    px = mg.prolong(1, device.to_device(x), device.zeros(P.shape[0])).to_host()
    rty = mg.restrict(1, device.to_device(y), device.zeros(P.shape[1])).to_host()
    e1, e2 = relerr(px, P @ x), relerr(rty, P.T @ y)
    print("%d -> %d dofs: prolong %.2e restrict %.2e" % (P.shape[1], P.shape[0], e1, e2))
    assert e1 <= 1e-15 and e2 <= 1e-15


# ------------------------------------------------------------------------------------------------ Galerkin products
def check_p_level(tb, device, dh, pattern, vals, ch, blocked):
    mg = tb.PMGPrecon().materialize(pattern, ch)
    dA = eliminated(tb, device, pattern, vals, ch)
    mg.setup(dA)
    first = mg.level_matrix(0)
    mg.setup(dA)
    assert np.array_equal(first, mg.level_matrix(0)), "two setups differ"
    flags = flags_of(dh, ch)
    P, cpre = pref.dense_p_level(tb, dh, mg.dhs[0], flags if flags.any() else None)
    Ac = pref.galerkin(P, pref.csr_to_dense(pattern.sp, dA.to_host()), cpre)
    want = pref.dense_to_csr(mg.sps[0], Ac)
    assert np.array_equal(pref.csr_to_dense(mg.sps[0], want) != 0, Ac != 0)                 # nothing of PᵀAP lies outside the Q1 pattern
    err = np.abs(first - want).max() / np.abs(want).max()
    got_blocked, terms = mg.plan(1)
    print("blocked %s, %d terms, %d plan bytes: max |A_c - PtAP| / max |PtAP| = %.3e" % (got_blocked, terms, mg.plan_bytes(1), err))
    assert err <= 1e-12
    assert got_blocked == blocked and terms > 0
    return mg, first


def test_galerkin_of_a_scalar_heat_matrix(tb, device):
    dh = tb.DofHandler(box(tb, (3, 2, 2), perturb=0.2), tb.LagrangeCollection(2))
    sp = tb.allocate_matrix(dh)
    M, K, pattern = scalar_forms(tb, device, dh, sp)
    check_p_level(tb, device, dh, pattern, M - 0.05 * K, None, blocked=False)


def guccione_tangent(tb, device, dh, sp, ch, facets):
    ms = tb.ConstantCoefficient(tb.OrthotropicMicrostructure(*np.eye(3)))
    model = tb.QuasiStaticModel("d", tb.PK1Model(tb.Guccione1991PassiveModel(), ms), list(facets))
    op = tb.setup_operator(tb.ElementAssemblyStrategy(device), model, dh, sp)
    u = np.random.default_rng(5).uniform(-5e-3, 5e-3, dh.ndofs)
    u[ch.prescribed_dofs] = 0.0
    tb.update_linearization(op, device.to_device(u), 0.0, residual=device.zeros(dh.ndofs))
    return op


@pytest.mark.parametrize("face", ["clamped", "x_only"])
def test_galerkin_of_a_guccione_tangent_under_both_plans(tb, device, face):
    """the default numbering is node-blocked: the blocked plan (with the x-only face the prescribed dofs cut through the blocks); the same tangent
    with both levels' dofs renumbered at random takes the per-dof plan; both give PᵀAP"""
    g = box(tb, (3, 2, 2), perturb=0.2)
    dh = tb.DofHandler(g, tb.LagrangeCollection(2) ** 3)
    sp = tb.allocate_matrix(dh)
    ch = tb.ConstraintHandler(dh, face_dofs(tb, dh, components=None if face == "clamped" else [0]))
    op = guccione_tangent(tb, device, dh, sp, ch, [tb.RobinBC(0.3, "right")])
    J = op.J.to_host()
    check_p_level(tb, device, dh, op.pattern, J, ch, blocked=True)
    # the same matrix under a random numbering of the Q2 dofs: A'[perm[i], perm[j]] = A[i, j]
    perm = np.random.default_rng(17).permutation(dh.ndofs).astype(np.int32)
    dh2 = tb.renumber_dofs(dh, perm)
    sp2 = tb.allocate_matrix(dh2)
    A2 = np.zeros((dh.ndofs, dh.ndofs))
    A2[np.ix_(perm, perm)] = pref.csr_to_dense(sp, J)
    ch2 = tb.ConstraintHandler(dh2, np.sort(perm[ch.prescribed_dofs]))
    pattern2 = dh2.device_mesh(device).pattern(sp2)
    check_p_level(tb, device, dh2, pattern2, pref.dense_to_csr(sp2, A2), ch2, blocked=False)


def test_galerkin_of_affine_cells_is_the_first_order_assembly(tb, device):
    """constant coefficients on an unperturbed box: Q1 ⊂ Q2 on the same cells and both quadratures are exact on affine cells, so Pᵀ(M − 0.05 K)_Q2 P is
    the matrix assembled on the first-order handler.  No permutation of the 27-node table but the right one passes."""
    dh = tb.DofHandler(box(tb, (3, 2, 2)), tb.LagrangeCollection(2))
    sp = tb.allocate_matrix(dh)
    M, K, pattern = scalar_forms(tb, device, dh, sp)
    mg = tb.PMGPrecon().materialize(pattern).setup(device.to_device(M - 0.05 * K))
    M1, K1, _ = scalar_forms(tb, device, mg.dhs[0], mg.sps[0])
    err = relerr(mg.level_matrix(0), M1 - 0.05 * K1)
    print("Galerkin vs first-order assembly: %.3e" % err)
    assert err <= 1e-12


# ------------------------------------------------------------------------------------------------ cycle
@pytest.fixture(scope="module")
def cycle_problem(tb, device):
    gh = tb.GridHierarchy(box(tb, (2, 2, 2)), 1)                       # 2³ → 4³ cells (Q1), Q2 on 4³
    dh = tb.DofHandler(gh.grids[-1], tb.LagrangeCollection(2))
    sp = tb.allocate_matrix(dh)
    _, K, pattern = scalar_forms(tb, device, dh, sp)
    ch = tb.ConstraintHandler(dh, face_dofs(tb, dh))
    dA = eliminated(tb, device, pattern, -K, ch)
    mg = tb.ChainedMGPrecon(tb.PMGPrecon(), tb.GMGPrecon(gh)).materialize(pattern, ch).setup(dA)
    assert mg.n_levels == 3 and [d.ip.order for d in mg.dhs] == [1, 1, 2]
    As, Ps, pres = pref.chained(tb, gh, mg.dhs, pref.csr_to_dense(sp, dA.to_host()), flags_of(dh, ch))
    lmax = [None] + [mg.lambda_max(l) for l in range(1, mg.n_levels)]
    return mg, dh, ch, As, Ps, pres, lmax


def test_chained_levels_are_the_galerkin_chain(tb, device, cycle_problem):
    mg, dh, ch, As, Ps, pres, lmax = cycle_problem
    for l in range(mg.n_levels - 1):
        assert relerr(mg.level_matrix(l), pref.dense_to_csr(mg.sps[l], As[l])) <= 1e-12, l


def test_chained_cycle_is_the_numpy_cycle(tb, device, cycle_problem):
    mg, dh, ch, As, Ps, pres, lmax = cycle_problem
    rng = np.random.default_rng(11)
    for k in range(2):
        r = rng.normal(size=dh.ndofs)
        z = mg.apply(device.to_device(r), device.zeros(dh.ndofs)).to_host()
        want = pref.vcycle(As, Ps, pres, lmax, mg.degree, mg.interval_ratio, r)
        err = relerr(z, want)
        print("rhs %d: lambda_max %s, max |z - z_numpy| / max |z_numpy| = %.3e" % (k, lmax[1:], err))
        assert err <= 1e-10
        assert np.all(z[ch.prescribed_dofs] == 0.0)               # r is non-zero there


def test_chained_cycle_is_symmetric_and_positive(tb, device, cycle_problem):
    mg, dh = cycle_problem[0], cycle_problem[1]
    rng = np.random.default_rng(12)
    x, y = rng.normal(size=dh.ndofs), rng.normal(size=dh.ndofs)
    mx = mg.apply(device.to_device(x), device.zeros(dh.ndofs)).to_host()
    my = mg.apply(device.to_device(y), device.zeros(dh.ndofs)).to_host()
    asym = abs(x @ my - y @ mx) / abs(x @ my)
    print("x.M^-1 y = %.15e, y.M^-1 x = %.15e, relative difference %.2e" % (x @ my, y @ mx, asym))
    assert asym <= 1e-12 and x @ mx > 0.0


def test_chained_cycle_replays_from_a_graph_with_the_same_bits(tb, device, cycle_problem):
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
def test_preconditioned_solve_of_second_order_diffusion(tb, device):
    """measured on one MI355X: multigrid 8 / 9 / 9 iterations at 4³ / 8³ / 16³ second-order cells, Jacobi 60 / 116 / 232 — the multigrid count grows
    by one where Jacobi's grows 3.9-fold, so the bound is the one the h-levels carry: at most two iterations more over two refinements"""
    its, jac = {}, {}
    for refinements in (1, 2, 3):                                  # Q2 on 4³, 8³, 16³ cells over a coarsest grid of 2³
        gh = tb.GridHierarchy(box(tb, (2, 2, 2)), refinements)
        dh = tb.DofHandler(gh.grids[-1], tb.LagrangeCollection(2))
        sp = tb.allocate_matrix(dh)
        _, K, pattern = scalar_forms(tb, device, dh, sp)
        ch = tb.ConstraintHandler(dh, face_dofs(tb, dh))
        dA = eliminated(tb, device, pattern, -K, ch)
        b = np.random.default_rng(21).uniform(0.0, 1.0, dh.ndofs)
        b[ch.prescribed_dofs] = 0.0
        db = device.to_device(b)
        n = 2 ** (refinements + 1)
        x = device.zeros(dh.ndofs)
        mg = tb.ChainedMGPrecon(tb.PMGPrecon(), tb.GMGPrecon(gh)).materialize(pattern, ch)
        its[n], res = tb.pcg_solve(pattern, dA, db, x, rtol=1e-10, atol=0.0, maxiter=200, precond=mg)
        assert tb.solve_converged(pattern, res), (n, its[n], res)
        xj = device.zeros(dh.ndofs)
        jac[n], resj = tb.pcg_solve(pattern, dA, db, xj, rtol=1e-10, atol=0.0, maxiter=5000, precond="jacobi")
        assert tb.solve_converged(pattern, resj)
        err = relerr(x.to_host(), xj.to_host())
        print("%d^3 Q2 cells, %d dofs: multigrid PCG %d iterations, Jacobi PCG %d, solutions differ by %.2e" % (n, dh.ndofs, its[n], jac[n], err))
        assert err <= 1e-6
        assert its[n] < jac[n], (n, its, jac)
    print("growth 4^3 -> 16^3: multigrid %d -> %d, Jacobi %d -> %d" % (its[4], its[16], jac[4], jac[16]))
    assert its[16] <= its[4] + 2, (its, jac)


# ------------------------------------------------------------------------------------------------ Newton
@pytest.mark.parametrize("pressure", [False, True])
def test_newton_with_chained_multigrid_reaches_the_chebyshev_solution(tb, device, pressure):
    """The free end is pulled by 0.001 in one step.  The first tangent — zero displacement inside, the whole pull in the last layer of cells — must be
    positive definite for CG under any preconditioner: on these second-order cells its smallest eigenvalue is +2.8e-4 at a pull of 0.001 and
    −3.5e-2 / −2.7e-1 at 0.002 / 0.004 (dense eigenvalues of the eliminated tangent), where CG refuses the matrix with the Chebyshev polynomial
    and with the multigrid alike."""
    gh = tb.GridHierarchy(tb.generate_mesh(tb.Hexahedron, (4, 1, 1), (0, 0, 0), (4.0, 1.0, 1.0)), 1)
    out = {}
    for name, precond in (("multigrid", tb.ChainedMGPrecon(tb.PMGPrecon(), tb.GMGPrecon(gh))), ("chebyshev", tb.ChebyshevPrecBuilder(8))):
        dh = tb.DofHandler(gh.grids[-1], tb.LagrangeCollection(2) ** 3)
        sp = tb.allocate_matrix(dh)
        ms = tb.ConstantCoefficient(tb.OrthotropicMicrostructure(*np.eye(3)))
        model = tb.QuasiStaticModel("d", tb.PK1Model(tb.Guccione1991PassiveModel(), ms), [tb.ConstantPressureBC(0.001, "top")] if pressure else [])
        op = tb.setup_operator(tb.ElementAssemblyStrategy(device), model, dh, sp)
        left, right = face_dofs(tb, dh, 0, 0.0), face_dofs(tb, dh, 0, 4.0, components=[0])
        ch = tb.ConstraintHandler(dh, np.concatenate([left, right]))
        order = {d: k for k, d in enumerate(ch.prescribed_dofs)}
        ch.values[[order[d] for d in right]] = 0.001                # the free end is pulled along the bar
        u = device.zeros(dh.ndofs)
        tb.apply(u, ch)
        solver = tb.NewtonRaphsonSolver(max_iter=20, tol=1e-9, inner_rtol=1e-8, inner_solver="cg", inner_precond=precond)
        assert tb.nlsolve(u, op, ch, solver), (name, solver.residual_norms, solver.linear_failure)
        out[name] = (u.to_host(), solver.iter, list(solver.linear_iters))
    print("pressure %s: Newton iterations %d / %d, linear iterations multigrid %s, Chebyshev(8) %s"
          % (pressure, out["multigrid"][1], out["chebyshev"][1], out["multigrid"][2], out["chebyshev"][2]))
    assert relerr(out["multigrid"][0], out["chebyshev"][0]) <= 1e-8
    assert out["multigrid"][1] == out["chebyshev"][1]


def test_the_beam_example_runs():
    """examples/pmultigrid_beam.py: the second-order bar at toy size converges with both preconditioners"""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "examples", "pmultigrid_beam.py")], capture_output=True, text=True, timeout=300, cwd=root)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-1500:])
    line = json.loads(out.stdout.strip().splitlines()[-1])
    print(out.stdout)
    assert line["converged"] and line["levels"] == 3 and line["p_level_blocked"]
    assert line["multigrid"]["converged"] and line["chebyshev"]["converged"]
    assert line["multigrid"]["newton_iterations"] == line["chebyshev"]["newton_iterations"]
    assert abs(line["multigrid"]["max_displacement"] - line["chebyshev"]["max_displacement"]) <= 1e-8


# ------------------------------------------------------------------------------------------------ errors
def test_errors(tb, device):
    """argument checks: every refusal names its condition and none reaches a kernel"""
    L, lib = tb._lib, tb.lib()
    gh = tb.GridHierarchy(box(tb, (2, 2, 2)), 1)
    q1c, q1f = tb.DofHandler(gh.grids[0]), tb.DofHandler(gh.grids[1])
    q2 = tb.DofHandler(gh.grids[1], tb.LagrangeCollection(2))
    pats = [d.device_mesh(device).pattern(tb.allocate_matrix(d)) for d in (q1c, q1f, q2)]

    def hierarchy(levels):
        h = C.c_void_p()
        tb.check(lib.tb_mg_create(device.h, len(levels), C.byref(h)))
        for l, p in enumerate(levels):
            tb.check(lib.tb_mg_set_level(h, l, p.h))
        return h

    h = hierarchy([pats[1], pats[2], pats[2]])
    assert lib.tb_mg_set_p_transfer(h, 1) == L.TB_ERR_UNSUPPORTED and b"fine_level must be 2" in lib.tb_last_error_string()      # below the top level
    lib.tb_mg_destroy(h)
    h = hierarchy([pats[0], pats[2]])
    assert lib.tb_mg_set_p_transfer(h, 1) == L.TB_ERR_BAD_ARG and b"cells" in lib.tb_last_error_string()                         # different cell counts
    lib.tb_mg_destroy(h)
    h = hierarchy([pats[1], pats[1]])
    assert lib.tb_mg_set_p_transfer(h, 1) == L.TB_ERR_UNSUPPORTED and b"second-order" in lib.tb_last_error_string()              # a first-order fine level
    lib.tb_mg_destroy(h)
    h = hierarchy([pats[1], pats[2]])
    pptr, pidx = gh.parents[0]
    rc = lib.tb_mg_set_transfer(h, 1, gh.grids[1].n_nodes, np.ascontiguousarray(pptr, dtype=np.int64).ctypes.data_as(L.c_i64p),
                                np.ascontiguousarray(pidx, dtype=np.int32).ctypes.data_as(L.c_i32p))
    assert rc == L.TB_ERR_UNSUPPORTED and b"tb_mg_set_p_transfer" in lib.tb_last_error_string()                                  # an h-transfer on a second-order level
    blocked, terms = C.c_int(), C.c_int64()
    assert lib.tb_mg_level_plan(h, 1, C.byref(blocked), C.byref(terms)) == L.TB_ERR_BAD_ARG                                      # before tb_mg_setup
    # setup inside an open capture refuses, and the capture survives
    tb.check(lib.tb_mg_set_p_transfer(h, 1))
    dA = device.to_device(spd_values(pats[2].sp))
    tb.check(lib.tb_graph_begin(device.h))
    rc = lib.tb_mg_setup(h, dA.ptr, 2, 4.0)
    gr = C.c_void_p()
    tb.check(lib.tb_graph_end(device.h, C.byref(gr)))
    if gr:
        lib.tb_graph_destroy(gr)
    assert rc == L.TB_ERR_BAD_ARG
    tb.check(lib.tb_mg_setup(h, dA.ptr, 2, 4.0))                                                                                 # and outside it runs
    tb.check(lib.tb_mg_level_plan(h, 1, C.byref(blocked), C.byref(terms)))
    assert blocked.value == 0 and terms.value > 0
    lib.tb_mg_destroy(h)
    # PMGPrecon alone over more than 1 024 first-order dofs
    big = tb.DofHandler(box(tb, (10, 10, 10)), tb.LagrangeCollection(2))
    spb = tb.allocate_matrix(big)
    pb = big.device_mesh(device).pattern(spb)
    with pytest.raises(tb.TBError, match="ChainedMGPrecon") as e:
        tb.PMGPrecon().materialize(pb).setup(device.to_device(spd_values(spb)))
    assert e.value.code == L.TB_ERR_UNSUPPORTED
