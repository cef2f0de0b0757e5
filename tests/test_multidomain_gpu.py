"""Multi-domain electrophysiology on the device: the interface matrix against the NumPy restatement (tests/multidomain_reference.py), bulk assembly
on the widened pattern, the coupled heat step, the packed reaction step against the single-model step, the reaction tangent, and the replay of the
reference's "Pacemaker subdomain" test (test/integration/test_electrophysiology.jl:124-195)."""
import ctypes as C

import numpy as np
import pytest

import multidomain_cases as cases
import multidomain_reference as ref
from helpers import rel_err

pytestmark = pytest.mark.gpu

WITH_INTERFACE = ["quad_2x1", "hex_2x1x1", "quad_3x3_centre", "hex_4x4x4_inner", "quad_split_to_boundary", "hex_3x2x2_perturbed"]
_CACHE = {}


def setup(tb, device, name):
    """grid after the insertion, DofHandler, narrow and widened pattern, device pattern of the widened one — built once per mesh"""
    if name not in _CACHE:
        g, g2 = cases.build(tb, name)
        dh = tb.DofHandler(g2)
        narrow, wide = tb.allocate_matrix(dh), tb.allocate_matrix(dh, g2.interfaces)
        _CACHE[name] = (g2, dh, narrow, wide, dh.device_mesh(device).pattern(wide))
    return _CACHE[name]


def interface_values(tb, device, name, G, q):
    g2, dh, narrow, wide, pat = setup(tb, device, name)
    form = tb.InterfaceDiffusionForm(dh.device_mesh(device), g2.interfaces, G, q)
    nz = device.zeros(wide.nnz)
    form.assemble(pat, nz)
    return form, nz


# ------------------------------------------------------------------------------------------------ the interface matrix
@pytest.mark.parametrize("name", WITH_INTERFACE + ["quad_no_touch"])
def test_interface_matrix_parity(tb, device, name):
    """constant and per-element G, 1, 2 and 3 Gauss points (0 selects 2): the added entries at the parity suite's 1e-12 relative maximum"""
    g2, dh, narrow, wide, pat = setup(tb, device, name)
    it = g2.interfaces
    rng = np.random.default_rng(11)
    for G in (1.7, rng.uniform(0.5, 2.0, len(it))):
        for q in (1, 2, 3, 0):
            _, nz = interface_values(tb, device, name, G, q)
            got = nz.to_host()
            if len(it) == 0:
                assert not got.any()
                continue
            dense = ref.dense_interface_matrix(g2.cell_kind, g2.xyz, g2.conn, dh.cell_dofs, dh.ndofs, it.records, it.pairing, G, q or 2)
            assert not dense[~ref.pattern_mask(wide.rowptr, wide.colidx)].any()
            want = ref.csr_of_dense(wide.rowptr, wide.colidx, dense)
            err = rel_err(got, want)
            print("%s G %s q %d: rel-max error %.3e" % (name, "const" if np.ndim(G) == 0 else "per element", q, err))
            assert err <= 1e-12


@pytest.mark.parametrize("name", WITH_INTERFACE)
def test_interface_matrix_properties(tb, device, name):
    g2, dh, narrow, wide, pat = setup(tb, device, name)
    G = np.random.default_rng(5).uniform(0.5, 2.0, len(g2.interfaces))
    form, nz = interface_values(tb, device, name, G, 2)
    first = nz.to_host()
    K = ref.dense_of_csr(wide.rowptr, wide.colidx, first)
    assert np.array_equal(K, K.T)                                      # symmetric entry for entry
    rows = np.abs(K.sum(axis=1))
    bound = 16 * np.finfo(float).eps * np.abs(K).sum(axis=1)           # each row sums to zero to rounding
    print("%s: max |row sum| %.3e (bound %.3e)" % (name, rows.max(), bound.max()))
    assert np.all(rows <= bound) and np.abs(K).max() > 0
    assert np.all(np.diag(K) <= 0)                                     # the sign of K is TB_FORM_DIFFUSION's
    nz.fill_zero()
    form.assemble(pat, nz)
    assert np.array_equal(nz.to_host().view(np.int64), first.view(np.int64))   # two assemblies: identical bits
    form.assemble(pat, nz)                                             # and it ADDS
    assert np.array_equal(nz.to_host(), 2 * first)


def test_interface_form_errors(tb, device):
    L = tb._lib
    g2, dh, narrow, wide, pat = setup(tb, device, "quad_3x3_centre")
    dm, it = dh.device_mesh(device), g2.interfaces
    form = tb.InterfaceDiffusionForm(dm, it, 1.0)
    with pytest.raises(tb.TBError) as e:                               # the narrow pattern lacks the a–b couplings
        form.assemble(dm.pattern(narrow), device.zeros(narrow.nnz))
    assert e.value.code == L.TB_ERR_PATTERN
    form.assemble(pat, device.zeros(wide.nnz))                         # the form goes on working, on the other pattern
    h = C.c_void_p()

    def create(records, pairing, q=0):
        records, pairing = np.ascontiguousarray(records, dtype=np.int32), np.ascontiguousarray(pairing, dtype=np.int32)
        return tb.lib().tb_interface_form_create(dm.h, records.ctypes.data_as(L.c_i32p), pairing.ctypes.data_as(L.c_i32p), len(records), q, 1.0, None, 0, C.byref(h))

    bad = it.records.copy(); bad[0, 0] = g2.n_cells
    assert create(bad, it.pairing) == L.TB_ERR_BAD_ARG                 # cell out of range
    bad = it.records.copy(); bad[0, 1] = 4
    assert create(bad, it.pairing) == L.TB_ERR_BAD_ARG                 # local facet out of range
    assert create(it.records, it.pairing[:, ::-1]) == L.TB_ERR_BAD_ARG  # copies that do not coincide in space
    assert b"coincide" in tb.lib().tb_last_error_string()
    assert create(it.records, it.pairing, q=4) == L.TB_ERR_BAD_ARG
    # a degenerate facet (both nodes of an edge at one place) raises the status block
    g = tb.Grid(g2.cell_kind, g2.xyz.copy(), g2.conn.copy())
    ca, la, cb, lb = it.records[0]
    va, vb = g.conn[ca, list(ref.FACETS[ref.QUAD][la])], g.conn[cb, it.pairing[0]]
    g.xyz[va[1]] = g.xyz[va[0]]
    g.xyz[vb[1]] = g.xyz[vb[0]]
    dh2 = tb.DofHandler(g)
    dm2 = dh2.device_mesh(device)
    f2 = tb.InterfaceDiffusionForm(dm2, it, 1.0)
    with pytest.raises(tb.TBError) as e:
        f2.assemble(dm2.pattern(tb.allocate_matrix(dh2, it)), device.zeros(wide.nnz))
    assert e.value.code == L.TB_ERR_NEG_DETJ


# ------------------------------------------------------------------------------------------------ bulk assembly on the widened pattern
@pytest.mark.parametrize("name", ["hex_4x4x4_inner", "quad_6x6"])
@pytest.mark.parametrize("strategy", ["Atomic", "PerColor", "Element", "Patch"])
def test_bulk_assembly_on_the_widened_pattern(tb, device, name, strategy):
    """M and K, one by one and as the fused pair: interface-only entries exactly 0.0, every other entry the bits it has on the narrow pattern"""
    g2, dh, narrow, wide, pat = setup(tb, device, name)
    st = getattr(tb, strategy + "AssemblyStrategy")(device)
    kap = np.diag([4.5e-4, 2.0e-4, 1.0e-4][:2 if g2.cell_kind == tb.Quadrilateral else 3])
    D = tb.ConductivityToDiffusivityCoefficient(tb.ConstantCoefficient(kap), tb.ConstantCoefficient(1.0), tb.ConstantCoefficient(1.0))
    mask_n = ref.pattern_mask(narrow.rowptr, narrow.colidx)
    in_narrow = ref.csr_of_dense(wide.rowptr, wide.colidx, mask_n)       # the column map: which widened entries the narrow pattern has, in its order
    assert in_narrow.sum() == narrow.nnz and (~in_narrow).sum() == wide.nnz - narrow.nnz > 0
    out = {}
    for label, sp in (("narrow", narrow), ("wide", wide)):
        M = tb.setup_operator(st, tb.BilinearMassIntegrator(tb.ConstantCoefficient(1.0)), dh, sp)
        K = tb.setup_operator(st, tb.BilinearDiffusionIntegrator(D), dh, sp)
        tb.update_operator(M, 0.0)
        tb.update_operator(K, 0.0)
        single = (M.A.to_host(), K.A.to_host())
        M.A.copy_from_host(np.full(sp.nnz, 7.0))                         # outputs are overwritten, not added to
        K.A.copy_from_host(np.full(sp.nnz, 7.0))
        tb.update_operators(M, K, 0.0)
        out[label] = single + (M.A.to_host(), K.A.to_host())
    for what, n, w in zip(("M", "K", "M of the pair", "K of the pair"), out["narrow"], out["wide"]):
        extra = w[~in_narrow]
        assert np.array_equal(extra, np.zeros_like(extra)), (what, "interface-only entries")
        assert np.array_equal(w[in_narrow].view(np.int64), n.view(np.int64)), (what, "bits on the narrow pattern")
        assert np.abs(n).max() > 0


# ------------------------------------------------------------------------------------------------ the coupled heat step
def fhn_models(tb, G, ion_a=None, ion_b=None, sdim=2, coords=None):
    kap = tb.ConstantCoefficient(np.diag([4.5e-4, 2.0e-4, 2.0e-4][:sdim]))
    one = tb.ConstantCoefficient(1.0)
    return {"a": tb.MonodomainModel(one, one, kap, tb.NoStimulationProtocol(), ion_a or tb.FHNModel(), "φₘ", "s1", cell_coordinates=coords),
            "b": tb.MonodomainModel(one, one, kap, tb.NoStimulationProtocol(), ion_b or tb.FHNModel(), "φₘ", "s2", cell_coordinates=coords),
            "interfaces": tb.InterfaceDiffusionModel(tb.ConstantCoefficient(G), "φₘ", "φₘi")}


def heat_problem(tb, device, name, G, phi_a):
    g, g2 = cases.build(tb, name)
    fun = tb.semidiscretize_ep(tb.ReactionDiffusionSplit(fhn_models(tb, G, sdim=2 if g2.cell_kind == tb.Quadrilateral else 3)), tb.PatchAssemblyStrategy(device), g2)
    on_a = np.zeros(fun.dh.ndofs, dtype=bool)
    on_a[fun.subdofs[0]] = True
    x = tb.dof_coordinates(fun.dh)
    phi0 = np.where(on_a, phi_a(x), 0.0)
    u0 = fun.initial_condition()
    u0[fun.heat_dofrange] = phi0
    cache = tb.setup_solver_cache(fun.functions, tb.ForwardEulerCellSolver(device), u=device.to_device(u0))
    ltg = tb.MultiDomainLieTrotterGodunov(fun.heat_stage(tb.BackwardEulerSolver()), fun.functions, cache)
    return fun, ltg, on_a, phi0, u0


@pytest.mark.parametrize("name", ["quad_6x6", "hex_4x4x4_inner"])
def test_decoupled_subdomains_do_not_exchange(tb, device, name):
    """G = 0: the system is block diagonal, and CG with zero right-hand side and zero initial guess on a block never leaves zero"""
    for phi_a in (lambda x: np.ones(len(x)), lambda x: 1.0 + 0.5 * np.sin(3.0 * x[:, 0]) * np.cos(2.0 * x[:, 1])):
        fun, ltg, on_a, phi0, u0 = heat_problem(tb, device, name, 0.0, phi_a)
        assert ltg.heat_step(0.0, 1.0)
        u = ltg.cell.u.to_host()
        phi = u[fun.heat_dofrange]
        assert np.array_equal(phi[~on_a], np.zeros((~on_a).sum()))       # exactly 0
        assert np.array_equal(ltg.phi.to_host(), phi)                    # the scatter wrote the heat vector back
        rest = np.ones(len(u), dtype=bool)
        rest[fun.heat_dofrange] = False
        assert np.array_equal(u[rest], u0[rest])                         # the other states are untouched
    assert ltg.heat.last_iters > 0 and not np.array_equal(phi[on_a], phi0[on_a])


@pytest.mark.parametrize("name", ["quad_6x6", "hex_4x4x4_inner"])
def test_coupled_subdomains_exchange(tb, device, oracle, name):
    """G > 0: φₘ on b moves, and the host residual with the reference-assembled matrix meets the solver's own stopping test"""
    dt, G = 1.0, 1.0
    fun, ltg, on_a, phi0, u0 = heat_problem(tb, device, name, G, lambda x: np.ones(len(x)))
    assert ltg.heat_step(0.0, dt)
    phi = ltg.cell.u.to_host()[fun.heat_dofrange]
    assert np.abs(phi[~on_a]).max() > 1e-6
    g2, dh, sp, it = fun.grid, fun.dh, fun.pattern, fun.interfaces
    quad = g2.cell_kind == tb.Quadrilateral
    om = oracle.Mesh(oracle.QUAD4 if quad else oracle.HEX8, 2, np.ascontiguousarray(g2.xyz[:, :2]) if quad else g2.xyz, g2.conn, dh.cell_dofs)
    kap = np.diag([4.5e-4, 2.0e-4]) if quad else np.diag([4.5e-4, 2.0e-4, 2.0e-4])
    M = oracle.assemble_matrix(om, 0, oracle.Coef(oracle.COEF_CONST_SCALAR, [1.0]), sp.rowptr, sp.colidx)
    K = oracle.assemble_matrix(om, 1, oracle.Coef(oracle.COEF_CONST_TENSOR, kap.ravel(), Cm=1.0, chi=1.0, wrap=True), sp.rowptr, sp.colidx)
    K = K + ref.csr_of_dense(sp.rowptr, sp.colidx, ref.dense_interface_matrix(g2.cell_kind, g2.xyz, g2.conn, dh.cell_dofs, dh.ndofs, it.records, it.pairing, G, 2))
    assert rel_err(fun.K.A.to_host(), K) <= 1e-12 and rel_err(fun.M.A.to_host(), M) <= 1e-12
    A = ref.dense_of_csr(sp.rowptr, sp.colidx, M - dt * K)
    b = ref.dense_of_csr(sp.rowptr, sp.colidx, M) @ phi0
    r0, r = np.linalg.norm(b - A @ phi0), np.linalg.norm(b - A @ phi)
    tol = ltg.heat.solver.atol + ltg.heat.solver.rtol * r0
    print("%s: |r0| %.3e  |r| %.3e  tolerance %.3e  iterations %d" % (name, r0, r, tol, ltg.heat.last_iters))
    assert r <= tol < r0


# ------------------------------------------------------------------------------------------------ the packed reaction step
def packed_problem(tb, device, layout, solvers, coords=None):
    g, g2 = cases.build(tb, "quad_6x6")
    fun = tb.semidiscretize_ep(tb.ReactionDiffusionSplit(fhn_models(tb, 1.0, tb.PCG2019(), tb.FHNModel(), coords=coords)), tb.PatchAssemblyStrategy(device), g2,
                               layout=layout)
    rng = np.random.default_rng(3)
    u0 = fun.initial_condition()
    u0[fun.heat_dofrange] += rng.uniform(0.0, 30.0, fun.dh.ndofs) * np.where(np.isin(np.arange(fun.dh.ndofs), fun.subdofs[0]), 1.0, 0.02)
    cache = tb.setup_solver_cache(fun.functions, solvers, u=device.to_device(u0))
    return fun, tb.MultiDomainLieTrotterGodunov(fun.heat_stage(), fun.functions, cache), u0


def cell_solvers(tb, device, which):
    if which == "euler":
        return [tb.ForwardEulerCellSolver(device)] * 2
    if which == "substepping":
        return [tb.AdaptiveForwardEulerSubstepper(device, substeps=8, reaction_threshold=0.5)] * 2
    return [tb.RushLarsenCellSolver(device), tb.ForwardEulerCellSolver(device)]     # FHN has no gate decomposition: its child steps forward Euler


@pytest.mark.parametrize("layout", ["PointBlocked", "StateBlocked"])
@pytest.mark.parametrize("which", ["euler", "substepping", "rush_larsen"])
@pytest.mark.parametrize("coords", [None, "cartesian"])
def test_packed_reaction_step_is_the_single_model_step(tb, device, layout, which, coords):
    """PCG2019 (7 states) beside FHN (2 states): every child's block after the packed step has the bits of the existing single-model step run on a
    copy of that block — it is the same kernel on the same data (one launch per child; the children are not fused)"""
    lay = getattr(tb, layout + "Layout")()
    solvers = cell_solvers(tb, device, which)
    fun, ltg, u0 = packed_problem(tb, device, lay, solvers, coords)
    t, dt = 0.3, 0.01
    for _ in range(2):
        assert ltg.reaction_step(t, dt)
    got = ltg.cell.u.to_host()
    assert not np.array_equal(got, u0)
    f = fun.functions
    for k, (child, solver) in enumerate(zip(f.functions, solvers)):
        lo, hi = int(f.offsets[k]), int(f.offsets[k + 1])
        assert (child.x is not None) == (coords is not None)
        single = tb.PointwiseODEFunction(child.npoints, child.ode, child.x, layout=lay)
        cache = tb.setup_solver_cache(single, solver, u=device.to_device(u0[lo:hi].copy()))
        for _ in range(2):
            tb.perform_step(single, cache, t, dt)
        want = cache.un.to_host()
        assert np.isfinite(want).all() and not np.array_equal(want, u0[lo:hi])
        assert np.array_equal(got[lo:hi].view(np.int64), want.view(np.int64)), (k, layout, which)


@pytest.mark.parametrize("layout", ["PointBlocked", "StateBlocked"])
def test_reaction_tangent_is_the_maximum_over_the_children(tb, device, layout):
    lay = getattr(tb, layout + "Layout")()
    fun, ltg, u0 = packed_problem(tb, device, lay, [tb.ForwardEulerCellSolver(device)] * 2)
    f = fun.functions

    def host_R():
        rs = []
        for k, (child, c) in enumerate(zip(f.functions, ltg.cell.children)):
            du = c.du.to_host()
            du = du.reshape(child.npoints, child.ode.nstates) if layout == "PointBlocked" else du.reshape(child.ode.nstates, child.npoints).T
            rs.append(du[:, child.ode.phi_index].max() if not np.isnan(du[:, child.ode.phi_index]).any() else np.nan)
        return rs

    ok, R = ltg.step_with_reaction_tangent(0.0, 0.01)
    rs = host_R()
    print("R %.6e, children %s" % (R, rs))
    assert ok and R == max(rs) and rs[0] != rs[1]
    ok, R2 = ltg.reaction_step_with_tangent(0.01, 0.01)
    assert ok and R2 == max(host_R())
    # a NaN in the internal state of ONE point of the second child reaches R (φₘ and with it the heat step stay finite)
    u = ltg.cell.u.to_host()
    lo = int(f.offsets[1])
    u[lo + (1 if layout == "PointBlocked" else f.functions[1].npoints)] = np.nan
    ltg.cell.u.copy_from_host(u)
    ok, R3 = ltg.step_with_reaction_tangent(0.02, 0.01)
    assert np.isnan(R3) and np.isnan(host_R()[1]) and np.isfinite(host_R()[0])
    rtc = tb.ReactionTangentController(ltg, 0.5, 1.0, (0.5, 2.0))
    with pytest.raises(RuntimeError, match="non-finite reaction tangent"):     # the existing rule of the controller applies
        rtc.solve(0.03, 0.05, 0.01)


# ------------------------------------------------------------------------------------------------ replay of "Pacemaker subdomain"
def isapprox(x, y, rtol):
    """Julia's x ≈ y rtol=…: ‖x − y‖ ≤ rtol · max(‖x‖, ‖y‖)"""
    return np.linalg.norm(x - y) <= rtol * max(np.linalg.norm(x), np.linalg.norm(y))


@pytest.fixture(scope="module")
def pacemaker_grid(tb):
    grid = tb.generate_mesh(tb.Quadrilateral, (64, 64), (-2.5, -2.5), (2.5, 2.5))
    pm = grid.addcellset("Pacemaker", lambda x: np.abs(x).max() <= 0.75)
    grid.addcellset("Myocardium", np.setdiff1d(np.arange(grid.n_cells), pm))
    return tb.insert_interfaces(grid, ["Pacemaker", "Myocardium"])


def solve_waveprop(tb, device, grid, models, stepper, strategy=None):
    """solve_waveprop of the reference test: φ₀ = max(1 − ‖x‖, 0), tspan (0, 10), Δt = 1; returns (final packed state, accepted steps)"""
    fun = tb.semidiscretize_ep(tb.ReactionDiffusionSplit(models), strategy or tb.PatchAssemblyStrategy(device), grid)
    u0 = fun.initial_condition()
    u0[:] = 0.0                                                          # u₀ = zeros(solution_size), then simple_initializer!
    u0[fun.heat_dofrange] = np.maximum(1.0 - np.linalg.norm(tb.dof_coordinates(fun.dh), axis=1), 0.0)
    cell = tb.AdaptiveForwardEulerSubstepper(device) if stepper == "adaptive" else tb.ForwardEulerCellSolver(device)
    cache = tb.setup_solver_cache(fun.functions, cell, u=device.to_device(u0))
    ltg = tb.MultiDomainLieTrotterGodunov(fun.heat_stage(tb.BackwardEulerSolver()), fun.functions, cache)
    if stepper == "rtc":
        hist = tb.ReactionTangentController(ltg, 0.5, 1.0, (0.5, 2.0)).solve(0.0, 10.0, 1.0)
        assert abs(sum(h for _, h in hist) - 10.0) < 1e-12
        naccept = len(hist)
    else:
        for k in range(10):
            assert ltg.step(float(k), 1.0), k                            # retcode Success
        naccept = 10
    u = cache.u.to_host()
    assert np.isfinite(u).all() and not isapprox(u, u0, 1e-8)            # integrator.u ≉ u₀
    return u, naccept


def pacemaker_models(tb):
    kap = tb.ConstantCoefficient(np.diag([4.5e-4, 2.0e-4]))
    one = tb.ConstantCoefficient(1.0)
    return {"Pacemaker": tb.MonodomainModel(one, one, kap, tb.NoStimulationProtocol(), tb.FHNModel(a=-0.5, b=1.0, c=-0.6, d=0.0, e=0.001, f=50 * 0.001), "φₘ", "s1"),
            "Myocardium": tb.MonodomainModel(one, one, kap, tb.NoStimulationProtocol(), tb.FHNModel(), "φₘ", "s2"),
            "interfaces": tb.InterfaceDiffusionModel(tb.ConstantCoefficient(1.0), "φₘ", "φₘi")}


def aliev_panfilov_on_the_pacemaker(tb):
    return {"Pacemaker": tb.MonodomainModel(tb.ConstantCoefficient(1.0), tb.ConstantCoefficient(1.0), tb.ConstantCoefficient(np.diag([4.5e-4, 2.0e-4])),
                                            tb.NoStimulationProtocol(), tb.AlievPanfilovModel(), "φₘ", "s1")}


@pytest.mark.parametrize("variant", ["two_subdomains", "pacemaker_only"])
def test_pacemaker_subdomain_replay(tb, device, pacemaker_grid, variant):
    models = pacemaker_models(tb) if variant == "two_subdomains" else aliev_panfilov_on_the_pacemaker(tb)
    u, n = solve_waveprop(tb, device, pacemaker_grid, models, "fixed")
    ua, _ = solve_waveprop(tb, device, pacemaker_grid, models, "adaptive")
    ur, nr = solve_waveprop(tb, device, pacemaker_grid, models, "rtc")
    d = lambda x, y: np.linalg.norm(x - y) / max(np.linalg.norm(x), np.linalg.norm(y))  # noqa: E731
    print("%s: fixed vs adaptive %.3e (1e-3), fixed vs RTC %.3e (5e-2), accepted steps %d vs %d" % (variant, d(u, ua), d(u, ur), n, nr))
    assert isapprox(u, ua, 1e-3)
    assert isapprox(u, ur, 5e-2)
    assert nr != n
    if variant == "two_subdomains":
        assert len(pacemaker_grid.interfaces) == 4 * 18 and len(u) == 2 * (65 * 65 + 72)
    else:
        assert len(u) == 2 * 19 * 19                                     # the Pacemaker cells alone: an 18 × 18 sub-grid


def test_hexahedral_end_to_end(tb, device):
    """five steps on the 4 × 4 × 4 box with the inner cube as pacemaker: they succeed, and two runs give the same bits (element strategy: its sums are ordered)"""
    g, g2 = cases.build(tb, "hex_4x4x4_inner")
    models = fhn_models(tb, 1.0, tb.FHNModel(a=-0.5, b=1.0, c=-0.6, d=0.0, e=0.001, f=0.05), tb.FHNModel(), sdim=3)
    runs = []
    for _ in range(2):
        fun = tb.semidiscretize_ep(tb.ReactionDiffusionSplit(models), tb.ElementAssemblyStrategy(device), g2)
        u0 = fun.initial_condition(lambda x: max(1.0 - np.linalg.norm(x - np.array([2.0, 1.5, 1.0])), 0.0))
        cache = tb.setup_solver_cache(fun.functions, tb.ForwardEulerCellSolver(device), u=device.to_device(u0))
        ltg = tb.MultiDomainLieTrotterGodunov(fun.heat_stage(), fun.functions, cache)
        for k in range(5):
            assert ltg.step(float(k), 1.0)
        runs.append(cache.u.to_host())
        assert np.isfinite(runs[-1]).all() and not np.array_equal(runs[-1], u0)
    assert np.array_equal(runs[0].view(np.int64), runs[1].view(np.int64))


def test_the_pacemaker_example_runs():
    """examples/pacemaker_2d.py at toy size (prints one JSON line)"""
    import json, os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "examples", "pacemaker_2d.py"), "--n", "16", "--tend", "3"], capture_output=True, text=True, timeout=300, cwd=root)
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads(out.stdout.strip().splitlines()[-1])
    assert d["time_steps"] == 3 and d["moved"] and d["interface_elements"] == 16 and d["solution_size"] == 2 * (17 * 17 + 16)
