"""Newmark elastodynamics on the device: the vector mass against the NumPy reference, the fused inertia stage against the composition of entries
that predate it (tb_spmv_csr with M, tb_axpy on the non-zeros), one step against the discrete equations it must satisfy, and replays of the
reference's test/integration/test_elastodynamics.jl with its own thresholds."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import newmark_reference as nref
import tet_reference as tref

from thunderbolt_jl_amd._lib import check as _check  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = 1e-12
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORTHO = ([1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0])


# ----------------------------------------------------------------------------------------------- meshes and references (built once)
@functools.lru_cache(maxsize=None)
def _grid(cell):
    import thunderbolt_jl_amd as tb
    if cell == "hex":
        return tb.generate_mesh(tb.Hexahedron, (3, 2, 2), (0.0, 0.0, 0.0), (1.0, 0.7, 0.5), perturb=0.2)
    return tref.perturbed_renumbered_box(tb, (2, 2, 2), (0.0, 0.0, 0.0), (1.0, 0.8, 0.6))


def _separate_components(dh):
    """permutation that moves component c of every node into the c-th third of the numbering: no node keeps its three dofs together"""
    d = np.arange(dh.ndofs)
    return ((d % 3) * (dh.ndofs // 3) + d // 3).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _case(cell, order, renumbered=False):
    import thunderbolt_jl_amd as tb
    g = _grid(cell)
    dh = tb.DofHandler(g, tb.LagrangeCollection(order) ** 3)
    if renumbered:
        dh = tb.renumber_dofs(dh, _separate_components(dh))
    return g, dh, tb.allocate_matrix(dh)


def _nodal_density(g):
    x = g.xyz[g.conn]                                           # (cells, vertices, 3): a smooth positive field sampled at the cell's vertices
    return np.ascontiguousarray(1.0 + 0.5 * x[:, :, 0] + 0.25 * x[:, :, 1] * x[:, :, 2])


@functools.lru_cache(maxsize=None)
def _reference(cell, order, nodal, renumbered=False):
    g, dh, sp = _case(cell, order, renumbered)
    kind = {("hex", 1): "hex8", ("hex", 2): "hex27", ("tet", 1): "tet4", ("tet", 2): "tet10"}[(cell, order)]
    nz = nref.assemble_vector_mass(kind, g.xyz, g.conn, dh.cell_dofs, sp.rowptr, sp.colidx, _nodal_density(g) if nodal else 1.7)
    nz.setflags(write=False)
    mask = nref.same_component_mask(dh.cell_dofs, sp.rowptr, sp.colidx)
    return nz, mask


def _mass_operator(tb, device, strategy_name, cell, order, nodal, renumbered=False):
    g, dh, sp = _case(cell, order, renumbered)
    rho = tb.FieldCoefficient(_nodal_density(g)) if nodal else tb.ConstantCoefficient(1.7)
    return tb.setup_operator(getattr(tb, strategy_name)(device), tb.BilinearMassIntegrator(rho), dh, sp)


STRATEGIES = ["AtomicAssemblyStrategy", "PerColorAssemblyStrategy", "ElementAssemblyStrategy", "PatchAssemblyStrategy"]


# ----------------------------------------------------------------------------------------------- 1. vector mass
@pytest.mark.parametrize("nodal", [False, True], ids=["const", "nodal"])
@pytest.mark.parametrize("strategy", STRATEGIES)
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("cell", ["hex", "tet"])
def test_vector_mass_matches_the_reference(tb, device, cell, order, strategy, nodal):
    ref, mask = _reference(cell, order, nodal)
    M = _mass_operator(tb, device, strategy, cell, order, nodal)
    tb.update_operator(M, 0.0)
    got = M.A.to_host()
    err = np.abs(got - ref).max() / np.abs(ref).max()
    print("vector mass %s order %d %s %s: rel-max error %.3e" % (cell, order, strategy, "nodal" if nodal else "const", err))
    assert err <= TOL
    assert np.all(got[~mask] == 0.0)                             # entries that couple different components are exactly 0.0
    assert (~mask).sum() > 0
    if strategy in ("PerColorAssemblyStrategy", "ElementAssemblyStrategy"):
        tb.update_operator(M, 0.0)
        assert np.array_equal(M.A.to_host(), got)               # ordered sums: identical bits


@pytest.mark.parametrize("strategy", ["AtomicAssemblyStrategy", "PerColorAssemblyStrategy"])
@pytest.mark.parametrize("cell,order", [("hex", 1), ("hex", 2), ("tet", 2)])
def test_vector_mass_follows_the_dof_table(tb, device, cell, order, strategy):
    """a numbering that separates a node's three components: the table must not be re-derived as dof = 3·node + c"""
    ref, mask = _reference(cell, order, True, True)
    M = _mass_operator(tb, device, strategy, cell, order, True, True)
    tb.update_operator(M, 0.0)
    got = M.A.to_host()
    assert np.abs(got - ref).max() / np.abs(ref).max() <= TOL
    assert np.all(got[~mask] == 0.0)


def test_scalar_mass_is_unchanged_by_a_vector_assembly(tb, device):
    g = _grid("hex")
    dh = tb.DofHandler(g)
    sp = tb.allocate_matrix(dh)
    for strategy in ("PatchAssemblyStrategy", "PerColorAssemblyStrategy"):
        Ms = tb.setup_operator(getattr(tb, strategy)(device), tb.BilinearMassIntegrator(tb.ConstantCoefficient(1.3)), dh, sp)
        tb.update_operator(Ms, 0.0)
        before = Ms.A.to_host()
        Mv = _mass_operator(tb, device, strategy, "hex", 1, False)
        tb.update_operator(Mv, 0.0)
        tb.update_operator(Ms, 0.0)
        assert np.array_equal(Ms.A.to_host(), before)


def test_vector_diffusion_is_still_refused(tb, device):
    g, dh, sp = _case("hex", 1)
    K = tb.setup_operator(tb.PerColorAssemblyStrategy(device), tb.BilinearDiffusionIntegrator(tb.ConstantCoefficient(1.0)), dh, sp)
    with pytest.raises(tb.TBError):
        tb.update_operator(K, 0.0)


# ----------------------------------------------------------------------------------------------- 2. inertia stage
@functools.lru_cache(maxsize=None)
def _stage_case(order, renumbered):
    import thunderbolt_jl_amd as tb
    g = tb.generate_mesh(tb.Hexahedron, (4, 3, 3), (0.0, 0.0, 0.0), (1.0, 0.8, 0.6), perturb=0.15)
    dh = tb.DofHandler(g, tb.LagrangeCollection(order) ** 3)
    if renumbered:
        dh = tb.renumber_dofs(dh, _separate_components(dh))
    return g, dh, tb.allocate_matrix(dh)


def _kernel_name(tb):
    return tb.lib().tb_last_kernel_name().decode()


def _stage(tb, pat, M, c, u, ut, J, r):
    _check(tb.lib().tb_newmark_stage(pat.h, M.ptr, float(c), None if u is None else u.ptr, None if ut is None else ut.ptr, None if J is None else J.ptr,
                                       None if r is None else r.ptr))


@pytest.mark.parametrize("renumbered", [False, True], ids=["blocks", "general"])
@pytest.mark.parametrize("order", [1, 2])
def test_stage_matches_the_composition(tb, device, order, renumbered):
    g, dh, sp = _stage_case(order, renumbered)
    Mop = tb.setup_operator(tb.PerColorAssemblyStrategy(device), tb.BilinearMassIntegrator(tb.ConstantCoefficient(1.0e3)), dh, sp)
    tb.update_operator(Mop, 0.0)
    pat, M, lib = Mop.pattern, Mop.A, tb.lib()
    if order == 2:
        assert np.diff(sp.rowptr).max() > 64                   # rows that span several waves' worth of lanes
    rng = np.random.default_rng(11)
    n, nnz = dh.ndofs, sp.nnz
    hu, hut, hJ, hr = rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(nnz), rng.standard_normal(n)
    c = 1.0 / (0.25 * 5e-3 ** 2)
    u, ut = device.to_device(hu), device.to_device(hut)
    hM = Mop.A.to_host()
    # the composition the parent commit has: d = u − ũ, r += c·M·d by tb_spmv_csr, J += c·M by tb_axpy over the non-zeros
    d = device.to_device(hu - hut)
    Jref, rref = device.to_device(hJ), device.to_device(hr)
    _check(lib.tb_spmv_csr(pat.h, M.ptr, d.ptr, c, 1.0, rref.ptr))
    _check(lib.tb_axpy(device.h, nnz, c, M.ptr, Jref.ptr))
    Jref, rref = Jref.to_host(), rref.to_host()

    J, r = device.to_device(hJ), device.to_device(hr)
    _stage(tb, pat, M, c, u, ut, J, r)
    name = _kernel_name(tb)
    assert name.startswith("newmark stage composition" if renumbered else "k_newmark_stage_b3"), name
    gJ, gr = J.to_host(), r.to_host()
    eJ, er = np.abs(gJ - Jref).max() / np.abs(Jref).max(), np.abs(gr - rref).max() / np.abs(rref).max()
    print("stage Q%d %s: J %.3e, r %.3e (%s)" % (order, "general" if renumbered else "blocks", eJ, er, name))
    assert eJ <= 1e-14 and er <= 1e-12
    # two calls give identical bits
    J2, r2 = device.to_device(hJ), device.to_device(hr)
    _stage(tb, pat, M, c, u, ut, J2, r2)
    assert np.array_equal(J2.to_host(), gJ) and np.array_equal(r2.to_host(), gr)
    # either output alone
    J3 = device.to_device(hJ)
    _stage(tb, pat, M, c, None, None, J3, None)
    assert np.array_equal(J3.to_host(), gJ)
    r3 = device.to_device(hr)
    _stage(tb, pat, M, c, u, ut, None, r3)
    assert np.array_equal(r3.to_host(), gr)
    assert np.array_equal(Mop.A.to_host(), hM) and np.array_equal(u.to_host(), hu) and np.array_equal(ut.to_host(), hut)   # inputs untouched
    # TB_NEWMARK_STAGE=rows, read at a pattern's first stage call: the fused general kernel on either pattern, held to the same bounds
    os.environ["TB_NEWMARK_STAGE"] = "rows"
    try:
        pat2 = type(pat)(Mop.dmesh, sp)                     # a second device pattern of the same CSR arrays
        J4, r4 = device.to_device(hJ), device.to_device(hr)
        _stage(tb, pat2, M, c, u, ut, J4, r4)
        assert _kernel_name(tb) == "k_newmark_stage_csr"
    finally:
        del os.environ["TB_NEWMARK_STAGE"]
    assert np.abs(J4.to_host() - Jref).max() / np.abs(Jref).max() <= 1e-14
    assert np.abs(r4.to_host() - rref).max() / np.abs(rref).max() <= 1e-12
    _stage(tb, pat, M, c, u, ut, device.to_device(hJ), device.to_device(hr))
    assert _kernel_name(tb) == name                         # the first pattern keeps its decision


def test_stage_takes_the_general_path_on_a_dense_block_pattern_of_separated_components(tb, device):
    """One cell: the pattern is dense, hence a CSR of 3 × 3 blocks under ANY numbering.  With the components separated a triple holds one component of
    three different nodes and the mass blocks are not m·I₃: the dof table, not the structure, must decide — the block kernel must not run."""
    g = tb.generate_mesh(tb.Hexahedron, (1, 1, 1), (0.0, 0.0, 0.0), (1.0, 0.8, 0.6))
    dh = tb.DofHandler(g, tb.LagrangeCollection(1) ** 3)
    dh = tb.renumber_dofs(dh, _separate_components(dh))
    sp = tb.allocate_matrix(dh)
    assert sp.nnz == 24 * 24
    Mop = tb.setup_operator(tb.PerColorAssemblyStrategy(device), tb.BilinearMassIntegrator(tb.ConstantCoefficient(1.0e3)), dh, sp)
    tb.update_operator(Mop, 0.0)
    hM = Mop.A.to_host().reshape(24, 24)
    assert np.abs(hM[0, 1]) > 0                                  # a block that is not a multiple of the identity
    rng = np.random.default_rng(7)
    hu, hut, hJ, hr = rng.standard_normal(24), rng.standard_normal(24), rng.standard_normal(576), rng.standard_normal(24)
    c = 4.0e4
    J, r = device.to_device(hJ), device.to_device(hr)
    _stage(tb, Mop.pattern, Mop.A, c, device.to_device(hu), device.to_device(hut), J, r)
    assert _kernel_name(tb).startswith("newmark stage composition")
    Jw, rw = hJ + c * hM.ravel(), hr + c * (hM @ (hu - hut))
    assert np.abs(J.to_host() - Jw).max() <= 1e-14 * np.abs(Jw).max()
    assert np.abs(r.to_host() - rw).max() <= 1e-12 * np.abs(rw).max()


def test_stage_refuses_bad_arguments(tb, device):
    from thunderbolt_jl_amd import _lib
    g, dh, sp = _stage_case(1, False)
    Mop = tb.setup_operator(tb.PerColorAssemblyStrategy(device), tb.BilinearMassIntegrator(tb.ConstantCoefficient(1.0)), dh, sp)
    tb.update_operator(Mop, 0.0)
    J, r, u, ut = device.zeros(sp.nnz), device.zeros(dh.ndofs), device.zeros(dh.ndofs), device.zeros(dh.ndofs)
    lib = tb.lib()
    assert lib.tb_newmark_stage(None, Mop.A.ptr, 1.0, u.ptr, ut.ptr, J.ptr, r.ptr) == _lib.TB_ERR_BAD_ARG
    for c in (0.0, -1.0, float("inf"), float("nan")):
        assert lib.tb_newmark_stage(Mop.pattern.h, Mop.A.ptr, c, u.ptr, ut.ptr, J.ptr, r.ptr) == _lib.TB_ERR_BAD_ARG
    assert lib.tb_newmark_stage(Mop.pattern.h, None, 1.0, u.ptr, ut.ptr, J.ptr, r.ptr) == _lib.TB_ERR_BAD_ARG
    assert np.all(J.to_host() == 0.0) and np.all(r.to_host() == 0.0)


def test_predict_correct_and_hermite_match_the_formulas(tb, device):
    rng = np.random.default_rng(5)
    n = 1000
    hu, hv, ha, hu1 = rng.standard_normal((4, n))
    u, v, a, u1 = (device.to_device(x) for x in (hu, hv, ha, hu1))
    ut, vt, an, vn, out = (device.zeros(n) for _ in range(5))
    lib = tb.lib()
    for beta, gamma, dt in ((0.25, 0.5, 5e-3), (0.36, 0.7, 0.3)):
        _check(lib.tb_newmark_predict(device.h, n, dt, beta, gamma, u.ptr, v.ptr, a.ptr, ut.ptr, vt.ptr))
        rut, rvt = nref.predict(hu, hv, ha, dt, beta, gamma)
        assert np.array_equal(ut.to_host(), rut) and np.array_equal(vt.to_host(), rvt)       # separately rounded operations in this order
        _check(lib.tb_newmark_correct(device.h, n, dt, beta, gamma, u1.ptr, ut.ptr, vt.ptr, an.ptr, vn.ptr))
        ra, rv = nref.correct(hu1, rut, rvt, dt, beta, gamma)
        assert np.array_equal(an.to_host(), ra) and np.array_equal(vn.to_host(), rv)
        for D in (0, 1, 2):
            for theta in (0.0, 0.37, 1.0):
                _check(lib.tb_hermite_interpolate(device.h, n, theta, dt, D, u.ptr, v.ptr, u1.ptr, a.ptr, out.ptr))
                want = nref.hermite(theta, dt, D, hu, hv, hu1, ha)
                S = sum(abs(c) * np.abs(x) for c, x in zip(nref.hermite_weights(theta, dt, D), (hu, hv, hu1, ha)))
                assert np.all(np.abs(out.to_host() - want) <= 2e-15 * S)    # four terms, fused or not: a few roundings of Σ |cₖ xₖ|
    from thunderbolt_jl_amd import _lib
    assert lib.tb_hermite_interpolate(device.h, n, 0.5, 1.0, 3, u.ptr, v.ptr, u1.ptr, a.ptr, out.ptr) == _lib.TB_ERR_BAD_ARG
    assert lib.tb_newmark_correct(device.h, n, 0.0, 0.25, 0.5, u1.ptr, ut.ptr, vt.ptr, an.ptr, vn.ptr) == _lib.TB_ERR_BAD_ARG


# ----------------------------------------------------------------------------------------------- the bar of test_elastodynamics.jl
def _material(tb):
    return tb.PK1Model(tb.Guccione1991PassiveModel(), tb.ConstantCoefficient(tb.OrthotropicMicrostructure(*ORTHO)))


def _bar(tb, device, ncells=(4, 1, 1), rho=1.0e3, clamped=True, facet_models=(), cell=None, material=None):
    g = tb.generate_mesh(cell or tb.Hexahedron, ncells, (0.0, 0.0, 0.0), (1.0, 0.2, 0.2))
    dh = tb.DofHandler(g, tb.LagrangeCollection(1) ** 3)
    sp = tb.allocate_matrix(dh)
    model = tb.ElastodynamicsModel("d", "v", material or _material(tb), facet_models, tb.ConstantCoefficient(rho))
    X = tb.dof_coordinates(dh)
    ch = tb.ConstraintHandler(dh, np.flatnonzero(X[:, 0] < 1e-12)) if clamped else None
    return model, dh, sp, ch, X


def _bending_velocity(dh, X, ch, amplitude):
    """bending_velocity of test_elastodynamics.jl: transverse (y) velocity growing along the bar, zero on the prescribed dofs"""
    v0 = np.zeros(dh.ndofs)
    ydofs = np.unique(dh.cell_dofs[:, 1::3])
    v0[ydofs] = amplitude * X[ydofs, 0]
    if ch is not None:
        v0[ch.prescribed_dofs] = 0.0
    return v0


def _integrator(tb, device, bar, v0, tend, dt, beta=0.25, gamma=0.5, u0=None, newton=None):
    model, dh, sp, ch, X = bar
    return tb.NewmarkIntegrator(model, dh, sp, ch, tb.ElementAssemblyStrategy(device), u0, v0, (0.0, tend), dt, solver=tb.NewmarkSolver(beta, gamma, newton))


def _approx(x, y, rtol):
    """Julia's isapprox(x, y; rtol) on vectors"""
    return np.linalg.norm(x - y) <= rtol * max(np.linalg.norm(x), np.linalg.norm(y))


# ----------------------------------------------------------------------------------------------- 3. one step satisfies the discrete equations
@pytest.mark.parametrize("cell", ["hex", "tet"])
@pytest.mark.parametrize("beta,gamma", [(0.25, 0.5), (0.36, 0.7)])
def test_one_step_satisfies_the_discrete_equations(tb, device, beta, gamma, cell):
    bar = _bar(tb, device, cell=tb.Tetrahedron if cell == "tet" else tb.Hexahedron)
    model, dh, sp, ch, X = bar
    v0 = _bending_velocity(dh, X, ch, 20.0)
    u0 = np.zeros(dh.ndofs)                                      # a deflected start, so that f_int(u₀) ≠ 0 and a₀ ≠ 0
    ydofs = np.unique(dh.cell_dofs[:, 1::3])
    u0[ydofs] = 0.02 * X[ydofs, 0] ** 2
    u0[ch.prescribed_dofs] = 0.0
    dt, tol = 5e-3, 1e-6
    newton = tb.NewtonRaphsonSolver(max_iter=20, tol=tol, inner_solver="cg", inner_rtol=1e-10, inner_maxiter=20000)
    it = _integrator(tb, device, bar, v0, 1.0, dt, beta, gamma, u0=u0, newton=newton)
    free = ch.free_dofs()
    lib = tb.lib()

    def balance(u, a):
        """M a + f_int(u) by operations that are not the integrator's: tb_residual and tb_spmv_csr with M"""
        f = device.zeros(dh.ndofs)
        tb.residual(it.op, f, u, 0.0)
        Ma = device.zeros(dh.ndofs)
        _check(lib.tb_spmv_csr(it.M.pattern.h, it.M.A.ptr, a.ptr, 1.0, 0.0, Ma.ptr))
        return Ma.to_host() + f.to_host(), f.to_host()

    a0 = it.a.to_host()
    b0, f0 = balance(it.u, it.a)
    assert np.linalg.norm(f0[free]) > 0 and np.linalg.norm(a0) > 0
    print("initial acceleration: |M a0 + f|/|f| on the free dofs %.3e (%d CG iterations)" % (np.linalg.norm(b0[free]) / np.linalg.norm(f0[free]), it.a0_iterations))
    assert np.linalg.norm(b0[free]) <= 1e-10 * np.linalg.norm(f0[free])     # CG to rtol 1e-13 on a mass matrix (condition number of order 10)
    assert np.all(a0[ch.prescribed_dofs] == 0.0)

    assert it.step()
    u1, v1, a1 = it.u.to_host(), it.v.to_host(), it.a.to_host()
    b1, _ = balance(it.u, it.a)
    print("after one step: |M a1 + f_int(u1)| on the free dofs %.3e (Newton tolerance %.1e, %d iterations)" % (np.linalg.norm(b1[free]), tol, newton.iter))
    assert np.linalg.norm(b1[free]) <= tol * (1.0 + 1e-6) + 1e-12 * np.linalg.norm(it.M.A.to_host()) * np.linalg.norm(a1)
    ut, vt = nref.predict(u0, v0, a0, dt, beta, gamma)           # formed on the host
    ra, rv = nref.correct(u1, ut, vt, dt, beta, gamma)
    assert np.abs(a1 - ra).max() <= 1e-13 * np.abs(ra).max()
    assert np.abs(v1 - rv).max() <= 1e-13 * np.abs(rv).max()
    assert np.array_equal(u1[ch.prescribed_dofs], np.zeros(len(ch.prescribed_dofs)))
    assert it.t == dt and it.tprev == 0.0
    # the action of the stage operator includes M/(βΔt²)
    x = device.to_device(np.random.default_rng(2).standard_normal(dh.ndofs))
    y = device.zeros(dh.ndofs)
    tb.update_linearization(it.op, it.u, it.t)                  # J = K alone: the stage operator adds the mass product itself
    it.stage.mul(y, x)
    Kx, Mx = device.zeros(dh.ndofs), device.zeros(dh.ndofs)
    _check(lib.tb_spmv_csr(it.op.pattern.h, it.op.J.ptr, x.ptr, 1.0, 0.0, Kx.ptr))
    _check(lib.tb_spmv_csr(it.op.pattern.h, it.M.A.ptr, x.ptr, 1.0, 0.0, Mx.ptr))
    want = Kx.to_host() + Mx.to_host() / (beta * dt * dt)
    assert np.abs(y.to_host() - want).max() <= 1e-12 * np.abs(want).max()
    res = device.zeros(dh.ndofs)
    it.stage.linearize(it.u, res, it.t, True)                   # J = K + M/(βΔt²), constraints eliminated: the product is J·x, no mass added twice
    it.stage.mul(y, x)
    Jx = device.zeros(dh.ndofs)
    _check(lib.tb_spmv_csr(it.op.pattern.h, it.op.J.ptr, x.ptr, 1.0, 0.0, Jx.ptr))
    assert np.array_equal(y.to_host(), Jx.to_host())
    assert np.abs(y.to_host()[free] - want[free]).max() > 0      # (eliminated columns: not the same product as above)


# ----------------------------------------------------------------------------------------------- 4. replays of the reference's testsets
def test_uniform_translation_is_exact(tb, device):
    bar = _bar(tb, device, clamped=False)
    model, dh, sp, ch, X = bar
    v0 = np.zeros(dh.ndofs)
    for c, val in enumerate((0.3, -0.2, 0.1)):
        v0[np.unique(dh.cell_dofs[:, c::3])] = val
    tend = 0.5
    it = _integrator(tb, device, bar, v0, tend, tend / 2)
    assert it.solve() and it.nsteps == 2 and it.t == tend
    assert _approx(it.u.to_host(), tend * v0, 1e-7)
    assert _approx(it.velocity().to_host(), v0, 1e-7)
    assert np.linalg.norm(it.acceleration().to_host()) < 1e-6


def test_convergence_order_in_time(tb, device):
    tend, dt0 = 0.02, 0.02 / 4

    def run(dt, gamma):
        bar = _bar(tb, device)
        model, dh, sp, ch, X = bar
        it = _integrator(tb, device, bar, _bending_velocity(dh, X, ch, 20.0), tend, dt, gamma=gamma)
        assert it.solve()
        return np.concatenate([it.u.to_host(), it.v.to_host()])  # the reference compares its whole state [d; v]

    reference = run(dt0 / 32, 0.5)

    def observed_order(gamma):
        errors = [np.linalg.norm(run(dt0 / refinement, gamma) - reference) for refinement in (2, 4)]
        assert all(e > 0 for e in errors)
        return float(np.log2(errors[0] / errors[1]))

    o2, o1 = observed_order(0.5), observed_order(0.7)
    print("observed order: gamma = 1/2 %.3f, gamma = 0.7 %.3f" % (o2, o1))
    assert abs(o2 - 2.0) <= 0.15
    assert o1 < 1.5


def test_numerical_dissipation_follows_gamma(tb, device):
    tend, dt = 2.2, 2.5e-2
    decay = []
    for gamma in (0.5, 0.6, 0.7):
        bar = _bar(tb, device, ncells=(2, 1, 1), rho=1.0e-2)
        model, dh, sp, ch, X = bar
        it = _integrator(tb, device, bar, _bending_velocity(dh, X, ch, 0.2), tend, dt, beta=(gamma + 0.5) ** 2 / 4, gamma=gamma)
        first_swing = last_swing = 0.0
        while it.t < tend - 1e-12:
            assert it.step()
            amplitude = np.abs(it.u.to_host()).max()
            if it.t < tend / 3:
                first_swing = max(first_swing, amplitude)
            if it.t > 2 * tend / 3:
                last_swing = max(last_swing, amplitude)
        assert it.nsteps == 88
        decay.append(last_swing / first_swing)
    print("swing-amplitude ratio last third / first third: gamma 0.5 %.4f, 0.6 %.4f, 0.7 %.4f" % tuple(decay))
    assert abs(decay[0] - 1.0) <= 0.05                           # average acceleration: no secular decay
    assert decay[2] < decay[1] < decay[0] - 0.05


def test_the_interpolant_is_hermite_not_linear(tb, device):
    bar = _bar(tb, device, ncells=(2, 1, 1), rho=1.0e-2)
    model, dh, sp, ch, X = bar
    it = _integrator(tb, device, bar, _bending_velocity(dh, X, ch, 0.2), 0.5, 0.005)
    for _ in range(4):
        assert it.step()
    tprev, t = it.tprev, it.t
    tmid = 0.5 * (tprev + t)
    assert np.array_equal(it(tprev).to_host(), it.uprev.to_host())
    assert np.array_equal(it(t).to_host(), it.u.to_host())
    assert np.array_equal(it.velocity(tprev).to_host(), it.vprev.to_host())
    assert np.array_equal(it.velocity(t).to_host(), it.velocity().to_host())
    h = 1e-6
    du = (it(tmid + h).to_host() - it(tmid - h).to_host()) / (2 * h)
    assert _approx(du, it.velocity(tmid).to_host(), 1e-8)
    dv = (it.velocity(tmid + h).to_host() - it.velocity(tmid).to_host()) / h
    assert _approx(dv, it.acceleration(tmid).to_host(), 1e-4)
    uprev, u = it.uprev.to_host(), it.u.to_host()
    linear = uprev + (tmid - tprev) / (t - tprev) * (u - uprev)
    assert not _approx(it(tmid).to_host(), linear, np.sqrt(np.finfo(float).eps))


def test_facet_models_reach_the_assembly(tb, device):
    def run(facet_models):
        bar = _bar(tb, device, ncells=(2, 1, 1), facet_models=facet_models)
        model, dh, sp, ch, X = bar
        it = _integrator(tb, device, bar, _bending_velocity(dh, X, ch, 5.0), 0.05, 0.005)
        assert it.solve()
        return it.u.to_host()

    uf, us = run(()), run((tb.RobinBC(1.0e8, "right"),))
    assert np.linalg.norm(us - uf) / np.linalg.norm(uf) > 0.01


def test_prescribing_the_velocity_is_refused(tb, device):
    model, dh, sp, ch, X = _bar(tb, device, ncells=(2, 1, 1))
    left = np.flatnonzero(X[:, 0] < 1e-12)
    with pytest.raises(ValueError, match="velocity"):
        tb.NewmarkIntegrator(model, dh, sp, [tb.Dirichlet("v", left)], tb.ElementAssemblyStrategy(device), None, None, (0.0, 1.0), 0.1)
    # the same condition on the displacement is what a clamped bar is
    it = tb.NewmarkIntegrator(model, dh, sp, [tb.Dirichlet("d", left)], tb.ElementAssemblyStrategy(device), None, _bending_velocity(dh, X, ch, 0.2), (0.0, 1.0), 0.1)
    assert it.step() and np.all(it.u.to_host()[left] == 0.0)


def test_condensed_models_and_adaptive_stepping_are_refused(tb, device):
    ms = tb.ConstantCoefficient(tb.OrthotropicMicrostructure(*ORTHO))
    active = tb.ActiveStressModel(tb.Guccione1991PassiveModel(), tb.SimpleActiveStress(220.0e3),
                                  tb.CaDrivenInternalSarcomereModel(tb.RDQ20MFModel(), tb.ConstantCoefficient(1.0)), ms)
    for material in (active, tb.LinearMaxwellMaterial()):
        model, dh, sp, ch, X = _bar(tb, device, ncells=(2, 1, 1), material=material)
        with pytest.raises(NotImplementedError):
            tb.NewmarkIntegrator(model, dh, sp, ch, tb.ElementAssemblyStrategy(device), None, None, (0.0, 1.0), 0.1)
    model, dh, sp, ch, X = _bar(tb, device, ncells=(2, 1, 1))
    with pytest.raises(NotImplementedError, match="adaptive"):
        tb.NewmarkIntegrator(model, dh, sp, ch, tb.ElementAssemblyStrategy(device), None, None, (0.0, 1.0), 0.1, adaptive=True)


def test_two_subdomains_carry_their_own_density(tb, device):
    """a density per subdomain is a nodal coefficient: the assembled mass equals the reference with ρ per cell"""
    g = tb.generate_mesh(tb.Hexahedron, (4, 1, 1), (0.0, 0.0, 0.0), (1.0, 0.2, 0.2))
    g.addcellset("left half", lambda x: x[0] <= 0.5)
    g.addcellset("right half", lambda x: x[0] >= 0.5)
    dh = tb.DofHandler(g, tb.LagrangeCollection(1) ** 3)
    sp = tb.allocate_matrix(dh)
    X = tb.dof_coordinates(dh)
    ch = tb.ConstraintHandler(dh, np.flatnonzero(X[:, 0] < 1e-12))
    models = {"left half": tb.ElastodynamicsModel("d", "v", _material(tb), tb.ConstantCoefficient(1.0e3)),
              "right half": tb.ElastodynamicsModel("d", "v", _material(tb), tb.ConstantCoefficient(2.0e3))}
    it = tb.NewmarkIntegrator(models, dh, sp, ch, tb.PerColorAssemblyStrategy(device), None, _bending_velocity(dh, X, ch, 1.0), (0.0, 0.05), 0.005)
    rho = np.where(np.isin(np.arange(g.n_cells), g.getcellset("left half")), 1.0e3, 2.0e3)[:, None] * np.ones((1, 8))
    ref = nref.assemble_vector_mass("hex8", g.xyz, g.conn, dh.cell_dofs, sp.rowptr, sp.colidx, rho)
    assert np.abs(it.M.A.to_host() - ref).max() <= TOL * np.abs(ref).max()
    assert it.solve() and np.all(np.isfinite(it.u.to_host())) and np.linalg.norm(it.u.to_host()) > 0


# ----------------------------------------------------------------------------------------------- 5. a failed solve leaves the state
def test_failed_solve_leaves_the_state(tb, device):
    bar = _bar(tb, device, ncells=(2, 1, 1), rho=1.0e-2)
    model, dh, sp, ch, X = bar
    # a tolerance the Newton cannot reach in two iterations; the loose inner tolerance keeps the increments above machine precision, so the loop
    # cannot leave through its vanishing-increment exit either
    newton = tb.NewtonRaphsonSolver(max_iter=2, tol=1e-30, inner_solver="cg", inner_rtol=1e-2)
    it = _integrator(tb, device, bar, _bending_velocity(dh, X, ch, 0.2), 0.5, 0.02, newton=newton)
    good = tb.NewtonRaphsonSolver(max_iter=20, tol=1e-8, inner_solver="cg", inner_rtol=1e-10)
    it.solver.inner_solver = good
    assert it.step()                                            # one accepted step first: u, v and a are all non-zero
    it.solver.inner_solver = newton
    before = [x.to_host() for x in (it.u, it.v, it.a, it.uprev, it.vprev)], it.t, it.tprev, it.nsteps
    assert all(np.abs(x).max() > 0 for x in before[0][:3])
    assert it.step() is False
    after = [x.to_host() for x in (it.u, it.v, it.a, it.uprev, it.vprev)], it.t, it.tprev, it.nsteps
    assert all(np.array_equal(x, y) for x, y in zip(before[0], after[0])) and before[1:] == after[1:]
    it.solver.inner_solver = good
    assert it.step()                                            # and the integrator carries on from the accepted state


# ----------------------------------------------------------------------------------------------- 6. example
def test_elastodynamics_example_runs():
    env = dict(os.environ, PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "elastodynamics_bar.py")], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "tip deflection" in out.stdout.lower()
