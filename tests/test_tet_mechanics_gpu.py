"""Tetrahedral mechanics on the device (P1 / P2 tetrahedra) against the NumPy reference of tests/tet_reference.py: parity of r and K for every
strategy, consistency of the tangent, closed forms, weak boundary conditions, status, bit reproducibility and the Land 2015 beam on tetrahedra."""
import os
import subprocess
import sys

import numpy as np
import pytest

import tet_reference as ref

pytestmark = pytest.mark.gpu

TOL = 1e-12
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HO_P = [0.059, 8.023, 18.472, 16.026, 2.581, 11.120, 0.216, 11.436]
GUCCIONE_P = [0.1, 29.8, 14.9, 14.9, 9.3, 19.2, 14.4]
NEL, LEFT, RIGHT = (4, 3, 3), (0.0, 0.0, 0.0), (1.0, 0.8, 0.7)


def relmax(got, want):
    return float(np.abs(got - want).max() / np.abs(want).max())


def strategies(tb, device):
    return [tb.AtomicAssemblyStrategy(device), tb.PerColorAssemblyStrategy(device), tb.ElementAssemblyStrategy(device), tb.PatchAssemblyStrategy(device)]


def frame():
    f = np.array([1.0, 2.0, 0.5]) / np.linalg.norm([1.0, 2.0, 0.5])
    s = np.cross(f, [0.0, 0.0, 1.0]); s /= np.linalg.norm(s)
    return np.array([f, s, np.cross(f, s)])


def models(tb, kind, fsn, fsn_field=None, act=None):
    """(device constitutive model, reference material)"""
    ms = tb.ConstantCoefficient(tb.OrthotropicMicrostructure(*fsn)) if fsn_field is None else tb.OrthotropicMicrostructureModel(fsn_field[:, :, 0], fsn_field[:, :, 1], fsn_field[:, :, 2])
    if kind == "ho":
        mat, rm = tb.HolzapfelOgden2009Model(), ref.Material(0, 0, HO_P, [1.0], fsn, fsn_field)
    else:
        mat = tb.Guccione1991PassiveModel(*GUCCIONE_P, mpU=tb.SimpleCompressionPenalty(100.0))
        rm = ref.Material(8, 0, GUCCIONE_P, [100.0], fsn, fsn_field)
    if act is None:
        return tb.PK1Model(mat, ms), rm
    tmax, field = act
    rm.tension, rm.act_field = tmax, field
    return tb.ActiveStressModel(mat, tb.SimpleActiveStress(tmax), tb.CaDrivenInternalSarcomereModel(tb.PelceSunLangeveld1995Model(), field), ms), rm


@pytest.fixture(scope="module")
def mesh(tb):
    g = ref.perturbed_renumbered_box(tb, NEL, LEFT, RIGHT)
    assert (ref.volumes(g.xyz, g.conn) > 0).all()            # nodes moved by ≤ 0.15 h: no cell inverts
    out = {}
    for order in (1, 2):
        dh = tb.DofHandler(g, tb.LagrangeCollection(order) ** 3)
        out[order] = (g, dh, tb.allocate_matrix(dh))
    return out


def device_Kr(tb, device, strategy, cm, dh, sp, u, facets=()):
    op = tb.setup_operator(strategy, tb.QuasiStaticModel("u", cm, facets), dh, sp)
    res = device.zeros(dh.ndofs)
    tb.update_linearization(op, device.to_device(u), 0.0, residual=res)
    name = tb.lib().tb_last_kernel_name().decode()
    return op.J.to_host(), res.to_host(), name


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("kind", ["ho", "guccione"])
def test_parity_with_the_reference_all_strategies(tb, oracle, device, mesh, order, kind):
    g, dh, sp = mesh[order]
    u = np.random.default_rng(0).uniform(-1e-2, 1e-2, dh.ndofs)
    cm, rm = models(tb, kind, frame())
    Kref, rref = ref.assemble(oracle, order, g.xyz, g.conn, dh.cell_dofs, u, rm, sp.rowptr, sp.colidx)
    for st in strategies(tb, device):
        K, r, name = device_Kr(tb, device, st, cm, dh, sp, u)
        eK, er = relmax(K, Kref), relmax(r, rref)
        print("P%d %s %s: K %.2e r %.2e  [%s]" % (order, kind, type(st).__name__, eK, er, name))
        assert "k_tet_mech<P%d" % order in name
        assert eK <= TOL and er <= TOL, (type(st).__name__, eK, er)
        # residual-only call
        op = tb.setup_operator(st, tb.QuasiStaticModel("u", cm), dh, sp)
        res = device.zeros(dh.ndofs)
        tb.residual(op, res, device.to_device(u), 0.0)
        assert relmax(res.to_host(), rref) <= TOL


@pytest.mark.parametrize("order", [1, 2])
def test_parity_nodal_fibre_field_and_active_stress(tb, oracle, device, mesh, order):
    g, dh, sp = mesh[order]
    rng = np.random.default_rng(3)
    u = np.random.default_rng(0).uniform(-1e-2, 1e-2, dh.ndofs)
    # nodal frames: the constant frame tilted a little, differently at every grid node (continuous field, per cell and geometry node)
    tilt = frame()[None, :, :] + 0.2 * rng.uniform(-1.0, 1.0, (g.n_nodes, 3, 3))
    fsn_field = np.ascontiguousarray(tilt[g.conn])                          # (n_cells, 4, 3 vectors, 3)
    cm, rm = models(tb, "ho", frame(), fsn_field=fsn_field)
    Kref, rref = ref.assemble(oracle, order, g.xyz, g.conn, dh.cell_dofs, u, rm, sp.rowptr, sp.colidx)
    ca = np.ascontiguousarray(rng.uniform(0.2, 1.0, g.n_nodes)[g.conn])     # (n_cells, 4)
    cma, rma = models(tb, "guccione", frame(), act=(0.5, ca))
    Kra, rra = ref.assemble(oracle, order, g.xyz, g.conn, dh.cell_dofs, u, rma, sp.rowptr, sp.colidx)
    cmh, rmh = models(tb, "ho", frame(), act=(0.5, ca))                     # hand-derived path with active stress
    Krh, rrh = ref.assemble(oracle, order, g.xyz, g.conn, dh.cell_dofs, u, rmh, sp.rowptr, sp.colidx)
    for st in strategies(tb, device):
        for label, model, Kw, rw in (("fibre field", cm, Kref, rref), ("active stress AD", cma, Kra, rra), ("active stress HO", cmh, Krh, rrh)):
            K, r, name = device_Kr(tb, device, st, model, dh, sp, u)
            print("P%d %s %s: K %.2e r %.2e  [%s]" % (order, label, type(st).__name__, relmax(K, Kw), relmax(r, rw), name))
            assert relmax(K, Kw) <= TOL and relmax(r, rw) <= TOL, (label, type(st).__name__)


def test_parity_on_the_reference_tetrahedron_mesh(tb, oracle, device):
    g = tb.meshio.load_mfem_grid(os.path.join(ROOT, "tests", "golden", "meshes", "mfem", "ref-tetrahedron.mesh")).grid(tb.meshio.TETRAHEDRON)
    for order in (1, 2):
        dh = tb.DofHandler(g, tb.LagrangeCollection(order) ** 3)
        sp = tb.allocate_matrix(dh)
        u = np.random.default_rng(0).uniform(-1e-2, 1e-2, dh.ndofs)
        cm, rm = models(tb, "guccione", frame())
        Kref, rref = ref.assemble(oracle, order, g.xyz, g.conn, dh.cell_dofs, u, rm, sp.rowptr, sp.colidx)
        for st in strategies(tb, device):
            K, r, _ = device_Kr(tb, device, st, cm, dh, sp, u)
            assert relmax(K, Kref) <= TOL and relmax(r, rref) <= TOL


def dofs_from_positions(dh, disp):
    u = np.empty(dh.ndofs)
    for c in range(3):
        d = dh.cell_dofs[:, c::3].ravel()
        u[d] = disp[d, c]
    return u


@pytest.mark.parametrize("order", [1, 2])
def test_tangent_consistency_against_the_reference_discrepancy(tb, oracle, device, mesh, order):
    g, dh, sp = mesh[order]
    rng = np.random.default_rng(0)
    u = rng.uniform(-1e-2, 1e-2, dh.ndofs)
    v = rng.uniform(-1.0, 1.0, dh.ndofs)
    h = 1e-6
    cm, rm = models(tb, "guccione", frame())
    Kref, _ = ref.assemble(oracle, order, g.xyz, g.conn, dh.cell_dofs, u, rm, sp.rowptr, sp.colidx)
    rp = ref.assemble(oracle, order, g.xyz, g.conn, dh.cell_dofs, u + h * v, rm)[1]
    rmn = ref.assemble(oracle, order, g.xyz, g.conn, dh.cell_dofs, u - h * v, rm)[1]
    d_ref = np.abs(ref.csr_matvec(sp.rowptr, sp.colidx, Kref, v) - (rp - rmn) / (2 * h)).max()
    st = tb.PatchAssemblyStrategy(device)
    K, _, _ = device_Kr(tb, device, st, cm, dh, sp, u)
    op = tb.setup_operator(st, tb.QuasiStaticModel("u", cm), dh, sp)
    res = device.zeros(dh.ndofs)
    dp = tb.residual(op, res, device.to_device(u + h * v), 0.0).to_host().copy()
    dm = tb.residual(op, res, device.to_device(u - h * v), 0.0).to_host().copy()
    d_dev = np.abs(ref.csr_matvec(sp.rowptr, sp.colidx, K, v) - (dp - dm) / (2 * h)).max()
    print("P%d K·v vs central difference: device %.3e, reference %.3e" % (order, d_dev, d_ref))
    assert d_dev <= 10.0 * d_ref


@pytest.mark.parametrize("order", [1, 2])
def test_rigid_rotation_and_patch_test(tb, oracle, device, mesh, order):
    from test_tet_mechanics_host import interior_dofs
    g, dh, sp = mesh[order]
    X = tb.dof_coordinates(dh)
    cm, rm = models(tb, "ho", frame())
    th = 0.3
    R = np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1.0]])
    G = np.array([[0.02, 0.01, 0.0], [0.0, -0.015, 0.005], [0.01, 0.0, 0.03]])
    for label, A, dofs in (("rigid rotation", R - np.eye(3), np.arange(dh.ndofs)), ("affine stretch", G, interior_dofs(g, dh))):
        u = dofs_from_positions(dh, X @ A.T)
        ref.assemble(oracle, order, g.xyz, g.conn, dh.cell_dofs, u, rm, sp.rowptr, sp.colidx)
        bound = 1e-12 * ref.assemble.kmax * np.abs(u).max()
        assert len(dofs) > 0
        for st in strategies(tb, device):
            _, r, _ = device_Kr(tb, device, st, cm, dh, sp, u)
            print("P%d %s %s: max |r| %.3e (bound %.3e)" % (order, label, type(st).__name__, np.abs(r[dofs]).max(), bound))
            assert np.abs(r[dofs]).max() <= bound


@pytest.mark.parametrize("order", [1, 2])
def test_facet_terms(tb, oracle, device, order):
    g = tb.generate_mesh(tb.Tetrahedron, (3, 2, 2), (0.0, 0.0, 0.0), (1.5, 1.0, 0.8))
    dh = tb.DofHandler(g, tb.LagrangeCollection(order) ** 3)
    sp = tb.allocate_matrix(dh)
    st = tb.PatchAssemblyStrategy(device)
    null = tb.PK1Model(tb.NullEnergyModel(), tb.ConstantCoefficient(tb.OrthotropicMicrostructure(*np.eye(3))))   # Ψ = 0: the volume term adds exact zeros

    def facet_only(bc, u):
        """device facet contribution = (volume + facet) − volume, both assembled on the device"""
        K1, r1, _ = device_Kr(tb, device, st, null, dh, sp, u, (bc,))
        K0, r0, _ = device_Kr(tb, device, st, null, dh, sp, u)
        return K1 - K0, r1 - r0
    p = 0.7
    fs = g.facetset("top")
    # u = 0: the volume residual vanishes identically, so the residual is the facet term alone
    _, r, _ = device_Kr(tb, device, st, null, dh, sp, np.zeros(dh.ndofs), (tb.PressureFieldBC(tb.ConstantCoefficient(p), "top"),))
    _, rref = ref.assemble_facets(order, g.xyz, g.conn, dh.cell_dofs, fs, np.zeros(dh.ndofs), "pressure", p)
    assert np.abs(r - rref).max() <= 1e-12 * np.abs(rref).max()
    tot = np.array([r[c::3].sum() for c in range(3)])
    assert np.allclose(tot, p * 1.5 * 1.0 * np.array([0.0, 0.0, 1.0]), rtol=0, atol=1e-13)     # p · A · n (sign as on hexahedra: + p n at u = 0)
    X = tb.dof_coordinates(dh)
    on_top = np.flatnonzero(X[:, 2] == 0.8)[2::3]                                # z-dofs on the face
    Af = 0.5 * (1.5 / 3) * (1.0 / 2)
    is_vertex = np.zeros(dh.ndofs, dtype=bool)
    is_vertex[dh.cell_dofs[:, :12].ravel()] = True
    for d in on_top:
        ncell = sum(1 for c, lf in fs if d in dh.cell_dofs[c])
        want = ncell * p * Af / 3.0 if (order == 1 or not is_vertex[d]) else 0.0
        assert abs(r[d] - want) <= 1e-14, (d, r[d], want)
    # pressure tangent with u ≠ 0: against the central difference, the reference's own discrepancy as yardstick
    rng = np.random.default_rng(0)
    u = rng.uniform(-1e-2, 1e-2, dh.ndofs)
    v = rng.uniform(-1.0, 1.0, dh.ndofs)
    h = 1e-6
    bc = tb.PressureFieldBC(tb.ConstantCoefficient(p), "top")
    Kf, rf = facet_only(bc, u)
    Kfr, rfr = ref.assemble_facets(order, g.xyz, g.conn, dh.cell_dofs, fs, u, "pressure", p, sp.rowptr, sp.colidx)
    assert np.abs(Kf - Kfr).max() <= 1e-10 * np.abs(Kfr).max() and np.abs(rf - rfr).max() <= 1e-10 * np.abs(rfr).max()   # (differences of two assemblies)
    rp = ref.assemble_facets(order, g.xyz, g.conn, dh.cell_dofs, fs, u + h * v, "pressure", p)[1]
    rm = ref.assemble_facets(order, g.xyz, g.conn, dh.cell_dofs, fs, u - h * v, "pressure", p)[1]
    d_ref = np.abs(ref.csr_matvec(sp.rowptr, sp.colidx, Kfr, v) - (rp - rm) / (2 * h)).max()
    dp = facet_only(bc, u + h * v)[1]
    dm = facet_only(bc, u - h * v)[1]
    d_dev = np.abs(ref.csr_matvec(sp.rowptr, sp.colidx, Kf, v) - (dp - dm) / (2 * h)).max()
    print("P%d pressure tangent vs central difference: device %.3e, reference %.3e" % (order, d_dev, d_ref))
    assert d_dev <= 10.0 * d_ref
    # Robin and normal spring are linear in u: r = K u
    for bc, name, par in ((tb.RobinBC(3.0, "left"), "robin", 3.0), (tb.NormalSpringBC(3.0, "right"), "spring", 3.0)):
        Kf, rf = facet_only(bc, u)
        Ku = ref.csr_matvec(sp.rowptr, sp.colidx, Kf, u)
        Kfr, rfr = ref.assemble_facets(order, g.xyz, g.conn, dh.cell_dofs, g.facetset(bc.boundary_name), u, name, par, sp.rowptr, sp.colidx)
        print("P%d %s: |r − K u| %.3e, K vs reference %.3e" % (order, name, np.abs(rf - Ku).max() / np.abs(Ku).max(), np.abs(Kf - Kfr).max() / np.abs(Kfr).max()))
        assert np.abs(rf - Ku).max() <= 1e-12 * max(np.abs(Ku).max(), np.abs(Kf).max() * np.abs(u).max())
        assert np.abs(Kf - Kfr).max() <= 1e-10 * np.abs(Kfr).max()


def test_inverted_tetrahedron_is_reported_and_the_next_call_succeeds(tb, device):
    g = tb.generate_mesh(tb.Tetrahedron, (2, 2, 2), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    bad = tb.Grid(tb.Tetrahedron, g.xyz, g.conn.copy())
    bad.conn[17, [1, 2]] = bad.conn[17, [2, 1]]
    cm = tb.PK1Model(tb.HolzapfelOgden2009Model(), tb.ConstantCoefficient(tb.OrthotropicMicrostructure(*np.eye(3))))
    st = tb.PatchAssemblyStrategy(device)
    dhb = tb.DofHandler(bad, tb.LagrangeCollection(2) ** 3)
    with pytest.raises(tb.TBError) as e:
        device_Kr(tb, device, st, cm, dhb, tb.allocate_matrix(dhb), np.zeros(dhb.ndofs))
    assert e.value.code == tb._lib.TB_ERR_NEG_DETJ and "17" in str(e.value)
    dh = tb.DofHandler(g, tb.LagrangeCollection(2) ** 3)
    K, r, _ = device_Kr(tb, device, st, cm, dh, tb.allocate_matrix(dh), np.zeros(dh.ndofs))
    assert np.isfinite(K).all() and np.abs(r).max() <= 1e-13


def test_element_strategy_is_bit_reproducible_on_tetrahedra(tb, device, mesh):
    g, dh, sp = mesh[2]
    u = np.random.default_rng(0).uniform(-1e-2, 1e-2, dh.ndofs)
    cm, _ = models(tb, "guccione", frame())
    st = tb.ElementAssemblyStrategy(device)
    K1, r1, _ = device_Kr(tb, device, st, cm, dh, sp, u)
    K2, r2, _ = device_Kr(tb, device, st, cm, dh, sp, u)
    assert K1.tobytes() == K2.tobytes() and r1.tobytes() == r2.tobytes()


def test_unsupported_on_tetrahedra_says_so(tb, device, mesh):
    g, dh, sp = mesh[2]
    with pytest.raises(tb.TBError) as e:
        tb.setup_operator(tb.PatchAssemblyStrategy(device), tb.QuasiStaticModel("u", tb.PK1Model(tb.HolzapfelOgden2009Model(), tb.ConstantCoefficient(
            tb.OrthotropicMicrostructure(*np.eye(3)))), (tb.BendingSpringBC(1.0, np.array([[0, 0]], dtype=np.int32)),)), dh, sp)
    assert e.value.code == tb._lib.TB_ERR_UNSUPPORTED and "tetrahedra" in str(e.value)


def test_land2015_benchmark_problem_1_on_tetrahedra(tb, oracle, device):
    """test/validation/land2015.jl with celltype = Tetrahedron: the twin of test_reference_validation_land2015_benchmark_problem_1 (same material, load
    path and solver) on generate_mesh(Tetrahedron, (25, 3, 3), …) with a quadratic displacement.  (a) the NumPy reference residual (volume + pressure) at
    the converged device solution is below the Newton tolerance on the free dofs; (b) the reference's assertion: tip deflection 3.17 ± 0.02."""
    import scipy.sparse as ssp
    import scipy.sparse.linalg as sla
    g = tb.generate_mesh(tb.Tetrahedron, (25, 3, 3), (0.0, 0.0, 0.0), (10.0, 1.0, 1.0))
    dh = tb.DofHandler(g, tb.LagrangeCollection(2) ** 3)
    sp = tb.allocate_matrix(dh)
    mat = tb.Guccione1991PassiveModel(C0=2.0, Bff=8.0, Bss=2.0, Bnn=2.0, Bns=1.0, Bfs=2.0, Bfn=2.0, mpU=tb.SimpleCompressionPenalty(100.0))
    ms = tb.ConstantCoefficient(tb.OrthotropicMicrostructure([1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0]))
    load = (tb.PressureFieldBC(lambda t: min(t, 1.0) * 0.004, "bottom"),)
    op = tb.setup_operator(tb.ElementAssemblyStrategy(device), tb.QuasiStaticModel("displacement", tb.PK1Model(mat, ms), load), dh, sp)
    X = tb.dof_coordinates(dh)
    fixed = np.flatnonzero(X[:, 0] < 1e-12)
    ch = tb.ConstraintHandler(dh, fixed)

    def sparse_lu(pattern, J, res, du):
        n = len(pattern.sp.rowptr) - 1
        A = ssp.csr_matrix((J.to_host(), pattern.sp.colidx, pattern.sp.rowptr), shape=(n, n))
        du.copy_from_host(sla.splu(A.tocsc()).solve(res.to_host()))
        return 1
    u = device.zeros(dh.ndofs)
    newton = tb.NewtonRaphsonSolver(tol=1e-4, max_iter=10, inner_solver=sparse_lu)
    path = tb.HomotopyPathSolver(newton)
    t, dt = 0.0, 0.2
    while t < 1.0 - 1e-12:
        h = min(dt, 0.2, 1.0 - t)
        assert path.solve(u, op, ch, (t, t + h), h, adaptive=True, maxiters=100), path.steps
        t += h
    uh = u.to_host()
    rm = ref.Material(8, 0, [2.0, 8.0, 2.0, 2.0, 1.0, 2.0, 2.0], [100.0], np.eye(3))
    _, rv = ref.assemble(oracle, 2, g.xyz, g.conn, dh.cell_dofs, uh, rm)
    _, rf = ref.assemble_facets(2, g.xyz, g.conn, dh.cell_dofs, g.facetset("bottom"), uh, "pressure", 0.004)
    free = np.setdiff1d(np.arange(dh.ndofs), fixed)
    rnorm = np.linalg.norm((rv + rf)[free])
    tip = np.flatnonzero((np.abs(X[:, 0] - 10.0) < 1e-9) & (np.abs(X[:, 1] - 0.5) < 1e-9) & (np.abs(X[:, 2] - 1.0) < 1e-9))
    zdofs = [d for d in tip if d % 3 == 2]
    assert len(zdofs) == 1
    deflection = uh[zdofs[0]]
    print("Land 2015 problem 1 on tetrahedra: reference residual on the free dofs %.3e, tip deflection %.4f (reference asserts 3.17 ± 0.02), %d load steps"
          % (rnorm, deflection, len(path.steps)))
    assert rnorm < 1e-4, rnorm
    assert abs(deflection - 3.17) <= 0.02, deflection


def test_land2015_example_runs_on_tetrahedra():
    env = dict(os.environ, PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "land2015_beam.py"), "--cell", "tet"], capture_output=True, text=True, env=env, timeout=900)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert "tet" in out.stdout.lower()
