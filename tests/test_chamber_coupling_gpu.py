"""3D-0D chamber coupling on the device: tb_chamber_assemble against the NumPy checker (tests/chamber_reference.py), self-consistency that does
not lean on the checker, closed forms, the status paths, the bordered Schur solve, volume control by the blocked Newton and a fragment of a
coupled heart beat.  The all-hex ventricle generator needs a circumferential count divisible by 4: the smallest ventricle is (8, 1, 2)."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import chamber_reference as ref

pytestmark = pytest.mark.gpu

TOL = 1e-12
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SGN = ref.HEX_SGN
P = 0.7


def relmax(got, want):
    return float(np.abs(np.asarray(got) - np.asarray(want)).max() / np.abs(want).max())


def dof_positions(dh, g, order):
    """position of the node behind every dof (through the trilinear map) and the component the dof stands for"""
    xi = SGN if order == 1 else ref.HEX27_TIX - 1.0
    N = 0.125 * np.prod(1.0 + SGN[None, :, :] * xi[:, None, :], axis=2)
    pos = np.einsum("ba,cak->cbk", N, g.xyz[g.conn])
    X, comp = np.empty((dh.ndofs, 3)), np.empty(dh.ndofs, dtype=np.int64)
    for c in range(3):
        X[dh.cell_dofs[:, c::3].ravel()] = pos.reshape(-1, 3)
        comp[dh.cell_dofs[:, c::3].ravel()] = c
    return X, comp


def field_at_dofs(V, comp):
    return np.ascontiguousarray(V[np.arange(len(comp)), comp])


def smooth_displacement(X, comp, seed, amp):
    """seeded smooth field, amplitude amp·L with wavelengths of about 3 L: |∇u| ≲ 2π·0.35·1.2·√3·amp ≈ 0.1 at amp = 0.02, so det F > 0 everywhere"""
    rng = np.random.default_rng(seed)
    k, ph = rng.uniform(0.3, 1.2, (3, 3)), rng.uniform(0, 2 * np.pi, 3)
    L = np.ptp(X, axis=0).max()
    return field_at_dofs(amp * L * np.sin(X @ k.T * (2 * np.pi / L) * 0.35 + ph), comp)


class Case:
    def __init__(self, tb, device, g, facets, order, seed):
        self.g, self.order, self.facets = g, order, np.ascontiguousarray(facets, dtype=np.int32)
        self.dh = tb.DofHandler(g, tb.LagrangeCollection(order) ** 3)
        self.sp = tb.allocate_matrix(self.dh)
        self.dmesh = self.dh.device_mesh(device)
        self.pattern = self.dmesh.pattern(self.sp)
        self.X, self.comp = dof_positions(self.dh, g, order)
        self.u = smooth_displacement(self.X, self.comp, seed, 0.02)
        self.du = device.to_device(self.u)
        self.refs = {}

    def reference(self, name, nq):
        key = (name, nq)
        if key not in self.refs:
            method = ref.RSAFDQ2022((0.0, 1.0, 0.0), (0.0, 0.0, -0.1)) if name == "rsafdq" else ref.Hirschvogel2017()
            o = ref.assemble(self.g.xyz, self.g.conn, self.dh.cell_dofs, self.order, self.facets, nq, self.u, P, method)
            o["nz"] = ref.scatter_csr(o["Ke"], self.sp.rowptr, self.sp.colidx)
            self.refs[key] = o
        return self.refs[key]


@pytest.fixture(scope="module")
def cases(tb, device):
    lv = tb.generate_ideal_lv_mesh_hex(8, 1, 2, inner_radius=3.9 * 0.7, outer_radius=3.9, longitudinal_upper=0.4, apex_inner=3.9 * 1.3, apex_outer=3.9 * 1.5)
    box = tb.generate_mesh(tb.Hexahedron, (3, 2, 2), (0, 0, 0), (1.0, 0.8, 0.7), perturb=0.15)
    bf = box.boundary_facets()
    assert set(bf[:, 1].tolist()) == set(range(6)) and np.bincount(bf[:, 0]).max() >= 3      # every local face; corner cells carry three facets
    out = {}
    for order in (1, 2):
        out["lv", order] = Case(tb, device, lv, lv.facetset("Endocardium"), order, 11)
        out["box", order] = Case(tb, device, box, bf, order, 12)
    return out


def method_of(tb, name):
    return tb.RSAFDQ2022SurrogateVolume() if name == "rsafdq" else tb.Hirschvogel2017SurrogateVolume()


def run(tb, device, case, method, nq, p=P, u=None, outputs=("nz", "r", "col", "row", "volume"), repeat=1):
    form = tb.ChamberForm(case.dmesh, case.facets, method, nq)
    n = case.dh.ndofs
    bufs = {"nz": device.zeros(case.sp.nnz), "r": device.zeros(n), "col": device.zeros(n), "row": device.zeros(n), "volume": device.zeros(1)}
    kw = {("nzval" if k == "nz" else k): bufs[k] for k in outputs}
    for _ in range(repeat):
        form.assemble(case.du if u is None else u, p, pattern=case.pattern if "nz" in outputs else None, **kw)
    return {k: bufs[k].to_host() for k in outputs}


@pytest.mark.parametrize("name", ["rsafdq", "hirschvogel"])
@pytest.mark.parametrize("order,nq", [(1, 2), (2, 3)])
@pytest.mark.parametrize("mesh", ["lv", "box"])
def test_kernel_parity(tb, device, cases, mesh, order, nq, name):
    case = cases[mesh, order]
    want = case.reference(name, nq)
    got = run(tb, device, case, method_of(tb, name), nq)
    errs = {k: relmax(got[k], want[k]) for k in ("col", "row", "r", "nz")}
    errs["volume"] = abs(got["volume"][0] - want["volume"]) / abs(want["volume"])
    print(mesh, order, name, errs)
    assert max(errs.values()) < TOL, errs
    twice = run(tb, device, case, method_of(tb, name), nq, repeat=2)      # the call ADDS to its outputs
    for k in got:                                            # up to the order of the atomic additions (a few dozen terms per entry at 1.1e-16 each)
        assert relmax(twice[k], 2.0 * got[k]) < 1e-13, k


@pytest.mark.parametrize("order", [1, 2])
def test_self_consistency(tb, device, cases, order):
    case = cases["lv", order]
    m = tb.RSAFDQ2022SurrogateVolume()
    r1 = run(tb, device, case, m, 0, p=1.0, outputs=("r", "col"))
    r0 = run(tb, device, case, m, 0, p=0.0, outputs=("r",))
    assert relmax(r1["r"] - r0["r"], r1["col"]) < 1e-13
    # the follower-load tangent is the one tb_facet_assemble adds for TB_BC_PRESSURE with param = p on the same facets
    got = run(tb, device, case, m, 0, outputs=("nz", "r"))
    h = C.c_void_p()
    L = tb._lib
    tb._lib.check(tb.lib().tb_facet_form_create(case.dmesh.h, L.TB_BC_PRESSURE, P, 0, case.facets.ctypes.data_as(L.c_i32p), len(case.facets), 0, C.byref(h)))
    nz, r = device.zeros(case.sp.nnz), device.zeros(case.dh.ndofs)
    tb._lib.check(tb.lib().tb_facet_assemble(h, case.pattern.h, case.du.ptr, 0.0, nz.ptr, r.ptr))
    tb.lib().tb_form_destroy(h)
    assert relmax(got["nz"], nz.to_host()) < 1e-13 and relmax(got["r"], r.to_host()) < 1e-13
    # row · δ against the central difference of the device volume
    for name in ("rsafdq", "hirschvogel"):
        row = run(tb, device, case, method_of(tb, name), 0, outputs=("row",))["row"]
        rng = np.random.default_rng(5)
        for _ in range(3):
            d = rng.uniform(-1, 1, case.dh.ndofs)
            d /= np.linalg.norm(d)
            eps = 1e-6 * np.linalg.norm(case.u)
            vp = run(tb, device, case, method_of(tb, name), 0, u=device.to_device(case.u + eps * d), outputs=("volume",))["volume"][0]
            vm = run(tb, device, case, method_of(tb, name), 0, u=device.to_device(case.u - eps * d), outputs=("volume",))["volume"][0]
            fd = (vp - vm) / (2 * eps)
            assert abs(row @ d - fd) < 1e-6 * abs(fd), (name, row @ d, fd)


@pytest.mark.parametrize("order,nq", [(1, 1), (1, 2), (2, 3)])
def test_closed_form_on_the_device(tb, device, order, nq):
    """all six faces of an a×b×c box under u = (A − I)x: RSAFDQ2022 with unit h and any b gives −det(A)·abc, Hirschvogel −3·det(A)·abc"""
    a, b, c = 1.3, 0.7, 0.9
    g = tb.generate_mesh(tb.Hexahedron, (3, 2, 2), (0, 0, 0), (a, b, c))
    case = Case(tb, device, g, g.boundary_facets(), order, 0)
    A = np.array([[1.10, 0.05, -0.03], [0.02, 0.93, 0.04], [-0.06, 0.01, 1.07]])
    u = device.to_device(field_at_dofs(case.X @ (A - np.eye(3)).T, case.comp))
    vol = np.linalg.det(A) * a * b * c
    h = np.array([1.0, 2.0, -0.5]) / np.linalg.norm([1.0, 2.0, -0.5])
    for bb in ([0.0, 0.0, -0.1], [0.3, -1.2, 0.8]):
        got = run(tb, device, case, tb.RSAFDQ2022SurrogateVolume(h, bb), nq, u=u, outputs=("volume", "col"))
        assert abs(got["volume"][0] + vol) < 1e-12 * vol
        assert np.abs(got["col"].reshape(-1, 3).sum(axis=0)).max() < 1e-12       # closed surface: no resultant of a uniform pressure
    got = run(tb, device, case, tb.Hirschvogel2017SurrogateVolume(), nq, u=u, outputs=("volume",))
    assert abs(got["volume"][0] + 3.0 * vol) < 1e-12 * vol
    assert abs(tb.compute_chamber_volume(case.dh, u, g.boundary_facets(), tb.Hirschvogel2017SurrogateVolume()) + 3.0 * vol) < 1e-12 * vol


def test_errors(tb, device, cases):
    L = tb._lib
    gt = tb.generate_mesh(tb.Tetrahedron, (2, 2, 2), (0, 0, 0), (1, 1, 1))
    dht = tb.DofHandler(gt, tb.LagrangeCollection(1) ** 3)
    with pytest.raises(tb.TBError) as e:
        tb.ChamberForm(dht.device_mesh(device), gt.boundary_facets()[:4], tb.RSAFDQ2022SurrogateVolume())
    assert e.value.code == L.TB_ERR_UNSUPPORTED and "tetrahedra" in str(e.value)
    case = cases["box", 1]
    with pytest.raises(tb.TBError) as e:
        tb.ChamberForm(case.dmesh, [[case.g.n_cells, 0]], tb.RSAFDQ2022SurrogateVolume())
    assert e.value.code == L.TB_ERR_BAD_ARG and "out of range" in str(e.value)
    with pytest.raises(tb.TBError) as e:
        tb.ChamberForm(case.dmesh, [[0, 6]], tb.RSAFDQ2022SurrogateVolume())
    assert e.value.code == L.TB_ERR_BAD_ARG
    with pytest.raises(tb.TBError) as e:
        tb.ChamberForm(case.dmesh, case.facets, tb.RSAFDQ2022SurrogateVolume(), 4)
    assert e.value.code == L.TB_ERR_BAD_ARG and "Gauss" in str(e.value)
    h = C.c_void_p()
    assert tb.lib().tb_chamber_form_create(case.dmesh.h, 7, None, 0, case.facets.ctypes.data_as(L.c_i32p), len(case.facets), 0, C.byref(h)) == L.TB_ERR_BAD_ARG
    # an inverted displacement (F = −1.5 I) raises the negative-Jacobian status; nothing stays poisoned: the next valid call gives the valid answer
    good = run(tb, device, case, tb.RSAFDQ2022SurrogateVolume(), 2, outputs=("volume", "row"))
    with pytest.raises(tb.TBError) as e:
        run(tb, device, case, tb.RSAFDQ2022SurrogateVolume(), 2, u=device.to_device(field_at_dofs(-2.5 * case.X, case.comp)), outputs=("volume", "row"))
    assert e.value.code == L.TB_ERR_NEG_DETJ
    again = run(tb, device, case, tb.RSAFDQ2022SurrogateVolume(), 2, outputs=("volume", "row"))
    # equal up to the order of the atomic additions (a few dozen terms per entry at 1.1e-16 each), as for the repeated call of the parity test
    assert relmax(again["row"], good["row"]) < 1e-13 and abs(again["volume"][0] - good["volume"][0]) < 1e-13 * abs(good["volume"][0])
    with pytest.raises(ValueError):
        tb.ChamberForm(case.dmesh, case.facets, tb.ConstantChamberVolume(1.0))


def node_dofs(dh, g, nodes):
    nd0 = np.empty(g.n_nodes, dtype=np.int64)
    nd0[g.conn.ravel()] = dh.cell_dofs[:, : 3 * 8: 3].ravel()
    return (nd0[np.asarray(nodes)][:, None] + np.arange(3)).ravel()


def bordered_system(tb, device):
    """3×3×3 Q1 box, x = 0 clamped, Holzapfel–Ogden tangent at a small load, one chamber on the opposite face, linearised"""
    g = tb.generate_mesh(tb.Hexahedron, (3, 3, 3), (0, 0, 0), (1.0, 1.0, 1.0))
    dh = tb.DofHandler(g, tb.LagrangeCollection(1) ** 3)
    sp = tb.allocate_matrix(dh)
    fsn = tb.ConstantCoefficient(tb.OrthotropicMicrostructure([1, 0, 0], [0, 1, 0], [0, 0, 1]))
    op = tb.setup_operator(tb.ElementAssemblyStrategy(device), tb.QuasiStaticModel("d", tb.PK1Model(tb.HolzapfelOgden2009Model(), fsn)), dh, sp)
    ch = tb.ConstraintHandler(dh, node_dofs(dh, g, np.flatnonzero(g.xyz[:, 0] < 1e-12)))
    form = tb.ChamberForm(op.dmesh, g.facetset("right"), tb.RSAFDQ2022SurrogateVolume((1.0, 0.0, 0.0), (0.0, 0.0, 0.0)))
    system = tb.BlockedChamberSystem(op, ch, [tb.ChamberTying(form, None, "right", 0.9)])
    system.p[:] = 0.3
    X, comp = dof_positions(dh, g, 1)
    uh = smooth_displacement(X, comp, 4, 0.01)
    uh[ch.prescribed_dofs] = 0.0
    u, res = device.to_device(uh), device.zeros(dh.ndofs)
    system.linearize(u, res, 0.0, True)
    system.u0 = uh                                           # the linearisation point (host)
    return dh, sp, op, ch, system, res


def test_bordered_solve(tb, device):
    """3×3×3 Q1 box, x = 0 clamped, Holzapfel–Ogden tangent at a small load, one chamber on the opposite face: the device Schur solution
    [Δd; Δp] against numpy.linalg.solve on the dense (n + 1)² matrix built from the downloaded CSR values, col and row"""
    dh, sp, op, ch, system, res = bordered_system(tb, device)
    n = dh.ndofs
    J = np.zeros((n + 1, n + 1))
    nz = op.J.to_host()
    for i in range(n):
        J[i, sp.colidx[sp.rowptr[i]:sp.rowptr[i + 1]]] = nz[sp.rowptr[i]:sp.rowptr[i + 1]]
    col, row = system.cols[0].to_host(), system.rows[0].to_host()
    assert np.all(col[ch.prescribed_dofs] == 0.0) and np.all(row[ch.prescribed_dofs] == 0.0) and np.abs(col).max() > 0 and np.abs(row).max() > 0
    J[:n, n], J[n, :n] = col, row
    b = np.r_[res.to_host(), system.r_p]
    want = np.linalg.solve(J, b)
    ls = tb.SchurComplementLinearSolver("gmres", rtol=1e-12, maxiter=20000, gmres_restart=100)
    d, dp, ok = ls.solve((op.pattern, op.J), system.cols, system.rows, None, res, system.r_p)
    assert ok and len(ls.inner_iters) == 2
    got = np.r_[d.to_host(), dp]
    print("bordered solve rel err", np.linalg.norm(got - want) / np.linalg.norm(want), "dp", dp, want[-1])
    assert np.linalg.norm(got - want) < 1e-8 * np.linalg.norm(want)
    assert abs(dp[0] - want[-1]) < 1e-8 * abs(want[-1])


def test_strict_inner_solve_on_the_blocked_system(tb, device):
    """an inner GMRES cut off after three iterations: the Schur solver fails by default and carries on with strict=False, and
    BlockedChamberSystem.solve_increment reports it the way nlsolve's strict_inner_solve branch reads it"""
    dh, sp, op, ch, system, res = bordered_system(tb, device)
    u0 = system.u0
    ls = tb.SchurComplementLinearSolver("gmres", rtol=1e-12, maxiter=3, gmres_restart=3)
    A = ((op.pattern, op.J), system.cols, system.rows, None, res, system.r_p)
    d, dp, ok = ls.solve(*A)
    assert not ok and d is None and dp is None and "above its tolerance" in ls.failure and len(ls.inner_iters) == 1
    d, dp, ok = ls.solve(*A, strict=False)
    assert ok and ls.inexact and ls.residual > 0.0 and len(ls.inner_iters) == 2 and np.isfinite(dp).all() and np.isfinite(d.to_host()).all()
    du = device.zeros(dh.ndofs)
    kw = dict(inner_solver=tb.SchurComplementLinearSolver("gmres"), inner_rtol=1e-12, inner_maxiter=3, gmres_restart=3)
    its, lres, converged = system.solve_increment(tb.NewtonRaphsonSolver(strict_inner_solve=False, **kw), res, du, 1e-12)
    assert not converged and lres > 0.0 and 0 < its <= 6 and np.abs(du.to_host()).max() > 0.0     # an inexact increment, residual norm reported
    its, lres, converged = system.solve_increment(tb.NewtonRaphsonSolver(**kw), res, du, 1e-12)
    assert not converged and lres is None and "above its tolerance" in system.failure_detail  # no increment: the step fails
    # through the loop: the strict solver fails the step and says why, the lenient one applies the inexact increments and records the event
    # (one iteration from the linearisation point, the chamber asked to shrink by 0.1 %: max_iter = 0 ends the loop after one increment)
    system.chambers[0].V0D = 0.999 * system.V3D[0]
    for strict in (True, False):
        solver = tb.NewtonRaphsonSolver(max_iter=0, tol=1e-30, strict_inner_solve=strict, **kw)
        u = device.to_device(u0)
        system.p[:] = 0.3
        assert not tb.nlsolve(u, op, ch, solver, t=0.0, system=system)
        assert "above its tolerance" in solver.linear_failure and len(solver.linear_iters) == 1
        assert (np.abs(u.to_host() - u0).max() > 0.0) == (not strict) and (system.p[0] != 0.3) == (not strict)
    with pytest.raises(TypeError, match="blocked"):
        tb.nlsolve(device.zeros(dh.ndofs), op, ch, tb.NewtonRaphsonSolver(**kw), t=0.0)       # a blocked solver without its blocked system


def test_volume_control(tb, device):
    """ideal LV (8, 1, 2), passive Guccione, base clamped, V0D = 0.95·V3D(0): the blocked Newton meets the volume; the converged pressure
    applied as ConstantPressureBC through the uncoupled nlsolve (code that predates the coupling) reproduces the displacement"""
    g = tb.generate_ideal_lv_mesh_hex(8, 1, 2)
    f, s, n = tb.ideal_lv_microstructure(g)
    dh = tb.DofHandler(g, tb.LagrangeCollection(1) ** 3)
    sp = tb.allocate_matrix(dh)
    cm = tb.PK1Model(tb.Guccione1991PassiveModel(), tb.OrthotropicMicrostructureModel(f, s, n))
    base_nodes = np.unique(g.conn[g.facetset("Base")[:, 0]][:, list(g.HEX_FACETS[5])])
    ch = tb.ConstraintHandler(dh, node_dofs(dh, g, base_nodes))
    strategy = tb.ElementAssemblyStrategy(device)
    method = tb.RSAFDQ2022SurrogateVolume()
    V0 = tb.compute_chamber_volume(dh, device.zeros(dh.ndofs), "Endocardium", method)
    assert V0 > 0
    circuit = tb.DummyLumpedCircuitModel(lambda t: 0.95 * V0)
    coupler = tb.LumpedFluidSolidCoupler([tb.ChamberVolumeCoupling("Endocardium", "lv-volume-control", method, "V", "p", "p")], "d")
    fun = tb.semidiscretize_rsafdq(tb.RSAFDQ2022Split(tb.RSAFDQ2022Model(tb.QuasiStaticModel("d", cm), circuit, coupler)), strategy, dh, sp, ch)
    assert abs(fun.chambers[0].V0D - V0) < 1e-13 * V0        # create_chamber_tyings: V0D starts at the volume of the undeformed mesh
    fun.chambers[0].V0D = float(circuit.default_initial_state()[0])
    # the residual mixes forces and a volume: its norm may rise once before the quadratic phase, so monotonicity is not enforced (Θ is still recorded)
    solver = tb.NewtonRaphsonSolver(max_iter=30, tol=1e-9 * V0, inner_solver=tb.SchurComplementLinearSolver("gmres"), inner_rtol=1e-12, inner_maxiter=20000,
                                    gmres_restart=200, enforce_monotonic_convergence=False)
    assert tb.nlsolve(fun.u, fun.op, ch, solver, t=0.0, system=fun.system), (solver.residual_norms, solver.linear_failure)
    V = fun.system.V3D[0]                                    # of the last linearisation, which is at the converged displacement
    print("volume control: p", fun.pressures, "V3D", V, "V0D", 0.95 * V0, "theta", solver.theta, "rnorm", solver.residual_norms)
    assert abs(V - 0.95 * V0) <= 1e-8 * 0.95 * V0
    assert solver.theta[-1] < 0.1
    # cross-check: the same pressure as a prescribed follower load, uncoupled Newton from u = 0
    op2 = tb.setup_operator(strategy, tb.QuasiStaticModel("d", cm, (tb.ConstantPressureBC(float(fun.pressures[0]), "Endocardium"),)), dh, sp)
    u2 = device.zeros(dh.ndofs)
    s2 = tb.NewtonRaphsonSolver(max_iter=30, tol=1e-9 * V0, inner_solver="gmres", inner_rtol=1e-12, inner_maxiter=20000, gmres_restart=200)
    assert tb.nlsolve(u2, op2, ch, s2, t=0.0), (s2.residual_norms, s2.linear_failure)
    a, b = fun.u.to_host(), u2.to_host()
    print("cross-check rel diff", np.linalg.norm(a - b) / np.linalg.norm(b))
    assert np.linalg.norm(a - b) < 1e-6 * np.linalg.norm(b)


def test_condensed_internal_variables_are_refused(tb, device):
    g = tb.generate_mesh(tb.Hexahedron, (2, 2, 2), (0, 0, 0), (1, 1, 1))
    dh = tb.DofHandler(g, tb.LagrangeCollection(1) ** 3)
    fsn = tb.ConstantCoefficient(tb.OrthotropicMicrostructure([1, 0, 0], [0, 1, 0], [0, 0, 1]))
    cm = tb.ActiveStressModel(tb.HolzapfelOgden2009Model(), tb.SimpleActiveStress(), tb.CaDrivenInternalSarcomereModel(tb.AsRateIndependent(tb.RDQ20MFModel()), lambda t: 0.5), fsn)
    coupler = tb.LumpedFluidSolidCoupler([tb.ChamberVolumeCoupling("right", "c", tb.RSAFDQ2022SurrogateVolume(), "V", "p", "p")], "d")
    model = tb.RSAFDQ2022Model(tb.QuasiStaticModel("d", cm), tb.DummyLumpedCircuitModel(lambda t: 1.0), coupler)
    with pytest.raises(ValueError, match="internal variables"):
        tb.semidiscretize_rsafdq(tb.RSAFDQ2022Split(model), tb.ElementAssemblyStrategy(device), dh, tb.allocate_matrix(dh), tb.ConstraintHandler(dh, [0]))


def test_coupled_heartbeat_fragment(tb, device):
    """examples/lv_3d0d.py's set-up for five steps of 1 ms: every Newton solve succeeds, |V3D − V0D| stays within the Newton tolerance, all
    values finite, and the circuit state moves (test_fsi.jl:59-60)"""
    spec = importlib.util.spec_from_file_location("lv_3d0d", os.path.join(ROOT, "examples", "lv_3d0d.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    fun, integrator, u0fluid = ex.setup(tb, device)
    newton = integrator.chamber_solver.inner_solver
    iv = fun.chambers[0].volume_index
    for k in range(5):
        v0d = float(fun.circuit_state[iv])
        assert integrator.step(1.0), (k, newton.residual_norms, newton.linear_failure)
        # the residual of the last linearisation is ‖[r_d; V3D − V0D]‖ < tol, and the volume row is one entry of it
        print("t %.1f p %.6e V3D %.8e V0D %.8e newton %d" % (integrator.t, fun.pressures[0], fun.V3D[0], v0d, newton.iter))
        assert abs(fun.V3D[0] - v0d) <= newton.tol
        assert np.isfinite(fun.pressures).all() and np.isfinite(fun.circuit_state).all() and np.isfinite(fun.u.to_host()).all()
    assert not np.allclose(fun.circuit_state, u0fluid)
    assert abs(integrator.t - 5.0) < 1e-12
