"""Quasi-static viscoelasticity (LinearMaxwellMaterial) on the device against the NumPy reference of tests/viscoelastic_reference.py: parity of K, r and
the viscous strain for every strategy and field, subdomains, the two test sets of the reference that exercise the material
(test/integration/test_solid_mechanics.jl:768-848) replayed, rejected steps, errors, and the how-to."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import viscoelastic_reference as R

pytestmark = pytest.mark.gpu

TOL = 1e-12
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT = 0.05

# the smallest meshes that still have interior nodes, several colours and a partial last group of cells in a workgroup (Q1 / P2: 4 cells per workgroup,
# P1: 16); the two (3, 1, 1) tetrahedral bars (18 cells) add the partial group to the single-launch strategies of the simplex kernels
CASES = {
    "Q1 3x2x2 perturbed": ("hex", 1, (3, 2, 2), 0.2),
    "Q1 5x1x1 bar": ("hex", 1, (5, 1, 1), 0.0),
    "Q2 2x2x1": ("hex", 2, (2, 2, 1), 0.0),
    "P1 2x2x2": ("tet", 1, (2, 2, 2), 0.0),
    "P2 2x2x2": ("tet", 2, (2, 2, 2), 0.0),
    "P1 3x1x1": ("tet", 1, (3, 1, 1), 0.0),
    "P2 3x1x1": ("tet", 2, (3, 1, 1), 0.0),
}


def relmax(got, want):
    return float(np.abs(got - want).max() / np.abs(want).max())


def strategies(tb, device):
    return [tb.AtomicAssemblyStrategy(device), tb.PerColorAssemblyStrategy(device), tb.ElementAssemblyStrategy(device), tb.PatchAssemblyStrategy(device)]


def build(tb, family, order, nel, perturb, left=(0.0, 0.0, 0.0), right=(1.0, 0.8, 0.7)):
    g = tb.generate_mesh(tb.Hexahedron if family == "hex" else tb.Tetrahedron, nel, left, right, perturb=perturb)
    dh = tb.DofHandler(g, tb.LagrangeCollection(order) ** 3)
    return g, dh, tb.allocate_matrix(dh)


def to_device_layout(Q):
    """[cell][q][6] → the device's (6, n_points), point = cell · n_qp + q"""
    return np.ascontiguousarray(Q.reshape(-1, 6).T).ravel()


def operator(tb, device, strategy, mat, dh, sp, Qknown=None, dt=DT, garbage=None):
    op = tb.setup_operator(strategy, tb.QuasiStaticModel("d", mat), dh, sp)
    if Qknown is not None:
        op.internal_known.u.copy_from_host(to_device_layout(Qknown))
    if garbage is not None:
        op.internal.u.copy_from_host(to_device_layout(garbage))
    tb.set_timestep(op, dt)
    return op


@pytest.fixture(scope="module")
def cases(tb):
    """mesh, inputs and the reference's K, r, Q of every case, computed once"""
    mat = R.Maxwell()
    out = {}
    for name, (family, order, nel, perturb) in CASES.items():
        g, dh, sp = build(tb, family, order, nel, perturb)
        rng = np.random.default_rng(11)
        u = rng.uniform(-1e-2, 1e-2, dh.ndofs)
        Q0 = rng.uniform(-1e-2, 1e-2, (g.n_cells, R.n_points(family, order), 6))
        K, r, Q1 = R.assemble(mat, family, order, g.xyz, g.conn, dh.cell_dofs, u, Q0, DT)
        out[name] = dict(family=family, order=order, g=g, dh=dh, sp=sp, u=u, Q0=Q0, K=R.csr_values(K, sp.rowptr, sp.colidx), r=r, Q1=Q1)
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_parity_of_K_r_and_Q_all_strategies(tb, device, cases, name):
    c = cases[name]
    dh, sp, u = c["dh"], c["sp"], device.to_device(c["u"])
    mat = tb.LinearMaxwellMaterial()
    field = name.split()[0]
    for st in strategies(tb, device):
        label = "%s %s" % (name, type(st).__name__)
        # K + r
        op = operator(tb, device, st, mat, dh, sp, c["Q0"])
        res = device.zeros(dh.ndofs)
        tb.update_linearization(op, u, 0.0, residual=res)
        kname = tb.lib().tb_last_kernel_name().decode()
        K, r, Q = op.J.to_host(), res.to_host(), tb.internal_variables(op)
        eK, er, eQ = relmax(K, c["K"]), relmax(r, c["r"]), relmax(Q, c["Q1"])
        print("%s: K %.2e r %.2e Q %.2e  [%s]" % (label, eK, er, eQ, kname))
        assert kname.startswith("k_viscoelastic<%s,K+r>" % field), kname
        assert eK <= TOL and er <= TOL and eQ <= TOL, label
        # K alone
        opk = operator(tb, device, st, mat, dh, sp, c["Q0"])
        tb.update_linearization(opk, u, 0.0)
        assert relmax(opk.J.to_host(), c["K"]) <= TOL and relmax(tb.internal_variables(opk), c["Q1"]) <= TOL, label
        # r alone; the state it leaves equals the linearisation's bit for bit
        opr = operator(tb, device, st, mat, dh, sp, c["Q0"])
        res2 = device.zeros(dh.ndofs)
        tb.residual(opr, res2, u, 0.0)
        assert relmax(res2.to_host(), c["r"]) <= TOL, label
        assert (tb.internal_variables(opr) == Q).all() and (tb.internal_variables(opk) == Q).all(), label
        if isinstance(st, tb.ElementAssemblyStrategy):      # ordered sums: a second assembly gives identical bits
            op2 = operator(tb, device, st, mat, dh, sp, c["Q0"])
            resb = device.zeros(dh.ndofs)
            tb.update_linearization(op2, u, 0.0, residual=resb)
            assert (op2.J.to_host() == K).all() and (resb.to_host() == r).all() and (tb.internal_variables(op2) == Q).all(), label
            tb.update_linearization(op, u, 0.0, residual=res)  # and so does the same operator, over its own previous result
            assert (op.J.to_host() == K).all() and (res.to_host() == r).all() and (tb.internal_variables(op) == Q).all(), label


@pytest.mark.parametrize("name", ["Q1 3x2x2 perturbed", "Q2 2x2x1", "P1 2x2x2", "P2 2x2x2"])
def test_subdomain_accumulates_and_leaves_other_points_alone(tb, device, cases, name):
    c = cases[name]
    g, dh, sp, u = c["g"], c["dh"], c["sp"], device.to_device(c["u"])
    mat = tb.LinearMaxwellMaterial()
    cells = np.arange(g.n_cells, dtype=np.int32)[1::2].copy()            # half the cells
    Kd, rd, Qd = R.assemble(R.Maxwell(), c["family"], c["order"], g.xyz, g.conn, dh.cell_dofs, c["u"], c["Q0"], DT, cells=cells)
    Kd = R.csr_values(Kd, sp.rowptr, sp.colidx)
    rng = np.random.default_rng(5)
    J0, r0 = rng.uniform(-1.0, 1.0, sp.nnz) * np.abs(Kd).max(), rng.uniform(-1.0, 1.0, dh.ndofs) * np.abs(rd).max()
    garbage = rng.uniform(-1.0, 1.0, c["Q0"].shape)
    outside = np.setdiff1d(np.arange(g.n_cells), cells)
    for st in (tb.PerColorAssemblyStrategy(device), tb.AtomicAssemblyStrategy(device)):
        op = operator(tb, device, st, mat, dh, sp, c["Q0"], garbage=garbage)
        tb.check(tb.lib().tb_form_set_cellset(op.form, cells.ctypes.data_as(tb._lib.c_i32p), len(cells), 0))
        tb.check(tb.lib().tb_form_set_accumulate(op.form, 1))
        op.J.copy_from_host(J0)
        res = device.to_device(r0)
        tb.update_linearization(op, u, 0.0, residual=res)
        Q = tb.internal_variables(op)
        # the pre-fill is of the size of the largest entry: its rounding is part of the sum
        assert np.abs(op.J.to_host() - (J0 + Kd)).max() <= TOL * np.abs(Kd).max() and np.abs(res.to_host() - (r0 + rd)).max() <= TOL * np.abs(rd).max()
        assert relmax(Q[cells], Qd[cells]) <= TOL
        assert (Q[outside] == garbage[outside]).all()
        res2 = device.to_device(r0)
        op.internal.u.copy_from_host(to_device_layout(garbage))
        tb.residual(op, res2, u, 0.0)
        assert np.abs(res2.to_host() - (r0 + rd)).max() <= TOL * np.abs(rd).max()
        assert (tb.internal_variables(op)[outside] == garbage[outside]).all()
        tb.check(tb.lib().tb_form_clear_cellset(op.form))
    for st in (tb.ElementAssemblyStrategy(device), tb.PatchAssemblyStrategy(device)):
        op = operator(tb, device, st, mat, dh, sp, c["Q0"])
        tb.check(tb.lib().tb_form_set_cellset(op.form, cells.ctypes.data_as(tb._lib.c_i32p), len(cells), 0))
        with pytest.raises(tb.TBError) as e:
            tb.update_linearization(op, u, 0.0)
        assert e.value.code == tb._lib.TB_ERR_UNSUPPORTED and "TB_STRATEGY_PER_COLOR or TB_STRATEGY_ATOMIC" in str(e.value)


def test_maxwell_subdomain_of_a_dict_model(tb, device):
    """one Maxwell subdomain beside a hyperelastic one in a multi-domain operator: the viscoelastic form accumulates onto the other's J and r"""
    g, dh, sp = build(tb, "hex", 1, (4, 1, 1), 0.0)
    g.addcellset("elastic", np.array([0, 1]))
    g.addcellset("viscous", np.array([2, 3]))
    ms = tb.ConstantCoefficient(tb.OrthotropicMicrostructure(*np.eye(3)))
    models = {"elastic": tb.QuasiStaticModel("d", tb.PK1Model(tb.HolzapfelOgden2009Model(), ms)), "viscous": tb.QuasiStaticModel("d", tb.LinearMaxwellMaterial())}
    rng = np.random.default_rng(2)
    u = rng.uniform(-1e-2, 1e-2, dh.ndofs)
    op = tb.setup_operator(tb.PerColorAssemblyStrategy(device), models, dh, sp)
    assert op.internal is not None and op.internal_form == op.forms[1][0]
    tb.set_timestep(op, DT)
    res = device.zeros(dh.ndofs)
    tb.update_linearization(op, device.to_device(u), 0.0, residual=res)
    ope = tb.setup_operator(tb.PerColorAssemblyStrategy(device), {"elastic": models["elastic"]}, dh, sp)
    rese = device.zeros(dh.ndofs)
    tb.update_linearization(ope, device.to_device(u), 0.0, residual=rese)
    Q0 = np.zeros((g.n_cells, 8, 6))
    Kv, rv, Qv = R.assemble(R.Maxwell(), "hex", 1, g.xyz, g.conn, dh.cell_dofs, u, Q0, DT, cells=[2, 3])
    Kv = R.csr_values(Kv, sp.rowptr, sp.colidx)
    assert np.abs(op.J.to_host() - ope.J.to_host() - Kv).max() <= TOL * np.abs(Kv).max()
    assert np.abs(res.to_host() - rese.to_host() - rv).max() <= TOL * np.abs(rv).max()
    Q = tb.internal_variables(op)
    assert relmax(Q[2:], Qv[2:]) <= TOL and (Q[:2] == 0.0).all()
    with pytest.raises(NotImplementedError):
        tb.setup_operator(tb.PerColorAssemblyStrategy(device), {"elastic": tb.QuasiStaticModel("d", tb.LinearMaxwellMaterial()), "viscous": models["viscous"]}, dh, sp)


def bar_problem(tb, device, nel, strategy, inner_solver="cg"):
    """cells on [−1, 1]³, left face clamped, right face moved by (0.1, 0, 0) — the set-up of both test sets of the reference"""
    g, dh, sp = build(tb, "hex", 1, nel, 0.0, (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
    X = tb.dof_coordinates(dh)
    xdofs = np.unique(dh.cell_dofs[:, 0::3])
    left, right = np.flatnonzero(X[:, 0] < -1 + 1e-12), np.flatnonzero(X[:, 0] > 1 - 1e-12)
    prescribed = np.unique(np.concatenate([left, right]))                  # (the handler keeps its dofs sorted; the values go with that order)
    target = np.zeros(dh.ndofs)
    target[np.intersect1d(right, xdofs)] = 0.1
    ch = tb.ConstraintHandler(dh, prescribed, target[prescribed])
    op = tb.setup_operator(strategy, tb.QuasiStaticModel("d", tb.LinearMaxwellMaterial(E0=70e3, E1=20e3, mu=1e3, eta1=1e3, nu=0.3), ()), dh, sp)
    solver = tb.NewtonRaphsonSolver(max_iter=10, tol=1e-8, inner_solver=inner_solver, inner_rtol=1e-12, inner_maxiter=2000)
    u = device.zeros(dh.ndofs)
    tb.apply(u, ch)
    return g, dh, sp, op, ch, solver, u, prescribed


def test_reference_viscoelasticity_creep(tb, device):
    """test/integration/test_solid_mechanics.jl:768-807: one cell, a creep test in x.  εᵛ₁₁ of the first point never decreases, Newton takes one
    iteration per step (the problem is linear), every step is accepted, the reference's end-state thresholds hold, and every point follows the
    recurrence of the local problem at ε₁₁ = 0.05 (the end values of the issue, computed from the reference's formulas)."""
    g, dh, sp, op, ch, solver, u, _ = bar_problem(tb, device, (1, 1, 1), tb.ElementAssemblyStrategy(device))
    assert tb.solution_size(op) == 3 * 8 + 8 * 6              # the reference's one-point rule gives 3·8 + 1·6; this package integrates Q1 with 2×2×2 points
    rec = R.creep_recurrence(R.Maxwell(), 0.05, 0.1, 10)
    prev = tb.internal_variables(op)[0, 0, 0]
    assert prev == 0.0
    for k in range(10):
        assert tb.perform_mechanics_step(u, op, ch, solver, 0.1 * k, 0.1), (k, solver.residual_norms)
        assert solver.iter == 1 and len(solver.linear_iters) == 1 and len(solver.theta) == 1, (k, solver.iter, solver.residual_norms)
        assert tb.local_solve_failures(op) == 0
        Q = tb.internal_variables(op)
        assert Q.shape == (1, 8, 6)
        assert prev <= Q[0, 0, 0]
        prev = Q[0, 0, 0]
        assert np.abs(Q - rec[k + 1]).max() <= 1e-13, (k, np.abs(Q - rec[k + 1]).max())
    assert abs(Q[0, 0, 0] - 0.05) <= 1e-5 and np.abs(Q[0, 0, 1:]).max() <= 1e-5            # the reference's own thresholds
    assert np.abs(Q[0, :, 0] - 0.04999699936779986).max() <= 1e-13
    assert np.abs(Q[0, :, [3, 5]] - 1.4999026457761e-06).max() <= 1e-13 and np.abs(Q[0, :, [1, 2, 4]]).max() <= 1e-13
    assert (tb.internal_variables(op) == op.internal_known.to_host().reshape(6, 1, 8).transpose(1, 2, 0)).all()


def test_reference_internal_variables_are_stored_per_cell(tb, device):
    """test/integration/test_solid_mechanics.jl:809-848: 2×1×1 cells, three steps of 0.1 — every cell's block of internal variables is non-zero — and,
    beyond the reference's check, u and Q equal the NumPy dense-solve stepper.  Inner CG at rtol 1e-12.  Tolerance: the larger of 1e-9 and ten times
    what the reference stepper itself moves when its linear solve is perturbed at 1e-12 relative (≈ 1e-13 here, so 1e-9 holds).
    Measured on MI355X: |u − u_ref| = |Q − Q_ref| = 1.4e-17; the reference moves by 2.5e-15 under the perturbation; the tolerance is 1e-9."""
    g, dh, sp, op, ch, solver, u, prescribed = bar_problem(tb, device, (2, 1, 1), tb.PerColorAssemblyStrategy(device))
    mat = R.Maxwell()
    rng = np.random.default_rng(0)

    def perturbed(A, b):
        x = np.linalg.solve(A, b)
        return x * (1.0 + 1e-12 * rng.uniform(-1.0, 1.0, x.shape))
    ur = up = u.to_host()
    Qr = Qp = np.zeros((2, 8, 6))
    for k in range(3):
        assert tb.perform_mechanics_step(u, op, ch, solver, 0.1 * k, 0.1), (k, solver.residual_norms, solver.linear_failure)
        assert solver.iter == 1
        ur, Qr, rleft = R.step(mat, "hex", 1, g.xyz, g.conn, dh.cell_dofs, ur, Qr, 0.1, prescribed)
        up, Qp, _ = R.step(mat, "hex", 1, g.xyz, g.conn, dh.cell_dofs, up, Qp, 0.1, prescribed, solve=perturbed)
    Q = tb.internal_variables(op)
    assert Q.shape == (2, 8, 6) and all(np.abs(Q[c]).max() > 0.0 for c in range(2))
    moved = max(np.abs(ur - up).max(), np.abs(Qr - Qp).max())
    tol = max(1e-9, 10.0 * moved)
    du, dQ = np.abs(u.to_host() - ur).max(), np.abs(Q - Qr).max()
    print("per-cell replay: |u - u_ref| %.2e |Q - Q_ref| %.2e; the reference moves %.2e under a 1e-12 perturbation of its solve; tolerance %.2e" % (du, dQ, moved, tol))
    assert du <= tol and dQ <= tol


def dense_solver(pattern, J, res, du):
    n = len(pattern.sp.rowptr) - 1
    A = np.zeros((n, n))
    rows = np.repeat(np.arange(n), np.diff(pattern.sp.rowptr))
    A[rows, pattern.sp.colidx] = J.to_host()
    du.copy_from_host(np.linalg.solve(A, res.to_host()))
    return 1


def test_rejected_step_restores_the_state_and_the_retry_reproduces_the_step(tb, device):
    st = tb.ElementAssemblyStrategy(device)
    g, dh, sp, op, ch, solver, u, _ = bar_problem(tb, device, (2, 1, 1), st, inner_solver=dense_solver)
    assert tb.perform_mechanics_step(u, op, ch, solver, 0.0, 0.1)
    assert tb.perform_mechanics_step(u, op, ch, solver, 0.1, 0.1)
    uA, QA = u.to_host(), op.internal.to_host()
    # the same two steps with an assembly at another displacement and its rejection in between
    g, dh, sp, op, ch, solver, u, _ = bar_problem(tb, device, (2, 1, 1), st, inner_solver=dense_solver)
    assert tb.perform_mechanics_step(u, op, ch, solver, 0.0, 0.1)
    known = op.internal_known.to_host()
    trial = device.to_device(u.to_host() + np.random.default_rng(1).uniform(-1e-2, 1e-2, dh.ndofs))
    tb.update_linearization(op, trial, 0.2)
    assert (op.internal.to_host() != known).any()
    tb.reject_internal_state(op)
    assert (op.internal.to_host() == known).all() and (op.internal_known.to_host() == known).all()
    assert tb.perform_mechanics_step(u, op, ch, solver, 0.1, 0.1)
    assert (u.to_host() == uA).all() and (op.internal.to_host() == QA).all()


def raw_form(tb, dh, device, params=(70e3, 20e3, 1e3, 1e3, 0.3), qorder=0):
    dm = dh.device_mesh(device)
    p = np.array(params, dtype=np.float64)
    form = C.c_void_p()
    rc = tb.lib().tb_viscoelastic_create(dm.h, qorder, p.ctypes.data_as(tb._lib.c_dp), len(p), C.byref(form))
    return rc, form, dm


def test_errors(tb, device, cases):
    L, lib = tb._lib, tb.lib()
    c = cases["Q1 3x2x2 perturbed"]
    g, dh, sp, u = c["g"], c["dh"], c["sp"], device.to_device(c["u"])
    mat = tb.LinearMaxwellMaterial()
    # assembling without a state, setting a non-positive time step
    op = tb.setup_operator(tb.PerColorAssemblyStrategy(device), tb.QuasiStaticModel("d", mat), dh, sp)
    res = device.zeros(dh.ndofs)
    for call in (lambda: tb.update_linearization(op, u, 0.0, residual=res), lambda: tb.residual(op, res, u, 0.0)):
        with pytest.raises(tb.TBError) as e:
            call()
        assert e.value.code == L.TB_ERR_BAD_ARG and "no internal state set" in str(e.value)
    for dt in (0.0, -1.0, float("nan")):
        with pytest.raises(tb.TBError) as e:
            tb.set_timestep(op, dt)
        assert e.value.code == L.TB_ERR_BAD_ARG and "time step must be positive" in str(e.value)
    # creation: parameters, scalar field, quadrature order
    for bad in ((np.nan, 20e3, 1e3, 1e3, 0.3), (70e3, 20e3, 1e3, 0.0, 0.3), (-1.0, 20e3, 1e3, 1e3, 0.3), (70e3, -1.0, 1e3, 1e3, 0.3), (70e3, 20e3, 1e3, 1e3, 0.5),
                (70e3, 20e3, 1e3, 1e3, -1.0), (70e3, 20e3, 1e3, 1e3)):
        assert raw_form(tb, dh, device, bad)[0] == L.TB_ERR_BAD_ARG and lib.tb_last_error_string()
    assert raw_form(tb, tb.DofHandler(g), device)[0] == L.TB_ERR_BAD_ARG
    assert raw_form(tb, dh, device, qorder=3)[0] == L.TB_ERR_BAD_ARG
    rc, form, dm = raw_form(tb, dh, device, (70e3, 0.0, 1e3, 1e3, 0.3))        # E₁ = 0 is the purely elastic material
    assert rc == L.TB_OK
    # what accepts the form and what refuses it
    npts = C.c_int64()
    assert lib.tb_hyperelastic_n_quadrature_points(form, C.byref(npts)) == L.TB_OK and npts.value == g.n_cells * 8
    nf, status = C.c_int64(-1), np.full(npts.value, 7, dtype=np.int32)
    assert lib.tb_hyperelastic_local_solve_report(form, C.byref(nf), status.ctypes.data, len(status)) == L.TB_OK
    assert nf.value == 0 and (status == L.TB_LOCAL_SUCCESS).all()
    assert lib.tb_hyperelastic_local_solve_report(form, C.byref(nf), status.ctypes.data, len(status) - 1) == L.TB_ERR_BAD_ARG
    nine = np.eye(3).ravel()
    seventeen = np.zeros(17)
    pat = dm.pattern(sp)
    refused = [lib.tb_hyperelastic_set_active_tension(form, 1.0, None, 0), lib.tb_hyperelastic_set_hill(form, None),
               lib.tb_hyperelastic_set_prestress(form, nine.ctypes.data_as(L.c_dp)),
               lib.tb_hyperelastic_set_condensation(form, L.TB_SARCOMERE_RDQ20MF, seventeen.ctypes.data_as(L.c_dp), 17, 1.0, 1e-4, 10),
               lib.tb_hyperelastic_set_previous_solution(form, u.ptr), lib.tb_facet_assemble(form, pat.h, u.ptr, 0.0, op.J.ptr, res.ptr),
               lib.tb_chamber_assemble(form, pat.h, u.ptr, 0.0, op.J.ptr, res.ptr, None, None, None), lib.tb_assemble_matrix(form, pat.h, L.TB_STRATEGY_ATOMIC, 0.0, op.J.ptr),
               lib.tb_assemble_vector(form, L.TB_STRATEGY_ATOMIC, 0.0, res.ptr)]
    ecg = C.c_void_p()
    refused.append(lib.tb_ecg_create(form, C.byref(ecg)))
    assert refused == [L.TB_ERR_BAD_ARG] * len(refused), refused
    # E₁ = 0 on the device: εᵛ₁ = εᵛ₀ bit for bit and the elastic tangent
    Q0 = np.random.default_rng(3).uniform(-1e-2, 1e-2, (g.n_cells, 8, 6))
    ope = operator(tb, device, tb.ElementAssemblyStrategy(device), tb.LinearMaxwellMaterial(E1=0.0), dh, sp, Q0)
    tb.update_linearization(ope, u, 0.0, residual=res)
    assert (tb.internal_variables(ope) == Q0).all()
    Ke, re_, _ = R.assemble(R.Maxwell(E1=0.0), "hex", 1, g.xyz, g.conn, dh.cell_dofs, c["u"], Q0, DT)
    assert relmax(ope.J.to_host(), R.csr_values(Ke, sp.rowptr, sp.colidx)) <= TOL and relmax(res.to_host(), re_) <= TOL
    assert lib.tb_form_destroy(form) == L.TB_OK


@pytest.mark.parametrize("family,order", [("hex", 1), ("hex", 2), ("tet", 1), ("tet", 2)])
def test_inverted_cell_and_nan_coordinate_are_reported(tb, device, family, order):
    g, _, _ = build(tb, family, order, (2, 2, 2), 0.0)
    mat = tb.LinearMaxwellMaterial()
    cell = 5
    bad = tb.Grid(g.cell_kind, g.xyz, g.conn.copy())
    if family == "hex":
        bad.conn[cell] = bad.conn[cell][[1, 0, 3, 2, 5, 4, 7, 6]]       # mirrored in its first direction
    else:
        bad.conn[cell, [1, 2]] = bad.conn[cell, [2, 1]]
    nan = tb.Grid(g.cell_kind, g.xyz.copy(), g.conn)
    nan.xyz[g.conn[cell, 0], 1] = np.nan
    for grid, named in ((bad, True), (nan, False)):
        dh = tb.DofHandler(grid, tb.LagrangeCollection(order) ** 3)
        sp = tb.allocate_matrix(dh)
        for st in (tb.ElementAssemblyStrategy(device), tb.AtomicAssemblyStrategy(device)):
            op = operator(tb, device, st, mat, dh, sp)
            with pytest.raises(tb.TBError) as e:
                tb.update_linearization(op, device.zeros(dh.ndofs), 0.0, residual=device.zeros(dh.ndofs))
            assert e.value.code == tb._lib.TB_ERR_NEG_DETJ
            if named:
                assert "cell %d" % cell in str(e.value) or str(cell) in str(e.value)
            with pytest.raises(tb.TBError) as e:
                tb.residual(op, device.zeros(dh.ndofs), device.zeros(dh.ndofs), 0.0)
            assert e.value.code == tb._lib.TB_ERR_NEG_DETJ


def test_newmark_still_refuses_the_material(tb, device):
    g, dh, sp = build(tb, "hex", 1, (2, 1, 1), 0.0)
    model = tb.ElastodynamicsModel("d", "v", tb.LinearMaxwellMaterial(), tb.ConstantCoefficient(1.0))
    with pytest.raises(NotImplementedError):
        tb.NewmarkIntegrator(model, dh, sp, [], tb.ElementAssemblyStrategy(device), None, None, (0.0, 1.0), 0.1)


def test_the_example_runs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "viscoelastic_creep.py")], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads(out.stdout.strip().splitlines()[-1])
    assert d["all_accepted"] and d["newton_iterations_per_step"] == 1 and d["monotone"]
    assert abs(d["viscous_strain_11"][-1] - 0.05) <= 1e-5
