"""Device eikonal solver (tb_eikonal_*, thunderbolt.jl_amd/eikonal.py) against exact plane waves and the NumPy fixed point of tests/eikonal_reference.py.

Yardstick.  REFERENCE_SPREAD is the largest difference between the Gauss–Seidel (forward, reversed) and Jacobi fixed points of the reference on the
meshes used here (tests/test_eikonal_cpu.py::test_reference_sweep_orders_reach_one_fixed_point prints it): 0.0 on all six.  The device is compared
with the reference at max(10 · REFERENCE_SPREAD, 1e-12 · max T): the floor covers what separates the two arithmetics — the device contracts
multiply–adds, NumPy does not, and the device accepts an update only beyond rtol·t (RTOL = 1e-14 here, so that the values it declines, summed
along a path of at most ~30 nodes, stay below the floor).
Measured on the device (max |T − reference| / max T, sweeps): hex_5x4x3 2.1e-16 (8), tet_3x3x2 2.2e-16 (4), hex_11x10x9_fibres 5.4e-15 (21),
hex_1 8.2e-17 (2); plane waves at most 4.7e-15; largest |residual| / T 7.6e-15 at RTOL = 1e-14; corner source: maximum error 0.0519 at 4³ and
0.0362 at 8³.  Every test prints its figures before it asserts.
"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import eikonal_reference as ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REFERENCE_SPREAD = 0.0
RTOL = 1e-14


def tolerance(Tmax):
    return max(10.0 * REFERENCE_SPREAD, 1e-12 * Tmax)


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def grid_of(tb, kind, xyz, conn):
    return tb.Grid(tb.Hexahedron if kind == "hex" else tb.Tetrahedron, xyz, conn)


def coefficient_of(tb, c):
    if "fibres" in c:
        f, s, n = c["fibres"]
        return tb.SpectralTensorCoefficient(tb.OrthotropicMicrostructureModel(f, s, n), tb.ConstantCoefficient(np.array(c["lam"])))
    return tb.ConstantCoefficient(np.asarray(c["G"], dtype=float))


def node_values(tb, dh, v):
    """a dof vector on the host → values at the grid nodes"""
    return np.asarray(v)[tb.ecg.vertex_dofs(dh)]


_solved = {}


def solved(tb, device, name):
    """(case, dh, cache, T at the nodes): every case is solved once per session"""
    if name not in _solved:
        c = ref.case(name)
        dh = tb.DofHandler(grid_of(tb, c["kind"], c["xyz"], c["conn"]))
        cache = tb.EikonalActivationCache(device, tb.EikonalModel(coefficient_of(tb, c)), dh)
        T = tb.solve_activation(cache, c["sources"], times=c["times"], rtol=RTOL)
        _solved[name] = (c, dh, cache, node_values(tb, dh, T.to_host()))
    return _solved[name]


# ------------------------------------------------------------------------------------------------ 1. plane waves
PLANE_TENSORS = [2.0 * np.eye(3), np.diag([9.0, 1.0, 1.0]), np.diag([1.0, 4.0, 1.0])]


@pytest.mark.parametrize("kind", ["hex", "tet"])
def test_plane_waves_are_exact(tb, device, kind):
    xyz, conn = ref.hex_box(5, 4, 3, perturb=0.2, seed=1) if kind == "hex" else ref.tet_box(3, 3, 2)
    assert kind != "hex" or len(xyz) == 120
    dh = tb.DofHandler(grid_of(tb, kind, xyz, conn))
    src = np.flatnonzero(xyz[:, 0] == 0.0)
    for G in PLANE_TENSORS:
        cache = tb.EikonalActivationCache(device, tb.EikonalModel(tb.ConstantCoefficient(G)), dh)
        T = node_values(tb, dh, tb.solve_activation(cache, src, rtol=RTOL).to_host())
        exact = xyz[:, 0] / np.sqrt(G[0, 0])
        err = np.abs(T - exact).max() / exact.max()
        print("plane wave %s G_xx = %g: %d sweeps, error %.3g" % (kind, G[0, 0], cache.sweeps, err))
        assert cache.converged and err <= 1e-12


# ------------------------------------------------------------------------------------------------ 2, 3. against the reference fixed point; the residual
CASES = ["hex_5x4x3", "tet_3x3x2", "hex_11x10x9_fibres", "hex_1"]


@pytest.mark.parametrize("name", CASES)
def test_matches_the_reference_fixed_point(tb, device, name):
    c, dh, cache, T = solved(tb, device, name)
    want = ref.solution(name)
    dev_ = np.abs(T - want).max()
    print("%s: %d sweeps, max |T - reference| = %.3g (%.3g of max T)" % (name, cache.sweeps, dev_, dev_ / want.max()))
    assert cache.converged and np.isfinite(T).all()
    assert dev_ <= tolerance(want.max())


@pytest.mark.parametrize("name", CASES)
def test_residual_meets_the_stopping_criterion(tb, device, name):
    c, dh, cache, T = solved(tb, device, name)
    res = node_values(tb, dh, cache.residual().to_host())
    free = np.ones(len(T), bool)
    free[c["sources"]] = False
    worst = (np.abs(res[free]) / T[free]).max()
    print("%s: max |res| / T = %.3g (rtol %.1g)" % (name, worst, RTOL))
    assert (np.abs(res[free]) <= RTOL * T[free]).all() and (res[~free] == 0.0).all()
    # the kernel's residual is the reference's, evaluated on the device's own T
    assert np.abs(res - ref.node_residual(c["xyz"], c["conn"], c["M6"], c["sources"], T)).max() <= tolerance(T.max())


# ------------------------------------------------------------------------------------------------ 4. identical bits
def test_two_solves_and_two_objects_give_identical_bits(tb, device):
    c, dh, cache, _ = solved(tb, device, "hex_11x10x9_fibres")
    a = tb.solve_activation(cache, c["sources"], times=c["times"], rtol=RTOL).to_host()
    b = tb.solve_activation(cache, c["sources"], times=c["times"], rtol=RTOL).to_host()
    assert bits(a) == bits(b)
    other = tb.EikonalActivationCache.__new__(tb.EikonalActivationCache)        # a second tb_eikonal over the SAME form
    other.device, other.model, other.dh, other.dmesh, other.form, other._keep = cache.device, cache.model, cache.dh, cache.dmesh, cache.form, cache._keep
    other.h = C.c_void_p()
    tb.check(tb.lib().tb_eikonal_create(cache.form.h, C.byref(other.h)))
    d = tb.solve_activation(other, c["sources"], times=c["times"], rtol=RTOL).to_host()
    assert bits(a) == bits(d) and other.sweeps == cache.sweeps
    assert (other.evaluations, other.updates, other.local_solves) == (cache.evaluations, cache.updates, cache.local_solves)
    assert 0 < cache.updates <= cache.evaluations and cache.evaluations <= cache.local_solves <= 24 * cache.evaluations


# ------------------------------------------------------------------------------------------------ 5. corner point source
def test_corner_source_is_never_early_and_converges(tb, device):
    errs = {}
    for name in ("corner_4", "corner_8"):
        c, dh, cache, T = solved(tb, device, name)
        exact = np.linalg.norm(c["xyz"], axis=1)
        assert (T >= exact - 1e-12).all()
        errs[name] = np.abs(T - exact).max()
        want = ref.solution(name)
        assert np.abs(T - want).max() <= tolerance(want.max())
    print("corner source: max error %.4f at 4^3, %.4f at 8^3" % (errs["corner_4"], errs["corner_8"]))
    assert errs["corner_8"] < errs["corner_4"]


# ------------------------------------------------------------------------------------------------ 6. two disconnected blocks
def test_unreached_block_stays_infinite(tb, device):
    xyz, conn = ref.hex_box(3, 2, 2)
    xyz2, conn2 = np.vstack([xyz, xyz + np.array([5.0, 0.0, 0.0])]), np.vstack([conn, conn + len(xyz)])
    dh = tb.DofHandler(grid_of(tb, "hex", xyz2, conn2))
    cache = tb.EikonalActivationCache(device, tb.EikonalModel(tb.ConstantCoefficient(np.diag([2.0, 1.0, 1.0]))), dh)
    T = tb.solve_activation(cache, [0], rtol=RTOL)
    Tn = node_values(tb, dh, T.to_host())
    assert cache.converged and not np.isnan(Tn).any()
    assert np.isfinite(Tn[:len(xyz)]).all() and np.isposinf(Tn[len(xyz):]).all()
    assert not np.isnan(cache.residual().to_host()).any()
    tpl = tb.ActionPotentialTemplate(0.0, 0.5, [-0.25, 1.0, 0.5, 0.0])
    phi = node_values(tb, dh, tb.activation_potential(cache, 10.0, tpl).to_host())
    assert (phi[len(xyz):] == -0.25).all() and (phi[:len(xyz)] == 0.0).all()          # rest where unreached, the last sample long after activation


# ------------------------------------------------------------------------------------------------ 7. the sweep bound
def test_max_sweeps_bounds_the_call(tb, device):
    c, dh, cache, Tconv = solved(tb, device, "hex_11x10x9_fibres")
    bounded = tb.EikonalActivationCache(device, tb.EikonalModel(coefficient_of(tb, c)), dh)
    T = node_values(tb, dh, tb.solve_activation(bounded, [0], rtol=RTOL, max_sweeps=2, allow_unconverged=True).to_host())
    assert bounded.sweeps == 2 and not bounded.converged
    full = node_values(tb, dh, tb.solve_activation(bounded, [0], rtol=RTOL).to_host())
    assert bounded.converged and bounded.sweeps > 2
    fin = np.isfinite(T)
    assert 1 < fin.sum() < len(T) and (T[fin] >= full[fin]).all()
    with pytest.raises(RuntimeError, match="not converged"):
        tb.solve_activation(bounded, [0], rtol=RTOL, max_sweeps=2)


# ------------------------------------------------------------------------------------------------ 8. potential recovery
@pytest.mark.parametrize("n", [1, 255, 1000])
def test_potential_matches_numpy_interp(tb, device, n):
    rng = np.random.default_rng(n)
    t0, dt, ns = 0.25, 0.125, 41
    U = rng.uniform(-1.0, 1.0, ns)
    tpl = tb.ActionPotentialTemplate(t0, dt, U)
    T = rng.uniform(0.0, 3.0, n)
    T[rng.integers(0, n, max(n // 10, 1))] = np.inf
    xp = t0 + dt * np.arange(ns)
    dT = device.to_device(T)
    for t in (-1.0, 0.2, 1.7, 3.3, 4.9, 9.0, 100.0):          # before every activation, inside the table for some or all nodes, beyond it for all
        got = tb.activation_potential(dT, t, tpl).to_host()
        with np.errstate(invalid="ignore"):
            want = np.where(np.isfinite(T), np.interp(t - np.where(np.isfinite(T), T, 0.0), xp, U), U[0])
        assert np.abs(got - want).max() <= 1e-14


# ------------------------------------------------------------------------------------------------ 9. refusals
def test_refusals(tb, device):
    L = tb._lib
    G = tb.EikonalModel(tb.ConstantCoefficient(1.0))
    quad = tb.DofHandler(tb.generate_mesh(tb.Quadrilateral, (3, 3), (0, 0), (1, 1)))
    with pytest.raises(tb.TBError, match="TB_QUAD4") as e:
        tb.EikonalActivationCache(device, G, quad)
    assert e.value.code == L.TB_ERR_UNSUPPORTED
    g = tb.generate_mesh(tb.Hexahedron, (3, 2, 2), (0, 0, 0), (1, 1, 1))
    with pytest.raises(tb.TBError, match="second-order") as e:
        tb.EikonalActivationCache(device, G, tb.DofHandler(g, tb.LagrangeCollection(2)))
    assert e.value.code == L.TB_ERR_UNSUPPORTED
    dh = tb.DofHandler(g)
    ok = tb.EikonalActivationCache(device, G, dh)
    # a form with a cell set (the forms that take one today are the mechanics forms)
    vmesh = tb.DofHandler(g, tb.LagrangeCollection(1) ** 3).device_mesh(device)
    mat, fh, h = L.tb_material(), C.c_void_p(), C.c_void_p()
    tb.check(tb.lib().tb_hyperelastic_create(vmesh.h, 0, C.byref(mat), C.byref(fh)))
    cells = np.arange(4, dtype=np.int32)
    tb.check(tb.lib().tb_form_set_cellset(fh, cells.ctypes.data_as(L.c_i32p), len(cells), 0))
    assert tb.lib().tb_eikonal_create(fh, C.byref(h)) == L.TB_ERR_UNSUPPORTED and b"cell set" in tb.lib().tb_last_error_string()
    tb.check(tb.lib().tb_form_destroy(fh))
    # a tensor that is not positive definite in ONE cell (nodal scalar field, negative in cell 7): the message names it
    kfield = np.ones((g.n_cells, 8))
    kfield[7] = -1.0
    with pytest.raises(tb.TBError, match=r"cell 7 \(0-based\) is not positive definite") as e:
        tb.EikonalActivationCache(device, tb.EikonalModel(tb.FieldCoefficient(kfield)), dh)
    assert e.value.code == L.TB_ERR_BAD_ARG
    with pytest.raises(tb.TBError, match="not positive definite"):
        tb.EikonalActivationCache(device, tb.EikonalModel(tb.ConstantCoefficient(np.diag([1.0, -1.0, 1.0]))), dh)
    # bad source lists and parameters
    for kwargs, pattern in ((dict(sources=[3, 3]), "twice"), (dict(sources=[0], times=[-1.0]), "source time"), (dict(sources=[0], times=[np.nan]), "source time"),
                            (dict(sources=[0], rtol=0.0), "rtol"), (dict(sources=[0], max_sweeps=0), "max_sweeps")):
        with pytest.raises(tb.TBError, match=pattern) as e:
            tb.solve_activation(ok, **kwargs)
        assert e.value.code == L.TB_ERR_BAD_ARG
    with pytest.raises(ValueError):
        tb.solve_activation(ok, [dh.grid.n_nodes])
    src, tm = np.array([dh.ndofs], dtype=np.int32), np.zeros(1)
    sw, cv = C.c_int(), C.c_int()
    T = device.zeros(dh.ndofs)
    assert tb.lib().tb_eikonal_solve(ok.h, 1, src.ctypes.data_as(L.c_i32p), tm.ctypes.data_as(L.c_dp), 1e-12, 10, T.ptr, C.byref(sw), C.byref(cv)) == L.TB_ERR_BAD_ARG
    # inside an open capture: create and solve are refused, the capture stays valid, the potential is accepted and replays
    tb.solve_activation(ok, [0])
    tpl = tb.ActionPotentialTemplate(0.0, 0.1, np.linspace(0.0, 1.0, 11))
    phi = tb.activation_potential(ok, 0.0, tpl)               # first use uploads the template: before the capture
    seen = {}

    def body():
        seen["create"] = tb.lib().tb_eikonal_create(ok.form.h, C.byref(h))
        try:
            tb.solve_activation(ok, [0], out=ok.T)
        except tb.TBError as err:
            seen["solve"] = err.code
        tb.activation_potential(ok, 0.0, tpl, out=phi)
    graph = device.capture(body)
    assert seen == {"create": L.TB_ERR_BAD_ARG, "solve": L.TB_ERR_BAD_ARG} and graph.nodes >= 1
    Th = ok.T.to_host()
    for t in (0.3, 0.8):
        graph.launch(t)
        device.synchronize()
        assert np.abs(phi.to_host() - tpl(t - Th)).max() <= 1e-14


# ------------------------------------------------------------------------------------------------ 10. the example
def test_example_prints_a_finite_trace():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "eikonal_ecg.py"), "--nc", "8", "--nr", "2", "--nl", "4", "--samples", "6"],
                         capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    d = json.loads(out.stdout.strip().splitlines()[-1])
    assert d["converged"] and d["ecg_finite"] and d["ecg_range"][1] > d["ecg_range"][0] and d["activation_end"] > 0
