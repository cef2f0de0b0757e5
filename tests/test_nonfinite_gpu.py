"""Nothing non-finite is lost: NaN and ±∞ are values, and every device entry that hands the host a verdict about them — a scalar reduction, the fused
reaction tangent, the detJ status of an assembly, the convergence report of a Krylov solve — has to carry them there.

The semantics are the reference's, i.e. Julia's `maximum`, `sum` and `dot` (NumPy's np.max, np.sum agree): any NaN among the addressed elements makes the
result NaN, +∞ without a NaN gives +∞, a slice of −∞ gives −∞, |−∞| = +∞, (+∞) + (−∞) = NaN.  Every input here is ordinary data and every index stays in
bounds; nothing tries to make a kernel fault."""
import ctypes as C
import re

import numpy as np
import pytest

from helpers import ADAPTIVE_DT, ADAPTIVE_THRESHOLD, FE_DT, hex_to_tets
from test_gpu_parity import MODELS, initial_points
from test_reduction_edges_gpu import at, length, poke, positions, scalar, strided

pytestmark = pytest.mark.gpu

NAN_BITS = [0x7ff8000000000000, 0xfff8000000000000, 0x7ff0000000000001]      # quiet, quiet with the sign x86 gives 0/0, signalling with a payload
NAN_LENGTHS = [65, 257, 4099, "grid+1"]


def bits_id(b):
    return "%016x" % b


def poke_bits(tb, device, vec, index, bits):
    """one element by its bit pattern (a uint64 copy: nothing canonicalises the NaN on the way)"""
    v = np.array([bits], dtype=np.uint64)
    tb.check(tb.lib().tb_memcpy_h2d(device.h, at(vec, index), v.ctypes.data_as(C.c_void_p), 8))


def same(got, ref):
    """equal as Julia's isequal would have it for these results: both NaN, or the same value"""
    return (np.isnan(got) and np.isnan(ref)) or got == ref


# ------------------------------------------------------------------------------------------- scalar reductions
_TRIDIAGONAL = {}


def tridiagonal(tb, device, n):
    """a device pattern of n rows (tridiagonal) on a mesh without cells: tb_meandiag at any length; (pattern, entries, index of every diagonal entry)"""
    if n not in _TRIDIAGONAL:
        g1 = tb.generate_mesh(tb.Hexahedron, (1, 1, 1))
        dh = tb.DofHandler(tb.Grid(tb.Hexahedron, g1.xyz, g1.conn[:0]), cell_dofs=np.zeros((0, 8), dtype=np.int32), ndofs=n)
        r = np.arange(n, dtype=np.int64)
        cols = np.stack([r - 1, r, r + 1], axis=1)
        ok = (cols >= 0) & (cols < n)
        rowptr = np.concatenate([[0], np.cumsum(ok.sum(axis=1))]).astype(np.int64)
        sp = tb.SparsityPattern(rowptr, cols[ok].astype(np.int32))
        diag = rowptr[:-1] + (r > 0)
        assert np.array_equal(sp.colidx[diag], r)
        _TRIDIAGONAL[n] = (dh, sp, dh.device_mesh(device).pattern(sp), diag)
    _, sp, pat, diag = _TRIDIAGONAL[n]
    return pat, sp.nnz, diag


@pytest.mark.parametrize("bits", NAN_BITS, ids=bits_id)
@pytest.mark.parametrize("n", NAN_LENGTHS, ids=str)
def test_one_nan_makes_max_absmax_dot_and_meandiag_nan(tb, device, n, bits):
    n = length(device, n)
    lib = tb.lib()
    rng = np.random.default_rng(n)
    x, y = rng.uniform(-1.0, 1.0, n), rng.uniform(1.0, 2.0, n)
    dx, dy = device.to_device(x), device.to_device(y)
    pat, nnz, diag = tridiagonal(tb, device, n)
    nz = rng.uniform(-1.0, 1.0, nnz)
    dnz = device.to_device(nz)

    def clean():
        return (scalar(tb, lib.tb_max, device.h, n, dx.ptr, 1), scalar(tb, lib.tb_absmax, device.h, n, dx.ptr, 1),
                scalar(tb, lib.tb_dot, device.h, n, dx.ptr, dy.ptr), scalar(tb, lib.tb_meandiag, pat.h, dnz.ptr))

    before = clean()
    assert before[0] == x.max() and before[1] == np.abs(x).max() and np.isfinite(before).all()
    u = 2.0 ** -53                                                                  # any-order bound of the device's sum plus NumPy's own
    assert abs(before[2] - x @ y) <= 2 * (n - 1) * u * np.abs(x * y).sum() and abs(before[3] - np.abs(nz[diag]).mean()) <= 2 * n * u * before[3]
    for p in positions(device, n):
        poke_bits(tb, device, dx, p, bits)
        got = dx.to_host()[p:p + 1].view(np.uint64)[0]
        assert got == bits, (hex(got), hex(bits))                                  # the pattern arrived as it was written
        assert np.isnan(scalar(tb, lib.tb_max, device.h, n, dx.ptr, 1)), ("tb_max", n, p)
        assert np.isnan(scalar(tb, lib.tb_absmax, device.h, n, dx.ptr, 1)), ("tb_absmax", n, p)
        assert np.isnan(scalar(tb, lib.tb_dot, device.h, n, dx.ptr, dy.ptr)), ("tb_dot", n, p)
        assert np.isnan(scalar(tb, lib.tb_dot, device.h, n, dy.ptr, dx.ptr)), ("tb_dot, second operand", n, p)
        poke(tb, device, dx, p, x[p])
        poke_bits(tb, device, dnz, diag[p], bits)
        assert np.isnan(scalar(tb, lib.tb_meandiag, pat.h, dnz.ptr)), ("tb_meandiag", n, p)
        poke(tb, device, dnz, diag[p], nz[diag[p]])
        if p + 1 < n:                                                              # an off-diagonal NaN is not the diagonal's business
            poke_bits(tb, device, dnz, diag[p] + 1, bits)
            assert abs(scalar(tb, lib.tb_meandiag, pat.h, dnz.ptr) - before[3]) <= 2 * n * u * before[3]
            poke(tb, device, dnz, diag[p] + 1, nz[diag[p] + 1])
    after = clean()
    assert after[:2] == before[:2] and np.isfinite(after).all()                    # nothing sticks to the read-back line or the slots


@pytest.mark.parametrize("stride,phi", [(2, 1), (19, 0)], ids=["stride2", "stride19"])
@pytest.mark.parametrize("n", NAN_LENGTHS, ids=str)
def test_nan_between_the_strides_is_not_read(tb, device, n, stride, phi):
    n = length(device, n)
    lib = tb.lib()
    v = np.random.default_rng(n + stride).uniform(-2.0, -1.0, n)                    # all negative: a skipped NaN, 0 or +x would each show
    buf, off = strided(n, stride, phi, v)
    raw = buf.view(np.uint64)
    skipped = np.ones(buf.size, dtype=bool)
    skipped[off:off + (n - 1) * stride + 1:stride] = False
    raw[skipped] = np.resize(np.array(NAN_BITS, dtype=np.uint64), int(skipped.sum()))   # every element the slice does not address: a NaN, the three kinds in turn
    assert np.isnan(buf[skipped]).all() and np.isfinite(buf[~skipped]).all() and (~skipped).sum() == n
    d = device.to_device(buf)
    assert scalar(tb, lib.tb_max, device.h, n, at(d, off), stride) == np.max(v)
    assert scalar(tb, lib.tb_absmax, device.h, n, at(d, off), stride) == np.max(np.abs(v))
    poke_bits(tb, device, d, off + (n - 1) * stride, NAN_BITS[1])                   # … and the last addressed one is read
    assert np.isnan(scalar(tb, lib.tb_max, device.h, n, at(d, off), stride))
    assert np.isnan(scalar(tb, lib.tb_absmax, device.h, n, at(d, off), stride))


@pytest.mark.parametrize("n", NAN_LENGTHS, ids=str)
def test_infinities_follow_the_reference_table(tb, device, n):
    n = length(device, n)
    lib = tb.lib()
    rng = np.random.default_rng(2 * n)
    base = rng.uniform(-1.0, 1.0, n)
    ones = np.ones(n)
    d1 = device.to_device(ones)
    pat, nnz, diag = tridiagonal(tb, device, n)
    tail = positions(device, n)[-1]                                                # the grid-stride tail where there is one, else the last element
    inf, nan = np.inf, np.nan
    cases = {"+inf": {tail: inf}, "-inf": {0: -inf}, "+inf and -inf": {63: inf, tail: -inf}, "+inf and nan": {64: inf, tail: nan},
             "-inf, +inf and nan": {0: -inf, 1: nan, tail: inf}, "all -inf": None}
    for name, put in cases.items():
        x = np.full(n, -inf) if put is None else base.copy()
        for p, v in (put or {}).items():
            x[p] = v
        dx = device.to_device(x)
        with np.errstate(invalid="ignore"):
            ref_max, ref_abs, ref_dot = np.max(x), np.max(np.abs(x)), np.sum(x * ones)
        got_max = scalar(tb, lib.tb_max, device.h, n, dx.ptr, 1)
        got_abs = scalar(tb, lib.tb_absmax, device.h, n, dx.ptr, 1)
        got_dot = scalar(tb, lib.tb_dot, device.h, n, dx.ptr, d1.ptr)
        assert same(got_max, ref_max) and same(got_abs, ref_abs), (name, n, got_max, ref_max, got_abs, ref_abs)
        assert same(got_dot, ref_dot) or (np.isfinite(ref_dot) and abs(got_dot - ref_dot) <= 1e-12 * np.abs(x).sum()), (name, n, got_dot, ref_dot)
        nz = rng.uniform(-1.0, 1.0, nnz)
        if put is None:
            nz[diag] = -inf
        for p, v in (put or {}).items():
            nz[diag[p]] = v
        dnz = device.to_device(nz)
        got_md = scalar(tb, lib.tb_meandiag, pat.h, dnz.ptr)
        assert same(got_md, np.nan if np.isnan(nz[diag]).any() else np.inf), (name, n, got_md)
    # the table itself, spelt out once
    x = base.copy(); x[tail] = inf
    dx = device.to_device(x)
    assert scalar(tb, lib.tb_max, device.h, n, dx.ptr, 1) == inf and scalar(tb, lib.tb_absmax, device.h, n, dx.ptr, 1) == inf
    x = np.full(n, -inf)
    dx = device.to_device(x)
    assert scalar(tb, lib.tb_max, device.h, n, dx.ptr, 1) == -inf and scalar(tb, lib.tb_absmax, device.h, n, dx.ptr, 1) == inf
    x = base.copy(); x[0] = -inf
    dx = device.to_device(x)
    assert scalar(tb, lib.tb_absmax, device.h, n, dx.ptr, 1) == inf and scalar(tb, lib.tb_max, device.h, n, dx.ptr, 1) == base[1:].max()
    x = np.zeros(n); x[0], x[tail] = inf, -inf
    dx = device.to_device(x)
    assert np.isnan(scalar(tb, lib.tb_dot, device.h, n, dx.ptr, d1.ptr))            # (+∞)·1 + (−∞)·1


# ------------------------------------------------------------------------------------------- fused reaction tangent
@pytest.mark.parametrize("solver", ["euler", "substepper"])
@pytest.mark.parametrize("layout", ["SOA", "AOS"])
@pytest.mark.parametrize("cls,oid", MODELS)
def test_nan_membrane_potential_reaches_R_and_stays_in_its_point(tb, oracle, device, cls, oid, layout, solver):
    """One point with φₘ = NaN: the reaction tangent is NaN through all three ways the host can ask for it, the point's own φₘ (and φₘ rate) stay NaN,
    and no other point notices.  exp_b clamps its argument, so inside the ionic models the NaN survives through the terms linear in φₘ; |NaN| < threshold
    is false, so under the adaptive sub-stepper the point takes the sub-step branch."""
    model = getattr(tb, cls)()
    ns, phi, n = model.nstates, model.phi_index, 4099
    pts = initial_points(tb, model, n, np.random.default_rng(11))
    where = [0, 64, 256, n - 1]
    pts[where] = model.default_initial_state()
    lay = tb.StateBlockedLayout() if layout == "SOA" else tb.PointBlockedLayout()
    f = tb.PointwiseODEFunction(n, model, layout=lay)
    if solver == "euler":
        sv, dt = tb.ForwardEulerCellSolver(device), FE_DT[ns]
    else:
        sv, dt = tb.AdaptiveForwardEulerSubstepper(device, substeps=5, reaction_threshold=ADAPTIVE_THRESHOLD[ns]), ADAPTIVE_DT[ns]

    def flat(p):
        return (np.ascontiguousarray(p.T) if layout == "SOA" else p).ravel().copy()

    def points(v):
        v = v.to_host()
        return v.reshape(ns, n).T if layout == "SOA" else v.reshape(n, ns)

    def run(p):
        """[(R, states after, rates or None)] of tb_reaction_step_rtc without du, with du, and of tb_reaction_step followed by tb_max"""
        out = []
        for keep_du, fused in ((False, True), (True, True), (True, False)):
            c = tb.setup_solver_cache(f, sv, u=device.to_device(flat(p)), keep_du=keep_du)
            if fused:
                ok, R = tb.perform_step_with_reaction_tangent(f, c, 0.0, dt)
            else:
                ok, R = tb.perform_step(f, c, 0.0, dt), tb.get_reaction_tangent(device, f, c)
            assert ok is True
            out.append((R, points(c.un), points(c.du) if keep_du else None))
        return out

    base = run(pts)
    assert all(np.isfinite(R) and np.isfinite(u).all() for R, u, _ in base)
    assert base[0][0] == base[1][0] == base[2][0]                                  # one maximum, three ways
    others = np.ones(n, dtype=bool)
    for p in where:
        bad = pts.copy()
        bad[p, phi] = np.nan
        others[:] = True
        others[p] = False
        for k, ((R, u, du), (_, u0, du0)) in enumerate(zip(run(bad), base)):
            assert np.isnan(R), (cls, layout, solver, "entry %d" % k, p, R)
            assert np.isnan(u[p, phi]), (cls, p, u[p])
            assert np.array_equal(u[others].view(np.uint64), u0[others].view(np.uint64))
            if du is not None:
                assert np.isnan(du[p, phi]), (cls, p, du[p])
                assert np.array_equal(du[others].view(np.uint64), du0[others].view(np.uint64))
        if cls in ("FHNModel", "TT06"):                                             # the CPU reference produces the NaN itself, and np.max keeps it
            du_ref = oracle.reaction_step(getattr(oracle, oid), model.params, flat(bad), n, getattr(oracle, "LAYOUT_" + layout), t=0.0, dt=dt,
                                          substeps=sv.substeps, threshold=sv.reaction_threshold)
            sl = du_ref.reshape(ns, n)[phi] if layout == "SOA" else du_ref.reshape(n, ns)[:, phi]
            assert np.isnan(sl).sum() == 1 and np.isnan(sl[p])
            assert np.isnan(np.max(sl))


def test_reaction_tangent_controller_stops_on_a_nan(tb, device):
    """the 6×6×6 split monodomain problem of test_reaction_tangent_fused_and_signed with one φₘ = NaN before `solve`: RuntimeError, and R is NaN"""
    model = tb.FHNModel()
    g = tb.generate_mesh(tb.Hexahedron, (6, 6, 6), (0, 0, 0), (1, 1, 1))
    dh = tb.DofHandler(g)
    nd = dh.ndofs
    X = np.empty((nd, 3)); X[tb.distributed.node_to_dof(dh)] = g.xyz
    u0 = np.zeros((2, nd))
    u0[0] = (X[:, 0] < 0.5).astype(float)
    u0[1] = 0.1 * (X[:, 1] > 0.5)
    u0[0, nd // 2] = np.nan
    fm = tb.PointwiseODEFunction(nd, model)
    cell = tb.setup_solver_cache(fm, tb.ForwardEulerCellSolver(device), u=device.to_device(u0.ravel()), keep_du=False)
    heat = tb.BackwardEulerStage(tb.BackwardEulerSolver(), tb.PatchAssemblyStrategy(device), dh, tb.ConstantCoefficient(np.diag([4.5e-3, 2.0e-3, 2.0e-3])))
    rtc = tb.ReactionTangentController(tb.LieTrotterGodunov(heat, fm, cell), 0.5, 1.0, (0.05, 0.4))
    with pytest.raises(RuntimeError) as e:
        rtc.solve(0.0, 2.0, 0.1)
    assert np.isnan(rtc.R)
    assert "t = 0" in str(e.value) and "nan" in str(e.value).lower()
    # a clean state on the same operators afterwards: the controller runs
    cell2 = tb.setup_solver_cache(fm, tb.ForwardEulerCellSolver(device), u=device.to_device(np.nan_to_num(u0).ravel()), keep_du=False)
    rtc2 = tb.ReactionTangentController(tb.LieTrotterGodunov(heat, fm, cell2), 0.5, 1.0, (0.05, 0.4))
    hist = rtc2.solve(0.0, 0.5, 0.1)
    assert len(hist) >= 2 and np.isfinite(rtc2.R) and np.isfinite(cell2.un.to_host()).all()


# ------------------------------------------------------------------------------------------- geometry
def _centre_node(xyz):
    return int(np.argmin(np.linalg.norm(xyz - xyz.mean(axis=0), axis=1)))


def _meshes(tb):
    """(name, cell kind, xyz, conn, orders of the displacement field): 4×3×3 hexahedra, the same cut into tetrahedra, 2×2×2 for the quadratic hexahedron"""
    g = tb.generate_mesh(tb.Hexahedron, (4, 3, 3), (0, 0, 0), (1.0, 0.8, 0.6), perturb=0.15)
    g2 = tb.generate_mesh(tb.Hexahedron, (2, 2, 2), (0, 0, 0), (1.0, 0.8, 0.6), perturb=0.1)
    return [("hex", tb.Hexahedron, g.xyz, g.conn, (1,)), ("tet", tb.Tetrahedron, g.xyz, hex_to_tets(g.xyz, g.conn), (1, 2)), ("hex 2x2x2", tb.Hexahedron, g2.xyz, g2.conn, (2,))]


def _entries(tb, device, grid, name, orders):
    """{label: call} of every assembly entry on this grid; the calls raise TBError"""
    lib, L = tb.lib(), tb._lib
    out = {}
    scalar_dhs = {1: tb.DofHandler(grid)}
    if name == "hex 2x2x2":
        scalar_dhs = {2: tb.DofHandler(grid, tb.LagrangeCollection(2))}
    strategies = [tb.ElementAssemblyStrategy, tb.PerColorAssemblyStrategy, tb.AtomicAssemblyStrategy, tb.PatchAssemblyStrategy]
    D = np.diag([4.5e-3, 2.0e-3, 2.0e-3])
    for order, dh in scalar_dhs.items():
        sp = tb.allocate_matrix(dh)
        # (the patch strategy is refused for the quadratic scalar field — TB_ERR_UNSUPPORTED, pinned by test_q2_scalar_forms_parity — so it is no entry there)
        for S in (strategies[:3] if order == 2 else strategies):
            st = S(device)
            M = tb.setup_operator(st, tb.BilinearMassIntegrator(tb.ConstantCoefficient(1.0)), dh, sp)
            K = tb.setup_operator(st, tb.BilinearDiffusionIntegrator(tb.ConstantCoefficient(D)), dh, sp)
            b = tb.setup_operator(st, tb.LinearIntegrator(tb.AnalyticalCoefficient("norm_plus_t")), dh)
            tag = "%s Q/P%d %s" % (name, order, S.__name__)
            out["tb_assemble_matrix mass " + tag] = lambda M=M: tb.update_operator(M, 0.0)
            out["tb_assemble_matrix diffusion " + tag] = lambda K=K: tb.update_operator(K, 0.0)
            out["tb_assemble_matrix_pair " + tag] = lambda M=M, K=K: L.check(lib.tb_assemble_matrix_pair(M.form.h, K.form.h, M.pattern.h, M.strategy.code, 0.0, M.A.ptr, K.A.ptr))
            out["tb_assemble_vector " + tag] = lambda b=b: tb.update_operator(b, 0.3)
    cm = tb.PK1Model(tb.HolzapfelOgden2009Model(), tb.ConstantCoefficient(tb.OrthotropicMicrostructure([1, 0, 0], [0, 1, 0], [0, 0, 1])))
    for order in orders:
        dh = tb.DofHandler(grid, tb.LagrangeCollection(order) ** 3)
        sp = tb.allocate_matrix(dh)
        for S in (tb.AtomicAssemblyStrategy, tb.PerColorAssemblyStrategy):
            Mv = tb.setup_operator(S(device), tb.BilinearMassIntegrator(tb.ConstantCoefficient(1.7)), dh, sp)
            out["vector mass %s order %d %s" % (name, order, S.__name__)] = lambda Mv=Mv: tb.update_operator(Mv, 0.0)
        for S in strategies:
            op = tb.setup_operator(S(device), tb.QuasiStaticModel("u", cm), dh, sp)
            u, res = device.zeros(dh.ndofs), device.zeros(dh.ndofs)
            tag = "%s order %d %s" % (name, order, S.__name__)
            out["tb_linearize " + tag] = lambda op=op, u=u, res=res: tb.update_linearization(op, u, 0.0, residual=res)
            out["tb_residual " + tag] = lambda op=op, u=u, res=res: tb.residual(op, res, u, 0.0)
    return out


@pytest.mark.parametrize("value", [np.nan, np.inf], ids=["nan", "inf"])
def test_a_non_finite_coordinate_is_reported_as_a_bad_cell(tb, device, value):
    """One node coordinate NaN, or +∞: detJ of the cells around the node is NaN (∞ − ∞), or ±∞.  Every assembly entry reports TB_ERR_NEG_DETJ and names one of
    those cells; the same entry on the clean mesh succeeds before and after.  84 entries: 4 scalar calls × 4 strategies on the hexahedra and on the
    tetrahedra, × 3 on the quadratic hexahedron; the vector mass under 2 strategies and tb_linearize / tb_residual under 4, for Q1, P1, P2 and Q2."""
    L = tb._lib
    checked = 0
    for name, kind, xyz, conn, orders in _meshes(tb):
        node = _centre_node(xyz)
        around = set(np.flatnonzero((conn == node).any(axis=1)).tolist())
        assert len(around) >= 8
        bad_xyz = xyz.copy()
        bad_xyz[node, 0] = value
        good = _entries(tb, device, tb.Grid(kind, xyz, conn), name, orders)
        bad = _entries(tb, device, tb.Grid(kind, bad_xyz, conn), name, orders)
        for label in good:
            good[label]()                                                           # (a refusal on the clean mesh raises here: no entry is dropped)
            with pytest.raises(tb.TBError) as e:
                bad[label]()
            assert e.value.code == L.TB_ERR_NEG_DETJ, (label, str(e.value))
            cell = int(re.search(r"cell (-?\d+)", str(e.value)).group(1))
            assert cell in around, (label, cell, sorted(around))
            good[label]()                                                           # nothing sticks
            checked += 1
    assert checked == 2 * 16 + 12 + 4 * (2 + 8) == 84


@pytest.mark.parametrize("value", [np.nan, np.inf], ids=["nan", "inf"])
def test_a_non_finite_coordinate_surfaces_at_the_poll_when_the_status_is_deferred(tb, device, value):
    name, kind, xyz, conn, _ = _meshes(tb)[0]
    node = _centre_node(xyz)
    around = set(np.flatnonzero((conn == node).any(axis=1)).tolist())
    bad_xyz = xyz.copy()
    bad_xyz[node, 1] = value
    for S in (tb.ElementAssemblyStrategy, tb.PerColorAssemblyStrategy, tb.AtomicAssemblyStrategy, tb.PatchAssemblyStrategy):
        st = S(device)
        ops = []
        for coords in (xyz, bad_xyz):
            dh = tb.DofHandler(tb.Grid(kind, coords, conn))
            ops.append(tb.setup_operator(st, tb.BilinearMassIntegrator(tb.ConstantCoefficient(1.0)), dh, tb.allocate_matrix(dh)))
        good, bad = ops
        device.defer_status(True)
        try:
            tb.update_operator(good, 0.0)
            device.poll_status()
            tb.update_operator(bad, 0.0)                                           # returns: the flag waits on the device
            tb.update_operator(good, 0.0)
            with pytest.raises(tb.TBError) as e:
                device.poll_status()
            assert e.value.code == tb._lib.TB_ERR_NEG_DETJ, S.__name__
            assert int(re.search(r"cell (-?\d+)", str(e.value)).group(1)) in around, S.__name__
            device.poll_status()
        finally:
            device.defer_status(False)
        assert np.isfinite(tb.update_operator(good, 0.0).A.to_host()).all()


# ------------------------------------------------------------------------------------------- Krylov entries
SOLVERS = ["cg", "cg_jacobi", "cg_from_residual", "pcg_l1gs", "pcg_chebyshev", "gmres", "cg_f32"]
MAXITER = 12


@pytest.fixture(scope="module")
def heat_system(tb, device):
    """the n = 120 heat matrix of test_jacobi_reuse_survives_other_solvers_on_the_shared_workspace, with its scipy solution"""
    import scipy.sparse as ssp
    import scipy.sparse.linalg as sla
    g = tb.generate_mesh(tb.Hexahedron, (5, 4, 3), (0, 0, 0), (1, 1, 1), perturb=0.2)
    dh = tb.DofHandler(g)
    sp = tb.allocate_matrix(dh)
    n = dh.ndofs
    assert n == 120
    st = tb.PatchAssemblyStrategy(device)
    kap = np.diag([4.5e-5, 2.0e-5, 2.0e-5])
    D = tb.ConductivityToDiffusivityCoefficient(tb.ConstantCoefficient(kap), tb.ConstantCoefficient(1.0), tb.ConstantCoefficient(1.0))
    M = tb.update_operator(tb.setup_operator(st, tb.BilinearMassIntegrator(tb.ConstantCoefficient(1.0)), dh, sp), 0.0)
    K = tb.update_operator(tb.setup_operator(st, tb.BilinearDiffusionIntegrator(D), dh, sp), 0.0)
    A = tb.heat_system_matrix(device, M, K, 0.01)
    Ah = A.to_host().copy()
    Am = ssp.csr_matrix((Ah, sp.colidx, sp.rowptr), shape=(n, n))
    bh = np.random.default_rng(7).normal(size=n)
    xs = sla.spsolve(Am.tocsc(), bh)
    return dict(n=n, sp=sp, pat=M.pattern, keep=(M, K), A=A, Ah=Ah, Am=Am, bh=bh, xs=xs, cond=float(np.linalg.cond(Am.toarray())))


def _solve(tb, device, name, pat, Ah, bh, x0h, rtol, maxiter, sp, jacobi_reuse_of=None):
    """(rc, iters, resnorm, tolerance, x, the device matrix) of one call; cg_from_residual gets b − A x₀ as the caller forms it"""
    lib, L = tb.lib(), tb._lib
    it, res = C.c_int(-1), C.c_double(-1.0)
    f32 = name == "cg_f32"
    dt = np.float32 if f32 else np.float64
    A = jacobi_reuse_of if jacobi_reuse_of is not None else device.to_device(Ah.astype(dt))
    rhs = bh
    if name == "cg_from_residual" and x0h.any():                                   # (x₀ = 0: the residual is b itself, no product — a non-finite entry of A is then
        import scipy.sparse as ssp                                                 #  first met INSIDE the iteration, by the pᵀAp check of the update kernel)
        with np.errstate(invalid="ignore", over="ignore"):
            rhs = bh - ssp.csr_matrix((Ah, sp.colidx, sp.rowptr), shape=(len(bh), len(bh))) @ x0h
    b, x = device.to_device(rhs.astype(dt)), device.to_device(x0h.astype(dt))
    args = (pat.h, A.ptr, b.ptr, x.ptr, rtol, 0.0, maxiter)
    if name in ("cg", "cg_jacobi"):
        rc = lib.tb_cg_solve(*args, (2 if jacobi_reuse_of is not None else 1) if name == "cg_jacobi" else 0, C.byref(it), C.byref(res))
    elif name == "cg_from_residual":
        rc = lib.tb_cg_solve_from_residual(*args, 1, C.byref(it), C.byref(res))
    elif name == "pcg_l1gs":
        rc = lib.tb_pcg_solve(*args, L.TB_PRECOND_L1GS, 64, C.byref(it), C.byref(res))
    elif name == "pcg_chebyshev":
        rc = lib.tb_pcg_solve(*args, L.TB_PRECOND_CHEBYSHEV, 4, C.byref(it), C.byref(res))
    elif name == "gmres":
        rc = lib.tb_gmres_solve(*args, 10, 1, C.byref(it), C.byref(res))
    else:
        rc = lib.tb_cg_solve_f32(*args, 1, C.byref(it), C.byref(res))
    tol = C.c_double(-1.0)
    tb.check(lib.tb_solver_last_tolerance(pat.h, C.byref(tol)))
    return rc, it.value, res.value, tol.value, x.to_host().astype(np.float64), A


@pytest.mark.parametrize("name", SOLVERS)
def test_krylov_solves_never_report_convergence_on_non_finite_data(tb, device, heat_system, name):
    """A contract, not an iterate check.  One NaN, or one +∞, in b, in x₀, on a diagonal or on an off-diagonal entry of A, maxiter = 12: the call returns — an
    error code, or TB_OK with iters ≤ 12 and a resnorm that does NOT compare ≤ tb_solver_last_tolerance.  The same solver on the clean system straight
    afterwards converges to the scipy solution: ‖x − x*‖ ≤ 2·κ(A)·(rtol + storage rounding)·‖x*‖, the residual bound of the stopping test with a factor 2
    for the drift between the recurred and the true residual (Float32 storage rounds A, b and x once each: 3·2⁻²⁴)."""
    L = tb._lib
    h = heat_system
    n, sp, pat = h["n"], h["sp"], h["pat"]
    rows = np.repeat(np.arange(n), np.diff(sp.rowptr))
    k_diag = int(np.flatnonzero((rows == 57) & (sp.colidx == 57))[0])
    k_off = int(np.flatnonzero((rows == 57) & (sp.colidx != 57))[0])
    f32 = name == "cg_f32"
    rtol = 1e-5 if f32 else 1e-10
    bound = 2.0 * h["cond"] * (rtol + (3 * 2.0 ** -24 if f32 else 0.0)) * np.linalg.norm(h["xs"])
    x0 = np.zeros(n)
    report = []
    for where in ("b", "x0", "A diagonal", "A off-diagonal"):
        for value in (np.nan, np.inf):
            Ah, bh, x0h = h["Ah"].copy(), h["bh"].copy(), x0.copy()
            if where == "b":
                bh[31] = value
            elif where == "x0":
                x0h[31] = value
            else:
                Ah[k_diag if where == "A diagonal" else k_off] = value
            rc, it, res, tol, _, _ = _solve(tb, device, name, pat, Ah, bh, x0h, rtol, MAXITER, sp)
            report.append("%s %s in %s: rc %d iters %d resnorm %g tolerance %g" % (name, value, where, rc, it, res, tol))
            if rc == L.TB_OK:
                assert 0 <= it <= MAXITER, report[-1]
                assert not (res <= tol), report[-1]                                # never "converged"
            else:
                assert rc == L.TB_ERR_BAD_ARG, report[-1]                          # "not positive definite" / "non-finite Arnoldi vector"; never a HIP error
            # the clean system straight afterwards (cg_jacobi: with the D⁻¹ of the clean matrix reused where A itself was clean — TB_JACOBI_REUSE)
            reuse = None
            if name == "cg_jacobi" and where in ("b", "x0"):
                rc0, _, _, _, _, reuse = _solve(tb, device, name, pat, h["Ah"], bh, x0h, rtol, MAXITER, sp)
                assert rc0 == L.TB_OK
            rc, it, res, tol, x, _ = _solve(tb, device, name, pat, h["Ah"], h["bh"], x0, rtol, 300, sp, jacobi_reuse_of=reuse)
            assert rc == L.TB_OK and 0 < it < 300 and np.isfinite(res) and res <= tol, (report[-1], rc, it, res, tol)
            err = np.linalg.norm(x - h["xs"])
            assert err <= bound, (report[-1], err, bound)
    print("\n".join(report))
