"""Device pseudo-ECG (tb_ecg_*, tb_scrub_scale, thunderbolt.jl_amd/ecg.py) against the NumPy restatement of tests/ecg_reference.py and the numbers of
the reference's own test (test/integration/test_ecg.jl).  Tolerances: fluxes 1e-12·max|flux| (the project's parity tolerance); sums 1e-12·Σ|terms|
(the device and NumPy add the same terms in different orders: each term carries a few ulp, the orders differ by ≤ n·ulp·Σ|terms| in the worst case
and ~√n·ulp in practice — 1e-12 leaves two decades at 5·10⁵ points); the reference's own absolute tolerances where its test sets them."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import ecg_reference as R
import transfer_reference as TR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = 16  # the electrode / row tile of the kernels (csrc/tb_ecg.hip: ECG_TILE)


def bits(a):
    return np.ascontiguousarray(a).tobytes()


def diffusion_op(tb, device, dh, coef):
    return tb.setup_operator(tb.PerColorAssemblyStrategy(device), tb.BilinearDiffusionIntegrator(coef), dh, tb.allocate_matrix(dh))


# ------------------------------------------------------------------------------------------------ 1. fluxes
FULL = np.array([[2.0, 0.3, 0.1], [0.3, 1.5, -0.2], [0.1, -0.2, 1.0]])
NONSYM = FULL + np.array([[0, 0.4, 0], [0, 0, 0], [0.25, 0, 0]])          # the non-symmetric tensor of coef_cases (test_gpu_parity.py)
F, S, N_ = np.array([1, 1, 0.0]) / np.sqrt(2), np.array([-1, 1, 0.0]) / np.sqrt(2), np.array([0, 0, 1.0])
LAM = np.array([3.0, 2.0, 0.5])


def tensor_cases(tb, g, with_fibres):
    """(name, coefficient, D at the points: scalar, (3, 3) or (nc, nq, 3, 3))"""
    rng = np.random.default_rng(0)
    nc, nv = g.conn.shape
    _, _, _, N = R.quadrature_geometry(g.xyz, g.conn)
    kfield = rng.uniform(0.2, 3.0, size=(nc, nv))
    cases = [
        ("scalar", tb.ConstantCoefficient(0.7), 0.7),
        ("full", tb.ConstantCoefficient(FULL), FULL),
        ("nonsym", tb.ConstantCoefficient(NONSYM), NONSYM),
        ("spectral", tb.SpectralTensorCoefficient(tb.ConstantCoefficient(tb.OrthotropicMicrostructure(F, S, N_)), tb.ConstantCoefficient(LAM)),
         sum(l * np.outer(v, v) for l, v in zip(LAM, (F, S, N_)))),
        ("iso_field", tb.ConductivityToDiffusivityCoefficient(tb.FieldCoefficient(kfield), tb.ConstantCoefficient(1.1), tb.ConstantCoefficient(0.8)),
         np.einsum("qa,ca->cq", N, kfield)[:, :, None, None] * np.eye(3) / (1.1 * 0.8)),
    ]
    if with_fibres:
        ff = rng.normal(size=(nc, nv, 3)) + np.array([2.0, 0, 0])
        sf = rng.normal(size=(nc, nv, 3)) * 0.3 + np.array([0, 2.0, 0])
        nf = rng.normal(size=(nc, nv, 3)) * 0.3 + np.array([0, 0, 2.0])
        cases.append(("fibre_field", tb.ConductivityToDiffusivityCoefficient(
            tb.SpectralTensorCoefficient(tb.OrthotropicMicrostructureModel(ff, sf, nf), tb.ConstantCoefficient(LAM)), tb.ConstantCoefficient(1.3),
            tb.ConstantCoefficient(0.9)), R.spectral_tensor(np.stack([ff, sf, nf], axis=2), LAM, N, 1.0 / (1.3 * 0.9))))
    return cases


@pytest.mark.parametrize("kind", ["hex", "tet"])
def test_fluxes_entry_by_entry(tb, device, kind):
    g = (tb.generate_mesh(tb.Hexahedron, (3, 4, 2), (0, 0, 0), (1, 1, 1), perturb=0.2) if kind == "hex"
         else tb.generate_mesh(tb.Tetrahedron, (2, 2, 2), (0, 0, 0), (1, 1, 1)))
    dh = tb.DofHandler(g)
    phi = np.random.default_rng(1).uniform(-1.0, 1.0, dh.ndofs)
    dphi = device.to_device(phi)
    for k, (name, coef, D) in enumerate(tensor_cases(tb, g, kind == "hex")):
        op = diffusion_op(tb, device, dh, coef)
        if k % 2:
            tb.update_operator(op, 0.0)           # every other case: the form's table already exists when the cache is made
        cache = tb.Plonsey1964ECGGaussCache(op, dphi)
        got = cache.fluxes()
        ref = R.fluxes(g.xyz, g.conn, dh.cell_dofs, phi, D)
        err = np.abs(got - ref).max() / np.abs(ref).max()
        print("%s %-11s max flux error / max|flux| = %.3e" % (kind, name, err))
        assert got.shape == ref.shape and err <= 1e-12, name
        tb.update_ecg(cache, dphi)
        assert bits(cache.fluxes()) == bits(got), name
    # a non-symmetric D multiplies from the left
    wrong = R.fluxes(g.xyz, g.conn, dh.cell_dofs, phi, NONSYM.T)
    assert np.abs(wrong - R.fluxes(g.xyz, g.conn, dh.cell_dofs, phi, NONSYM)).max() > 1e-2 * np.abs(wrong).max()


# ------------------------------------------------------------------------------------------------ 2. the Plonsey sum
def grid_cap_n(device):
    """the smallest n with 8 n³ points above the grid cap of tb_ecg_evaluate, 256 lanes × 8 · CUs workgroups (41 on the 256 CUs of an MI355X)"""
    cap = 256 * 8 * device.info()["n_cu"]
    n = 1
    while 8 * n ** 3 <= cap:
        n += 1
    return n


def plonsey_case(tb, device, g):
    dh = tb.DofHandler(g)
    phi = np.random.default_rng(2).uniform(-1.0, 1.0, dh.ndofs)
    cache = tb.Plonsey1964ECGGaussCache(diffusion_op(tb, device, dh, tb.ConstantCoefficient(1.0)), device.to_device(phi))
    xq, dO, _, _ = R.quadrature_geometry(g.xyz, g.conn)
    flux = R.fluxes(g.xyz, g.conn, dh.cell_dofs, phi, 1.0)
    lo, hi = g.xyz.min(axis=0), g.xyz.max(axis=0)
    rng = np.random.default_rng(3)
    el = 0.5 * (lo + hi) + (hi - lo) * rng.uniform(0.8, 2.0, (2 * T + 3, 3)) * rng.choice([-1.0, 1.0], (2 * T + 3, 3))   # outside the mesh
    el[0] = g.xyz[g.conn[0]].mean(axis=0)   # INSIDE the mesh: the centroid of cell 0, which is no quadrature point of either rule
    assert np.linalg.norm(xq.reshape(-1, 3) - el[0], axis=1).min() > 1e-3 * np.linalg.norm(hi - lo)
    ref, mag = R.plonsey(flux, xq, dO, el, 0.9)
    for ne in (1, T, T + 1, 2 * T + 3):
        out = tb.evaluate_ecg(cache, el[:ne], 0.9)
        got = out.to_host()
        err = np.abs(got - ref[:ne]) / mag[:ne]
        print("%d cells, %d points, %2d electrodes: max |device − NumPy| / Σ|terms| = %.3e" % (g.n_cells, cache.n_points, ne, err.max()))
        assert got.shape == (ne,) and (err <= 1e-12).all()
        assert bits(tb.evaluate_ecg(cache, el[:ne], 0.9).to_host()) == bits(got)          # two evaluations: identical bits
    one = tb.evaluate_ecg(cache, el[1], 0.9).to_host()                                    # a single point
    assert one.shape == (1,) and abs(one[0] - ref[1]) <= 1e-12 * mag[1]
    tb.update_ecg(cache, device.zeros(dh.ndofs))
    assert (tb.evaluate_ecg(cache, el, 0.9).to_host() == 0.0).all()                       # φ = 0: exactly 0
    return cache.n_points


def test_plonsey_one_cell(tb, device):
    assert plonsey_case(tb, device, tb.generate_mesh(tb.Hexahedron, (1, 1, 1), (0, 0, 0), (1, 2, 3))) == 8          # fewer points than a wave


def test_plonsey_partial_workgroup(tb, device):
    assert plonsey_case(tb, device, tb.generate_mesh(tb.Hexahedron, (3, 4, 2), (0, 0, 0), (1, 1, 1), perturb=0.2)) == 192


def test_plonsey_tetrahedra(tb, device):
    assert plonsey_case(tb, device, tb.generate_mesh(tb.Tetrahedron, (2, 2, 2), (0, 0, 0), (1, 1, 1))) == 192


def test_plonsey_more_than_64_workgroups(tb, device):
    assert plonsey_case(tb, device, tb.generate_mesh(tb.Hexahedron, (13, 13, 13), (0, 0, 0), (1, 1, 1), perturb=0.2)) == 17576  # 69 workgroups


def test_plonsey_grid_stride_loop(tb, device):
    n = grid_cap_n(device)                  # n = 41 with 256 CUs: 8 · 41³ = 551 368 points > 256 · 2 048
    npts = plonsey_case(tb, device, tb.generate_mesh(tb.Hexahedron, (n, n, n), (0, 0, 0), (1, 1, 1), perturb=0.2))
    assert npts > 256 * 8 * device.info()["n_cu"] >= 8 * (n - 1) ** 3


# ------------------------------------------------------------------------------------------------ 3. tb_ecg_leads, tb_scrub_scale
def test_scrub_scale(tb, device):
    x = np.array([np.nan, 0.0, -0.0, 1.5, -2.0, np.nan, 3e300] + [np.nan if k % 7 == 0 else k - 300.0 for k in range(600)])
    d = device.to_device(x)
    tb.scrub_scale(d, -1.0)
    want = -1.0 * np.where(np.isnan(x), 0.0, x)
    assert bits(d.to_host()) == bits(want)                         # −0.0 for the scrubbed NaNs and +0, +0.0 for −0: bit for bit
    assert np.signbit(d.to_host()[:3]).tolist() == [True, True, False]


def test_leads_grid_stride_loop(tb, device):
    """n above the grid cap of tb_ecg_leads (256 lanes × 8 · CUs workgroups; 524 293 columns with 256 CUs): every lane takes a second column"""
    check_leads(tb, device, 256 * 8 * device.info()["n_cu"] + 5)


@pytest.mark.parametrize("n", [1, 63, 64 * 1024 + 5])
def test_leads(tb, device, n):
    check_leads(tb, device, n)


def check_leads(tb, device, n):
    rng = np.random.default_rng(n)
    ldz = n + 3
    Z = rng.uniform(-1.0, 1.0, (T + 1, ldz))
    v = rng.uniform(-1.0, 1.0, n)
    v[::5] = np.nan
    dv = device.to_device(v)
    tb.scrub_scale(dv, 1.0)
    v = np.where(np.isnan(v), 0.0, v)
    assert bits(dv.to_host()) == bits(v)
    dZ = device.to_device(Z.ravel())
    for nl in (1, T, T + 1):
        out = device.to_device(np.full(nl + 1, 777.0))
        call = lambda: tb.check(tb.lib().tb_ecg_leads(device.h, nl, n, dZ.ptr, ldz, dv.ptr, -1.0, out.ptr))   # noqa: E731
        call()
        got = out.to_host()
        terms = Z[:nl, :n] * v
        err = np.abs(got[:nl] + terms.sum(axis=1)) / np.maximum(np.abs(terms).sum(axis=1), 1e-300)
        print("n = %d, %d leads: max |device − NumPy| / Σ|terms| = %.3e" % (n, nl, err.max()))
        assert (err <= 1e-12).all() and got[nl] == 777.0          # nothing behind the last lead is touched
        call()
        assert bits(out.to_host()) == bits(got)


# ------------------------------------------------------------------------------------------------ 4. the reference's test_ecg.jl
SIZE = 2.0
ELECTRODES = np.array([[0.0, 0, 0], [-SIZE, 0, 0], [SIZE, 0, 0], [0, -SIZE, 0], [0, SIZE, 0], [0, 0, -SIZE], [0, 0, SIZE]])


class Blocks:
    """test_ecg.jl:5-88: heart 6³ on [−1,1]³ mapped x → sign(x)·x², torso 16³ on [−2,2]³, κ = 1, κᵢ = 1 in the torso cells with ‖x‖∞ ≤ 1 and 0 outside,
    ground at the vertex nearest the origin, electrodes at the origin and at ±2 on the axes; the leads pair the origin with each of the six"""

    def __init__(self, tb, device, kind):
        self.tb, self.device = tb, device
        heart = tb.generate_mesh(kind, (6, 6, 6))
        heart.xyz[:] = np.sign(heart.xyz) * heart.xyz ** 2
        torso = tb.generate_mesh(kind, (16, 16, 16), (-SIZE,) * 3, (SIZE,) * 3)
        torso.addcellset("heart", lambda x: np.abs(x).max() <= 1.0)
        self.heart, self.torso = heart, torso
        self.hdh, self.tdh = tb.DofHandler(heart), tb.DofHandler(torso)
        self.X = tb.dof_coordinates(self.hdh)
        kappa, kappa_i = tb.ConstantCoefficient(1.0), tb.cellset_coefficient(torso, "heart")
        ground = [tb.get_closest_vertex(ELECTRODES[0], torso)]
        self.phi = device.zeros(self.hdh.ndofs)
        self.plonsey = tb.Plonsey1964ECGGaussCache(diffusion_op(tb, device, self.hdh, kappa), self.phi)
        self.poisson = tb.PoissonECGReconstructionCache(device, self.hdh, self.tdh, kappa_i, kappa, ELECTRODES, ground, torso_heart_domain="heart")
        self.leads = tb.Geselowitz1989ECGLeadCache(device, self.hdh, self.tdh, kappa_i, kappa, [[ELECTRODES[0], e] for e in ELECTRODES[1:]], ground,
                                                   torso_heart_domain="heart")
        self._ref = None

    def set(self, f):
        u = f(self.X)
        self.phi.copy_from_host(u)
        return u

    def all_three(self):
        tb = self.tb
        for c in (self.plonsey, self.poisson, self.leads):
            tb.update_ecg(c, self.phi)
        return tb.evaluate_ecg(self.plonsey, ELECTRODES, 1.0).to_host(), tb.evaluate_ecg(self.poisson).to_host(), tb.evaluate_ecg(self.leads).to_host()

    def dense_reference(self, u):
        """(φₑ at the electrodes, leads) by sparse direct solves in NumPy / SciPy; the operators are built once"""
        tb, torso, tdh = self.tb, self.torso, self.tdh
        if self._ref is None:
            _, _, _, N = R.quadrature_geometry(torso.xyz, torso.conn)
            ki = np.einsum("qa,ca->cq", N, tb.cellset_coefficient(torso, "heart").data)[:, :, None, None] * np.eye(3)
            K = R.diffusion_matrix(torso.xyz, torso.conn, tdh.cell_dofs, tdh.ndofs, 1.0)
            Ki = R.diffusion_matrix(torso.xyz, torso.conn, tdh.cell_dofs, tdh.ndofs, ki)
            n2d = tb.vertex_dofs(tdh)
            ev = n2d[[tb.get_closest_vertex(e, torso) for e in ELECTRODES]]
            dofs, nodes = tb.intergrid_dofs(tdh, "heart")
            cells, xi = TR.locate(self.heart, nodes, 1e-10)
            Z = R.lead_fields(K, [[ev[0], e] for e in ev[1:]], ev[0])
            self._ref = (K, Ki, ev, dofs, cells, xi, Z)
        K, Ki, ev, dofs, cells, xi, Z = self._ref
        phi_t = np.zeros(tdh.ndofs)
        phi_t[dofs] = TR.evaluate(self.hdh, u, cells, xi)[:, 0]
        return R.poisson(K, Ki, phi_t, ev[0])[ev], -Z @ (Ki @ phi_t)


@pytest.fixture(scope="module", params=["hex", "tet"])
def blocks(request, tb, device):
    return Blocks(tb, device, tb.Hexahedron if request.param == "hex" else tb.Tetrahedron)


def test_blocks_equilibrium(blocks):
    blocks.set(lambda X: np.zeros(len(X)))
    pl, po, le = blocks.all_three()
    assert len(pl) == 7 and len(po) == 7 and len(le) == 6
    assert np.abs(pl).max() <= 1e-14 and np.abs(po).max() <= 1e-14 and np.abs(le).max() <= 1e-14


def test_blocks_idempotence(blocks):
    blocks.set(lambda X: np.random.default_rng(5).normal(size=len(X)))
    pl, po, le = blocks.all_three()
    pl2, po2, le2 = blocks.all_three()
    assert bits(pl) == bits(pl2) and bits(le) == bits(le2)        # == as in the reference: ordered reductions
    # the reference asserts == for its direct solver; here the solve is a CG whose inner products are NOT ordered (reduction slots, arrival order
    # free), so two solves agree to the solver tolerance, not bit for bit
    print("Poisson, two updates: max difference / max|φₑ| = %.3e" % (np.abs(po - po2).max() / np.abs(po).max()))
    assert np.abs(po - po2).max() <= 1e-12 * np.abs(po).max()


@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_blocks_planar_wave(blocks, sign):
    u = blocks.set(lambda X: sign * X[:, 0] ** 3)
    pl, po, le = blocks.all_three()
    print("sign %+d: Plonsey %s\n  Poisson %s\n  leads %s" % (sign, pl, po, le))
    if sign > 0:
        assert pl[2] > 0.04 and pl[1] < 0.04                       # test_ecg.jl:143-152
    else:
        assert pl[2] < 0.04 and pl[1] > 0.04                       # :197-206
    assert np.abs(pl[3:]).max() <= 1e-4                            # transverse electrodes
    assert abs(po[0]) <= 1e-12                                     # ground
    assert abs((po[2] - po[1]) - (-sign * 2 * 0.37)) <= 1e-2 and abs(po[4] - po[3]) <= 1e-4 and abs(po[6] - po[5]) <= 1e-4
    assert abs((le[1] - le[0]) - (-sign * 2 * 0.37)) <= 1e-2 and abs(le[3] - le[2]) <= 1e-4 and abs(le[5] - le[4]) <= 1e-4
    # beyond the reference: the two torso methods agree (lead i = φₑ(eᵢ) − φₑ(origin)) to 1e-8·max|φₑ| — solver rtol 1e-12 times the O(10³) condition
    # number of the 16³ Laplacian, with a decade to spare — and both match the direct solve
    scale = np.abs(po).max()
    ref_po, ref_le = blocks.dense_reference(u)
    print("  Poisson vs leads %.3e, Poisson vs direct %.3e, leads vs direct %.3e (all / max|φₑ|)" % (
        np.abs(le - (po[1:] - po[0])).max() / scale, np.abs(po - ref_po).max() / scale, np.abs(le - ref_le).max() / scale))
    assert np.abs(le - (po[1:] - po[0])).max() <= 1e-8 * scale
    assert np.abs(po - ref_po).max() <= 1e-8 * scale and np.abs(le - ref_le).max() <= 1e-8 * scale


def test_blocks_symmetric_stimuli(blocks):
    blocks.set(lambda X: np.sqrt(3.0) - np.linalg.norm(X, axis=1))
    pl, po, le = blocks.all_three()
    for a, b in ((2, 1), (1, 4), (4, 3), (3, 6), (6, 5)):          # test_ecg.jl:255-267: (+x, −x), (−x, +y), (+y, −y), (−y, +z), (+z, −z)
        assert abs(pl[a] - pl[b]) <= 1e-2
    assert abs(po[0]) <= 1e-12 and np.abs(po[2:] - po[1]).max() <= 1e-1
    assert np.abs(le[2:] - le[1]).max() <= 1e-1
    blocks.set(lambda X: X[:, 0] ** 2)
    pl, po, le = blocks.all_three()
    for a, b in ((2, 1), (4, 3), (3, 6), (6, 5)):                  # :288-298
        assert abs(pl[a] - pl[b]) <= 1e-2
    assert abs(po[0]) <= 1e-12
    for d in range(3):
        assert abs(po[2 * d + 2] - po[2 * d + 1]) <= 1e-1 and abs(le[2 * d + 1] - le[2 * d]) <= 1e-1


# ------------------------------------------------------------------------------------------------ 5. captured step
def test_captured_step_equals_the_calls(tb, device, blocks):
    """ONE DeviceGraph holds three time steps' worth of update + evaluate + leads, sample k written at d_out + k·n; it is replayed three times, each
    time with three other φₘ in the buffers it reads, and every replay equals the uncaptured calls bit for bit"""
    pl, le, n = blocks.plonsey, blocks.leads, blocks.hdh.ndofs
    x = device.to_device(ELECTRODES.ravel())
    phis = [device.zeros(n) for _ in range(3)]
    tr_pl, tr_le = device.zeros(3 * 7), device.zeros(3 * 6)

    def steps():
        for k in range(3):
            tb.update_ecg(pl, phis[k])
            tb.evaluate_ecg(pl, x, 1.0, out=tr_pl.view(7 * k, 7))
            tb.update_ecg(le, phis[k])
            tb.evaluate_ecg(le, out=tr_le.view(6 * k, 6))

    steps()                                                        # workspaces reach their size outside the capture
    graph = device.capture(steps)
    assert graph.nodes >= 3 * 7
    rng = np.random.default_rng(11)
    for replay in range(3):
        for p in phis:
            p.copy_from_host(rng.normal(size=n))
        steps()
        want = tr_pl.to_host(), tr_le.to_host()
        tr_pl.fill_zero(); tr_le.fill_zero()
        graph.launch()
        device.synchronize()
        assert bits(tr_pl.to_host()) == bits(want[0]) and bits(tr_le.to_host()) == bits(want[1]), replay
        assert np.abs(want[0]).min() > 0.0 and len(set(want[0][::7])) == 3
    graph.close()


def test_workspace_growth_inside_a_capture_is_refused(tb, blocks):
    dev2 = tb.MI355XDevice(0)                                      # a device object of its own: its reduction workspace is still empty
    try:
        cache = tb.Plonsey1964ECGGaussCache(diffusion_op(tb, dev2, blocks.hdh, tb.ConstantCoefficient(1.0)), dev2.zeros(blocks.hdh.ndofs))
        x, out = dev2.to_device(ELECTRODES.ravel()), dev2.zeros(7)
        with pytest.raises(tb.TBError) as e:
            dev2.capture(lambda: tb.evaluate_ecg(cache, x, 1.0, out=out))
        assert e.value.code == tb._lib.TB_ERR_BAD_ARG and "workspace" in str(e.value)
        tb.evaluate_ecg(cache, x, 1.0, out=out)                    # grows it; the same call is then capturable, and so is a smaller one
        g = dev2.capture(lambda: (tb.evaluate_ecg(cache, x, 1.0, out=out), tb.check(tb.lib().tb_ecg_leads(dev2.h, 1, 7, x.ptr, 7, x.ptr, -1.0, out.ptr))))
        g.launch()
        dev2.synchronize()
        g.close()
    finally:
        dev2.synchronize()                                         # (the device object stays: meshes cached on the handlers still point at it)


# ------------------------------------------------------------------------------------------------ 6. error paths
def test_create_error_paths(tb, device):
    g = tb.generate_mesh(tb.Hexahedron, (2, 2, 2))
    dh = tb.DofHandler(g)
    h = C.c_void_p()
    mass = tb.setup_operator(tb.PerColorAssemblyStrategy(device), tb.BilinearMassIntegrator(tb.ConstantCoefficient(1.0)), dh, tb.allocate_matrix(dh))
    assert tb.lib().tb_ecg_create(mass.form.h, C.byref(h)) == tb._lib.TB_ERR_BAD_ARG and not h
    with pytest.raises(TypeError):
        tb.Plonsey1964ECGGaussCache(mass, device.zeros(dh.ndofs))
    q2 = tb.DofHandler(g, tb.LagrangeCollection(2))
    with pytest.raises(tb.TBError) as e:
        tb.Plonsey1964ECGGaussCache(diffusion_op(tb, device, q2, tb.ConstantCoefficient(1.0)), device.zeros(q2.ndofs))
    assert e.value.code == tb._lib.TB_ERR_UNSUPPORTED
    conn = g.conn.copy()
    conn[5, [0, 1]] = conn[5, [1, 0]]                              # cell 5 inverted
    bad = tb.DofHandler(tb.Grid(tb.Hexahedron, g.xyz, conn))
    with pytest.raises(tb.TBError) as e:
        tb.Plonsey1964ECGGaussCache(diffusion_op(tb, device, bad, tb.ConstantCoefficient(1.0)), device.zeros(bad.ndofs))
    assert e.value.code == tb._lib.TB_ERR_NEG_DETJ and "cell 5" in str(e.value)


def test_poisson_electrode_outside_the_torso_raises(tb, device):
    heart = tb.generate_mesh(tb.Hexahedron, (2, 2, 2), (-0.5,) * 3, (0.5,) * 3)
    torso = tb.generate_mesh(tb.Hexahedron, (4, 4, 4))
    torso.addcellset("heart", lambda x: np.abs(x).max() <= 0.5)
    with pytest.raises(RuntimeError, match="not found in the torso mesh"):
        tb.PoissonECGReconstructionCache(device, tb.DofHandler(heart), tb.DofHandler(torso), tb.cellset_coefficient(torso, "heart"),
                                         tb.ConstantCoefficient(1.0), [[0.9, 0.0, 0.0], [1.5, 0.0, 0.0]], [0], torso_heart_domain="heart")


# ------------------------------------------------------------------------------------------------ 7. example
def test_example_ecg_block():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "ecg_block.py"), "--steps", "20"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    print(res)
    assert res["poisson_leadfield_agreement"] < 1e-6 and res["steps"] == 20
    assert res["plonsey_range"][1] > res["plonsey_range"][0]
