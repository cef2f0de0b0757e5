"""The multigrid family (tb_multigrid.hip, tb_amg.hip, tb_bidomain_mg.hip and the Chebyshev-preconditioned solve of tb_krylov.hip) against the bits of the
commit before its smoother, coarsest inverse, diagonal fill and partial fold were made to exist once (tests/golden/mg_family_parent_bits.npz, written by
record() below with TB_LIBTBHIP naming a library of that commit).  Every input is exact — the matrix values stored with
tests/golden/amg_parent_gmg_solution.npz, dyadic rationals, seeded host vectors — and every sum of these runs has one order (729 dofs: one workgroup per
atomic-ended sum; 1 989 nodes: below the 64 workgroups up to which the block solve's slot sums are ordered), so every comparison is `==`.
Arrays of up to 1 024 values are stored whole, larger ones as the SHA-256 of their bytes and their first and last eight values."""
import hashlib
import os

import numpy as np
import pytest

import bidomain_mg_reference as bmref
import bidomain_reference as bref
from gmg_case import gmg_problem

pytestmark = pytest.mark.gpu

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GOLDEN = os.path.join(GOLDEN_DIR, "mg_family_parent_bits.npz")
VALUES = os.path.join(GOLDEN_DIR, "amg_parent_gmg_solution.npz")
BD_GROUNDS = ("off_coarse", "face")
BD_DEGREE, BD_RATIO = 2, 4.0


def put(out, key, a):
    a = np.ascontiguousarray(a)
    if a.size <= 1024:
        out[key] = a
    else:
        out[key + ".sha256"] = np.frombuffer(hashlib.sha256(a.tobytes()).digest(), dtype=np.uint8)
        out[key + ".ends"] = np.concatenate([a.ravel()[:8], a.ravel()[-8:]])


# ------------------------------------------------------------------------------------------------ (a) – (c): the 729-dof heat matrix
def scalar_problem(tb, device):
    gh, dh, sp, pattern, _, ch, b = gmg_problem(tb, device)
    return gh, dh, pattern, device.to_device(np.load(VALUES)["vals"]), ch, b          # the stored values, not the assembly of this run


def amg_alone(tb, device):
    """(a) AMGPrecon(max_coarse=32, degree=3, interval_ratio=4.0): λmax, level matrices and prolongators, one cycle, the preconditioned solve"""
    gh, dh, pattern, dA, ch, b = scalar_problem(tb, device)
    amg = tb.AMGPrecon(max_coarse=32, degree=3, interval_ratio=4.0).materialize(pattern, ch)
    amg.setup(dA)
    nl = amg.n_levels
    assert nl >= 2
    out = {}
    put(out, "a.n_levels", np.int64(nl))
    for l in range(nl):
        put(out, "a.A%d" % l, amg.level_matrix(l).data)
        if l < nl - 1:
            put(out, "a.lmax%d" % l, np.float64(amg.lambda_max(l)))
            put(out, "a.P%d" % l, amg.prolongator(l).data)
    put(out, "a.z", amg.apply(device.to_device(b), device.zeros(dh.ndofs)).to_host())
    x = device.zeros(dh.ndofs)
    it, res = tb.pcg_solve(pattern, dA, device.to_device(b), x, rtol=1e-10, atol=0.0, maxiter=200, precond=amg)
    put(out, "a.iterations", np.int64(it))
    put(out, "a.resnorm", np.float64(res))
    put(out, "a.x", x.to_host())
    amg.close()
    return out


def chebyshev_solve(tb, device):
    """(b) pcg_solve with ChebyshevPrecBuilder(3)"""
    gh, dh, pattern, dA, ch, b = scalar_problem(tb, device)
    x = device.zeros(dh.ndofs)
    it, res = tb.pcg_solve(pattern, dA, device.to_device(b), x, rtol=1e-10, atol=0.0, maxiter=500, precond=tb.ChebyshevPrecBuilder(3))
    out = {}
    put(out, "b.iterations", np.int64(it))
    put(out, "b.resnorm", np.float64(res))
    put(out, "b.x", x.to_host())
    return out


def geometric_over_amg(tb, device):
    """(c) GMGPrecon(gh, coarse=AMGPrecon(max_coarse=32)): one cycle"""
    gh, dh, pattern, dA, ch, b = scalar_problem(tb, device)
    mg = tb.GMGPrecon(gh, coarse=tb.AMGPrecon(max_coarse=32)).materialize(pattern, ch)
    mg.setup(dA)
    out = {}
    put(out, "c.z", mg.apply(device.to_device(b), device.zeros(dh.ndofs)).to_host())
    return out


# ------------------------------------------------------------------------------------------------ (d): the bidomain block cycle on mesh B
def bidomain_problem(tb):
    """mesh B of bidomain_mg_reference with planes filled from (i, j) by dyadic rationals: M diagonal 1 + (i mod 4)/8, off-diagonal 1/64; the stiffness
    planes as the diffusion form leaves them, negative semidefinite (𝒜 = [[M − ΔtKᵢ, −ΔtKᵢ], [−ΔtKᵢ, −Δt(Kᵢ + Kₑ)]]): −L with L the graph Laplacian of the
    off-diagonal weights (1 + (i + j) mod 5)/64 (Kᵢ) and (2 + (i·j) mod 3)/64 (Kₑ).  With +L no node block of 𝒜 is positive definite: record() checks.
    Every value and every row sum is a small multiple of 1/64: exact."""
    nel, refinements, extent = bmref.MESHES["B"]
    gh = tb.GridHierarchy(tb.generate_mesh(tb.Hexahedron, nel, (0.0, 0.0, 0.0), extent), refinements)
    dhs = [tb.DofHandler(g) for g in gh.grids]
    sps = [tb.allocate_matrix(d) for d in dhs]
    sp, n = sps[-1], dhs[-1].ndofs
    i, j = np.repeat(np.arange(n, dtype=np.int64), np.diff(sp.rowptr)), sp.colidx.astype(np.int64)
    diag = i == j

    def stiffness(weight):
        v = np.where(diag, 0.0, weight)
        rowsum = np.zeros(n)
        np.add.at(rowsum, i, v)
        v[diag] = -rowsum[i[diag]]
        return v

    M = np.where(diag, 1.0 + (i % 4) / 8.0, 1.0 / 64.0)
    Ki, Ke = stiffness((1.0 + (i + j) % 5) / 64.0), stiffness((2.0 + (i * j) % 3) / 64.0)
    return dict(name="B", gh=gh, dhs=dhs, sps=sps, host=(M, Ki, Ke), n=n)


def bidomain_cycle(tb, device, kind, p=None):
    """(d) BidomainMultigrid(degree 2, ratio 4) under ground `kind`: level planes, λmax, one cycle, the solve"""
    p = p or bidomain_problem(tb)
    n, sp, (M, Ki, Ke) = p["n"], p["sps"][-1], p["host"]
    flags = np.zeros(n, dtype=np.uint8)
    flags[bmref.ground_dofs(p, kind)] = 1
    pattern = p["dhs"][-1].device_mesh(device).pattern(sp)
    system = tb.BidomainSystem(pattern)
    system.set_matrices(device.to_device(M), device.to_device(Ki), device.to_device(Ke), bref.DT, device.to_device(flags),
                        bref.ground_diagonal(sp.rowptr, sp.colidx, Ki, Ke, bref.DT))
    mg = tb.BidomainMultigrid(system, p["gh"], BD_DEGREE, BD_RATIO).setup()
    assert mg.n_levels == 3
    out, k = {}, "d.%s." % kind
    for l in range(mg.n_levels):
        for q, plane in enumerate(mg.level_blocks(l)):
            put(out, k + "planes%d.%d" % (l, q), plane)
        if l > 0:
            put(out, k + "lmax%d" % l, np.float64(mg.lambda_max(l)))
    rng = np.random.default_rng(47)
    r = rng.uniform(-1.0, 1.0, 2 * n)
    r[2 * np.flatnonzero(flags) + 1] = 0.0                                            # interleaved: the φₑ of a grounded node
    put(out, k + "z", mg.apply(device.to_device(r), device.zeros(2 * n)).to_host())
    x = device.zeros(2 * n)
    it, res = system.solve(device.to_device(r), x, rtol=1e-10, atol=0.0, maxiter=500, precond=mg)
    put(out, k + "iterations", np.int64(it))
    put(out, k + "resnorm", np.float64(res))
    put(out, k + "x", x.to_host())
    mg.close()
    return out


def record(tb, device, path=GOLDEN):
    """writes the golden file: run once, on the parent commit's library.  Confirms first, on the host, that the block operator of (d) has a positive
    λmax(B⁻¹𝒜) on every level under both grounds (bidomain_mg_reference.lambda_star also asserts that every node block is positive definite)."""
    p = bidomain_problem(tb)
    for kind in BD_GROUNDS:
        lv = bmref.reference_levels(p, kind)
        stars = bmref.lambda_stars(lv["As"], lv["gs"])
        assert all(s > 0.0 for s in stars[1:]), (kind, stars)
    out = {}
    for part in (amg_alone(tb, device), chebyshev_solve(tb, device), geometric_over_amg(tb, device)):
        out.update(part)
    for kind in BD_GROUNDS:
        out.update(bidomain_cycle(tb, device, kind, p))
    np.savez(path, **out)
    return out


# ------------------------------------------------------------------------------------------------ the tests
@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLDEN))


def check(got, gold, prefix):
    want = {k: v for k, v in gold.items() if k.startswith(prefix)}
    differ = [k for k in sorted(set(got) | set(want)) if k not in got or k not in want or got[k].dtype != want[k].dtype or not np.array_equal(got[k], want[k])]
    print("%s %d arrays, differing: %s" % (prefix, len(want), differ or "none"))
    assert len(want) > 0 and not differ


def test_amg_alone_keeps_the_parents_bits(tb, device, gold):
    check(amg_alone(tb, device), gold, "a.")


def test_chebyshev_preconditioned_solve_keeps_the_parents_bits(tb, device, gold):
    check(chebyshev_solve(tb, device), gold, "b.")


def test_geometric_levels_over_amg_keep_the_parents_bits(tb, device, gold):
    check(geometric_over_amg(tb, device), gold, "c.")


@pytest.mark.parametrize("kind", BD_GROUNDS)
def test_bidomain_block_multigrid_keeps_the_parents_bits(tb, device, gold, kind):
    check(bidomain_cycle(tb, device, kind), gold, "d.%s." % kind)
