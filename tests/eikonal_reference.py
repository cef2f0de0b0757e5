"""NumPy restatement of the eikonal scheme of csrc/tb_eikonal.hip, written independently of csrc/tb_eikonal.hpp: the same local solver (minimum over
the unit simplex of Σ λᵢTᵢ + √(e(λ)ᵀ M e(λ)), candidates from the closed form on the face, its edges and its vertices — here through
numpy.linalg.solve on the sub-blocks of Q, not through adjugates), swept to the fixed point: Gauss–Seidel in forward or reversed node order, or
Jacobi.  An update is accepted iff it is strictly smaller, so the iteration ends at the exact fixed point of the arithmetic.

It is pinned on exact cases by tests/test_eikonal_cpu.py (plane waves; equality of the three sweep orders) before any device result is compared with
it.  Meshes and cases of the device tests are built here too, once per session (functools.lru_cache), and never modified."""
import functools
import itertools

import numpy as np

KUHN = np.array([[0, 1, 2, 6], [0, 5, 1, 6], [0, 2, 3, 6], [0, 3, 7, 6], [0, 4, 5, 6], [0, 7, 4, 6]])     # include/tbhip.h, tb_host_generate_grid_tet
SUBSETS = [(0,), (1,), (2,), (0, 1), (0, 2), (1, 2), (0, 1, 2)]
HEX_SIGNS = np.array([(-1, -1, -1), (1, -1, -1), (1, 1, -1), (-1, 1, -1), (-1, -1, 1), (1, -1, 1), (1, 1, 1), (-1, 1, 1)], dtype=float)


def sym6_to_33(m6):
    m6 = np.asarray(m6, dtype=float)
    out = np.empty(m6.shape[:-1] + (3, 3))
    for k, (i, j) in enumerate([(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]):
        out[..., i, j] = out[..., j, i] = m6[..., k]
    return out


def objective(Y, T, M, lam):
    """F(λ) = Σ λᵢTᵢ + √(eᵀMe), e = Σ λᵢYᵢ; Y (…, 3, 3) rows xᵢ − x₄, T (…, 3) finite, M (…, 3, 3), lam (…, 3)"""
    e = np.einsum("...i,...id->...d", lam, Y)
    return np.einsum("...i,...i->...", lam, T) + np.sqrt(np.maximum(np.einsum("...d,...de,...e->...", e, M, e), 0.0))


def local_solve(Y, T, M):
    """batched local solver: Y (n, 3, 3), T (n, 3) with +inf allowed, M (n, 3, 3) → values (n,), lam (n, 3)"""
    Y, T, M = np.asarray(Y, float), np.asarray(T, float), np.asarray(M, float)
    n = len(T)
    fin = np.isfinite(T)
    T0 = np.where(fin, T, np.inf).min(axis=1)
    t = np.where(fin, T - np.where(np.isfinite(T0), T0, 0.0)[:, None], 0.0)
    Q = np.einsum("nid,nde,nje->nij", Y, M, Y)
    best = np.full(n, np.inf)
    blam = np.zeros((n, 3))
    for S in SUBSETS:
        idx = list(S)
        ok = fin[:, idx].all(axis=1)
        if not ok.any():
            continue
        rows = np.flatnonzero(ok)
        Qs = Q[np.ix_(rows, idx, idx)]
        ts = t[np.ix_(rows, idx)]
        u = np.linalg.solve(Qs, np.ones((len(rows), len(idx), 1)))[..., 0]
        v = np.linalg.solve(Qs, ts[..., None])[..., 0]
        a, b, c = u.sum(axis=1), v.sum(axis=1), (ts * v).sum(axis=1) - 1.0
        disc = b * b - a * c
        good = (disc >= 0.0) & (a > 0.0)
        mu = (b + np.sqrt(np.where(good, disc, 0.0))) / np.where(good, a, 1.0)
        w = mu[:, None] * u - v
        sw = w.sum(axis=1)
        good &= (w >= 0.0).all(axis=1) & (sw > 0.0)
        lam = np.zeros((len(rows), 3))
        lam[:, idx] = w / np.where(good, sw, 1.0)[:, None]
        val = np.where(good, objective(Y[rows], t[rows], M[rows], lam), np.inf)
        better = val < best[rows]
        best[rows[better]] = val[better]
        blam[rows[better]] = lam[better]
    return np.where(np.isfinite(best), T0 + best, np.inf), blam


# ------------------------------------------------------------------------------------------------ meshes
def tetrahedra(conn):
    """(n_tets, 4) node ids and the cell of every tetrahedron: a tetrahedral mesh as it is, hexahedra by the Kuhn split of their local order"""
    conn = np.asarray(conn)
    if conn.shape[1] == 4:
        return conn.copy(), np.arange(len(conn))
    return conn[:, KUHN].reshape(-1, 4), np.repeat(np.arange(len(conn)), 6)


def corner_records(tets, tet_cell, n_nodes):
    """per node, in ascending (cell, tetrahedron) order: (the three other nodes, cell); CSR"""
    node = tets.ravel()
    others = np.stack([np.delete(tets, a, axis=1) for a in range(4)], axis=1).reshape(-1, 3)
    cell = np.repeat(tet_cell, 4)
    order = np.argsort(node, kind="stable")
    ptr = np.concatenate([[0], np.cumsum(np.bincount(node, minlength=n_nodes))])
    return ptr, others[order], cell[order], node[order]


def fixed_point(xyz, conn, M6, sources, times, order="jacobi", max_sweeps=10000):
    """arrival times at the nodes (ids of `conn`); M6 (n_cells, 6) or (6,).  order: "forward" / "reversed" (Gauss–Seidel) or "jacobi"."""
    xyz = np.asarray(xyz, float)
    n = len(xyz)
    tets, tet_cell = tetrahedra(conn)
    M6 = np.broadcast_to(np.asarray(M6, float), (len(conn), 6))
    M = sym6_to_33(M6)
    ptr, others, cell, node = corner_records(tets, tet_cell, n)
    Yall = xyz[others] - xyz[node][:, None, :]
    Mall = M[cell]
    T = np.full(n, np.inf)
    fixed = np.zeros(n, bool)
    T[np.asarray(sources)] = times
    fixed[np.asarray(sources)] = True
    dirty = np.ones(n, bool)
    for _ in range(max_sweeps):
        changed = False
        if order == "jacobi":
            val, _ = local_solve(Yall, T[others], Mall)
            new = np.full(n, np.inf)
            np.minimum.at(new, node, val)
            upd = (new < T) & ~fixed
            changed = bool(upd.any())
            T = np.where(upd, new, T)
        else:
            # a node is solved again only if a neighbour moved since its last solve (its update is a function of the neighbours alone)
            seq = range(n) if order == "forward" else range(n - 1, -1, -1)
            for i in seq:
                if fixed[i] or ptr[i] == ptr[i + 1] or not dirty[i]:
                    continue
                r = slice(ptr[i], ptr[i + 1])
                Tn = T[others[r]]
                if not np.isfinite(Tn).any():
                    continue
                dirty[i] = False
                val, _ = local_solve(Yall[r], Tn, Mall[r])
                v = val.min()
                if v < T[i]:
                    T[i] = v
                    dirty[others[r]] = True
                    changed = True
        if not changed:
            return T
    raise RuntimeError("eikonal reference: no fixed point after %d sweeps" % max_sweeps)


def node_residual(xyz, conn, M6, sources, T):
    """T_i − min(local solves on T) for the nodes that are not sources (0 there and where both are ∞)"""
    xyz = np.asarray(xyz, float)
    n = len(xyz)
    tets, tet_cell = tetrahedra(conn)
    M = sym6_to_33(np.broadcast_to(np.asarray(M6, float), (len(conn), 6)))
    ptr, others, cell, node = corner_records(tets, tet_cell, n)
    val, _ = local_solve(xyz[others] - xyz[node][:, None, :], T[others], M[cell])
    new = np.full(n, np.inf)
    np.minimum.at(new, node, val)
    with np.errstate(invalid="ignore"):
        res = np.where(np.isfinite(T) | np.isfinite(new), T - new, 0.0)
    res[np.asarray(sources)] = 0.0
    return res


def hex_box(nx, ny, nz, left=(0.0, 0.0, 0.0), right=(1.0, 1.0, 1.0), perturb=0.0, seed=0):
    """Ferrite-order hexahedral box (nodes x-fastest); interior nodes moved by `perturb`·h with a fixed seed, boundary nodes left on the faces"""
    xs = [np.linspace(left[d], right[d], m + 1) for d, m in enumerate((nx, ny, nz))]
    Z, Yc, X = np.meshgrid(xs[2], xs[1], xs[0], indexing="ij")
    xyz = np.stack([X.ravel(), Yc.ravel(), Z.ravel()], axis=1)
    px, py = nx + 1, ny + 1
    nid = lambda i, j, k: i + px * (j + py * k)
    conn = np.array([[nid(i, j, k), nid(i + 1, j, k), nid(i + 1, j + 1, k), nid(i, j + 1, k), nid(i, j, k + 1), nid(i + 1, j, k + 1),
                      nid(i + 1, j + 1, k + 1), nid(i, j + 1, k + 1)] for k in range(nz) for j in range(ny) for i in range(nx)], dtype=np.int32)
    if perturb:
        h = np.array([(right[d] - left[d]) / m for d, m in enumerate((nx, ny, nz))])
        I, J, K = np.meshgrid(range(nx + 1), range(ny + 1), range(nz + 1), indexing="ij")
        interior = np.zeros(len(xyz), bool)
        ii, jj, kk = np.arange(1, nx), np.arange(1, ny), np.arange(1, nz)
        for i, j, k in itertools.product(ii, jj, kk):
            interior[nid(i, j, k)] = True
        rng = np.random.default_rng(seed)
        xyz[interior] += perturb * h * rng.uniform(-1.0, 1.0, size=(int(interior.sum()), 3))
    return xyz, conn


def tet_box(nx, ny, nz, left=(0.0, 0.0, 0.0), right=(1.0, 1.0, 1.0)):
    xyz, hexes = hex_box(nx, ny, nz, left, right)
    return xyz, hexes[:, KUHN].reshape(-1, 4).astype(np.int32)


def transverse_tensor(angle, lam_f, lam_t):
    f = np.array([np.cos(angle), np.sin(angle), 0.0])
    return lam_f * np.outer(f, f) + lam_t * (np.eye(3) - np.outer(f, f))


def inverse6(G):
    Mi = np.linalg.inv(np.asarray(G, float))
    return np.stack([Mi[..., 0, 0], Mi[..., 0, 1], Mi[..., 0, 2], Mi[..., 1, 1], Mi[..., 1, 2], Mi[..., 2, 2]], axis=-1)


def rotating_fibres(xyz, conn, zmin, zmax, a0=-1.0, a1=1.0):
    """nodal f, s, n per cell, (n_cells, 8, 3) each: the fibre turns in the xy-plane from angle a0 at zmin to a1 at zmax"""
    z = xyz[conn][:, :, 2]
    ang = a0 + (a1 - a0) * (z - zmin) / (zmax - zmin)
    f = np.stack([np.cos(ang), np.sin(ang), np.zeros_like(ang)], axis=2)
    s = np.stack([-np.sin(ang), np.cos(ang), np.zeros_like(ang)], axis=2)
    nrm = np.broadcast_to(np.array([0.0, 0.0, 1.0]), f.shape).copy()
    return f, s, nrm


def spectral_cell_mean(f, s, nrm, lam):
    """per cell the mean over the 8 Gauss points of λ₁ f⊗f + λ₂ s⊗s + λ₃ n⊗n with f, s, n interpolated, normalised and orthogonalised at the
    point as csrc/tb_assembly.hip does (normalise all three, Gram–Schmidt without renormalising)"""
    g = 0.5773502691896258
    G = np.zeros((len(f), 3, 3))
    for q in range(8):
        xi = np.array([g if q & 1 else -g, g if q & 2 else -g, g if q & 4 else -g])
        N = 0.125 * np.prod(1.0 + HEX_SIGNS * xi, axis=1)
        fq, sq, nq = (np.einsum("a,cad->cd", N, v) for v in (f, s, nrm))
        fq, sq, nq = (v / np.linalg.norm(v, axis=1, keepdims=True) for v in (fq, sq, nq))
        sq = sq - (fq * sq).sum(axis=1, keepdims=True) * fq
        nq = nq - (fq * nq).sum(axis=1, keepdims=True) * fq - (sq * nq).sum(axis=1, keepdims=True) * sq
        for l, v in zip(lam, (fq, sq, nq)):
            G += l * np.einsum("ci,cj->cij", v, v)
    return G / 8.0


# ------------------------------------------------------------------------------------------------ the cases of the device tests
G_TRANSVERSE = transverse_tensor(0.5, 4.0, 1.0)     # 4 : 1, fibre at 0.5 rad in the xy-plane
SPECTRAL_LAMBDA = (4.0, 1.0, 0.5)


def two_interior_sources(xyz):
    """the nodes closest to two interior points, onsets 0 and 0.3"""
    lo, hi = xyz.min(axis=0), xyz.max(axis=0)
    pts = [lo + (hi - lo) * np.array([0.3, 0.35, 0.4]), lo + (hi - lo) * np.array([0.7, 0.6, 0.6])]
    ids = [int(np.argmin(((xyz - p) ** 2).sum(axis=1))) for p in pts]
    assert ids[0] != ids[1]
    return np.array(ids, dtype=np.int32), np.array([0.0, 0.3])


@functools.lru_cache(maxsize=None)
def case(name):
    """name → dict(kind, xyz, conn, G or fibres, M6, sources, times): the problems of test 2 of the device tests"""
    if name == "hex_5x4x3":
        xyz, conn = hex_box(5, 4, 3, perturb=0.2, seed=1)
        src, tm = two_interior_sources(xyz)
        return dict(kind="hex", xyz=xyz, conn=conn, G=G_TRANSVERSE, M6=inverse6(G_TRANSVERSE), sources=src, times=tm)
    if name == "tet_3x3x2":
        xyz, conn = tet_box(3, 3, 2)
        src, tm = two_interior_sources(xyz)
        return dict(kind="tet", xyz=xyz, conn=conn, G=G_TRANSVERSE, M6=inverse6(G_TRANSVERSE), sources=src, times=tm)
    if name == "hex_11x10x9_fibres":
        xyz, conn = hex_box(11, 10, 9)
        f, s, nrm = rotating_fibres(xyz, conn, 0.0, 1.0)
        G = spectral_cell_mean(f, s, nrm, SPECTRAL_LAMBDA)
        src, tm = two_interior_sources(xyz)
        return dict(kind="hex", xyz=xyz, conn=conn, fibres=(f, s, nrm), lam=SPECTRAL_LAMBDA, M6=inverse6(G), sources=src, times=tm)
    if name == "hex_1":
        xyz, conn = hex_box(1, 1, 1)
        return dict(kind="hex", xyz=xyz, conn=conn, G=G_TRANSVERSE, M6=inverse6(G_TRANSVERSE), sources=np.array([0], dtype=np.int32), times=np.array([0.0]))
    if name in ("corner_4", "corner_8"):
        m = int(name.split("_")[1])
        xyz, conn = hex_box(m, m, m)
        return dict(kind="hex", xyz=xyz, conn=conn, G=np.eye(3), M6=inverse6(np.eye(3)), sources=np.array([0], dtype=np.int32), times=np.array([0.0]))
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def solution(name, order="jacobi"):
    c = case(name)
    T = fixed_point(c["xyz"], c["conn"], c["M6"], c["sources"], c["times"], order)
    T.setflags(write=False)
    return T
