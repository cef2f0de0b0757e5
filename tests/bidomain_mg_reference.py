"""NumPy restatement of the multigrid preconditioner of the bidomain block system (csrc/tb_bidomain_mg.hip): ground flags per level, the dense block
transfers 𝒫 = diag(P, G_f P G_c), the Galerkin chain with the diagonal fill, the masked 2 × 2 block inverses, the Chebyshev recurrences, the V-cycle, λmax as
a dense eigenvalue, and the preconditioned conjugate gradients.  Nothing here imports the package.  Unknowns are ordered BLOCKED, (φₘ; φₑ), as in
bidomain_reference; `interleave` / `deinterleave` there go to and from the device's layout.  Levels are listed coarsest first, as MultigridHierarchy does."""
import numpy as np

import bidomain_reference as bref
import multigrid_reference as mref

# the meshes: the smallest at which each mechanism can go wrong — (cells of the coarsest grid, refinements, extents)
MESHES = {
    "A": ((2, 2, 2), 1, (1.0, 1.0, 1.0)),       # 5³ = 125 nodes: two slices of 64 rows, the second with 61; two levels
    "B": ((2, 3, 4), 2, (1.0, 1.3, 0.8)),       # 9 × 13 × 17 = 1 989 nodes, a partial last slice; three levels, so one level runs the four-plane product
}
GROUNDS = ("vertex", "off_coarse", "face")


def ground_nodes(gh, kind):
    """node ids of the three grounds on the finest grid of `gh`: (i) vertex 0; (ii) two fine vertices that are no vertices of the next-coarser grid (coarse
    nodes are a prefix of the fine nodes: an edge centre and the last cell centre); (iii) the whole face x = 0"""
    fine, nc = gh.grids[-1], gh.grids[-2].n_nodes
    if kind == "vertex":
        return np.array([0])
    if kind == "off_coarse":
        return np.array([nc + 3, fine.n_nodes - 2])
    if kind == "face":
        return np.flatnonzero(np.abs(fine.xyz[:, 0]) < 1e-12)
    raise KeyError(kind)


def scalar_dofs(dh):
    return mref.node_dofs(dh)[:, 0]


def level_grounds(gh, dhs, ground_fine):
    """flags by dof per level: a coarse node is grounded iff the fine node it coincides with is"""
    gs = [None] * len(dhs)
    gs[-1] = np.asarray(ground_fine, dtype=bool)
    for l in range(len(dhs) - 1, 0, -1):
        nf, ncs = scalar_dofs(dhs[l]), scalar_dofs(dhs[l - 1])
        g = np.zeros(dhs[l - 1].ndofs, dtype=bool)
        g[ncs] = gs[l][nf[:len(ncs)]]
        gs[l - 1] = g
    return gs


def block_P(parents, dh_fine, dh_coarse, g_fine, g_coarse):
    """𝒫 = diag(P, G_f P G_c), dense, (2 n_f) × (2 n_c)"""
    nf, ncs = scalar_dofs(dh_fine), scalar_dofs(dh_coarse)
    P = np.zeros((dh_fine.ndofs, dh_coarse.ndofs))
    P[np.ix_(nf, ncs)] = mref.nodal_P(parents, dh_coarse.grid.n_nodes)
    Pe = P.copy()
    Pe[g_fine, :] = 0.0
    Pe[:, g_coarse] = 0.0
    Z = np.zeros_like(P)
    return np.block([[P, Z], [Z, Pe]])


def galerkin(P, A, g_coarse):
    """𝒫ᵀ𝒜𝒫; the φₑφₑ diagonal of a grounded coarse node (row and column are empty) is the mean |diagonal| of the free φₑφₑ entries"""
    Ac = P.T @ A @ P
    n = len(g_coarse)
    if g_coarse.any():
        d = np.abs(np.diag(Ac)[n:])[~g_coarse]
        idx = n + np.flatnonzero(g_coarse)
        Ac[idx, idx] = d.mean() if len(d) else 1.0
    return Ac


def hierarchy(gh, dhs, A_fine, ground_fine, dtype=np.float64):
    """dense level operators, block transfers and ground flags (coarsest first) → (As, Ps, gs); A_fine: the eliminated block matrix.  dtype
    np.longdouble: the Galerkin products and the fill accumulate in extended precision and the coarse operators stay in it"""
    nl = len(dhs)
    gs = level_grounds(gh, dhs, ground_fine)
    As, Ps = [None] * nl, [None] * nl
    As[-1] = A_fine
    for l in range(nl - 1, 0, -1):
        Ps[l] = block_P(gh.parents[l - 1], dhs[l], dhs[l - 1], gs[l], gs[l - 1])
        As[l - 1] = galerkin(Ps[l].astype(dtype), As[l].astype(dtype), gs[l - 1])
    return As, Ps, gs


def planes(A, sp):
    """(a₁₁, a₁₂, a₂₁, a₂₂) of a dense block matrix as CSR values on the scalar pattern `sp`, and whether anything lies outside the pattern"""
    n = len(sp.rowptr) - 1
    rows = np.repeat(np.arange(n), np.diff(sp.rowptr))
    out, inside = [], np.zeros((n, n), dtype=bool)
    inside[rows, sp.colidx] = True
    clean = True
    for a in (0, 1):
        for b in (0, 1):
            blk = A[a * n:(a + 1) * n, b * n:(b + 1) * n]
            out.append(blk[rows, sp.colidx])
            clean &= not (blk[~inside] != 0.0).any()
    return out, clean


def block_inverse(A, g, mask=True):
    """(b₁₁, b₁₂, b₂₂): the inverse of every node's 2 × 2 diagonal block; mask: zero in the φₑ row and column of a grounded node"""
    n = len(g)
    d = np.diag(A)
    d11, d22, d12 = d[:n], d[n:], A[np.arange(n), n + np.arange(n)]
    det = d11 * d22 - d12 * d12
    b11, b12, b22 = d22 / det, -d12 / det, d11 / det
    if mask:
        b11 = np.where(g, 1.0 / d11, b11)
        b12, b22 = np.where(g, 0.0, b12), np.where(g, 0.0, b22)
    return b11, b12, b22


def apply_blocks(binv, v):
    b11, b12, b22 = binv
    n = len(b11)
    return np.concatenate([b11 * v[:n] + b12 * v[n:], b12 * v[:n] + b22 * v[n:]])


def lambda_star(A, g):
    """λmax(B⁻¹𝒜) as the largest eigenvalue of the dense B^-½ 𝒜 B^-½ (closed-form 2 × 2 square roots through their eigen-decompositions)"""
    n = len(g)
    idx = np.arange(n)
    B = np.empty((n, 2, 2))
    B[:, 0, 0], B[:, 1, 1] = np.diag(A)[:n], np.diag(A)[n:]
    B[:, 0, 1] = B[:, 1, 0] = A[idx, n + idx]
    w, V = np.linalg.eigh(B)
    assert (w > 0.0).all()
    R = np.einsum("nij,nj,nkj->nik", V, 1.0 / np.sqrt(w), V)
    r00, r01, r11 = R[:, 0, 0, None], R[:, 0, 1, None], R[:, 1, 1, None]
    SA = np.vstack([r00 * A[:n] + r01 * A[n:], r01 * A[:n] + r11 * A[n:]])                                # S = [[R₀₀, R₀₁], [R₀₁, R₁₁]], diagonal blocks
    C = np.hstack([SA[:, :n] * r00.T + SA[:, n:] * r01.T, SA[:, :n] * r01.T + SA[:, n:] * r11.T])
    return float(np.linalg.eigvalsh(0.5 * (C + C.T))[-1])


def chebyshev(A, binv, lmax, ratio, degree, r, x=None):
    """`degree` steps of the Chebyshev iteration on B⁻¹𝒜 for 𝒜 x = r (Saad, Alg. 12.1: the recurrences of k_mg_cheb), from x (None: zero); the arithmetic
    runs in the dtype of A and r"""
    lmin = lmax / ratio
    theta, delta = 0.5 * (lmax + lmin), 0.5 * (lmax - lmin)
    sigma1 = theta / delta
    rho = 1.0 / sigma1
    x = np.zeros_like(r) if x is None else x.copy()
    d = apply_blocks(binv, r - A @ x) / theta
    x = x + d
    for _ in range(1, degree):
        rho_new = 1.0 / (2.0 * sigma1 - rho)
        d = rho_new * rho * d + 2.0 * rho_new / delta * apply_blocks(binv, r - A @ x)
        x = x + d
        rho = rho_new
    return x


class Cycle:
    """ℳ⁻¹ of a hierarchy: V(degree, degree) from zero, masked block-Jacobi–Chebyshev smoothing, exact coarsest solve.  dtype np.longdouble: every
    product and sum in extended precision and the coarsest solve refined (bidomain_reference.solve_refined) — what the float64 cycle is measured against."""

    def __init__(self, As, Ps, gs, lmax, degree, ratio, dtype=np.float64):
        self.dtype, self.degree, self.ratio, self.lmax, self.gs = dtype, degree, ratio, lmax, gs
        self.A0 = np.asarray(As[0], dtype=np.float64)          # what the LU factorisation of the coarsest solve sees
        self.As = [a.astype(dtype) for a in As]
        self.Ps = [None if p is None else p.astype(dtype) for p in Ps]
        self.binv = [None] + [tuple(b.astype(dtype) for b in block_inverse(As[l], gs[l])) for l in range(1, len(As))]

    def coarsest(self, r):
        if self.dtype is np.float64:
            return np.linalg.solve(self.A0, r)
        x = bref.solve_refined(self.A0, r.astype(np.float64), steps=3).astype(self.dtype)
        for _ in range(2):                                       # two more refinements with the extended-precision operator and residual carried in full
            res = r - self.As[0] @ x
            x = x + np.linalg.solve(self.A0, res.astype(np.float64)).astype(self.dtype)
        return x

    def __call__(self, r, level=None):
        l = len(self.As) - 1 if level is None else level
        r = np.asarray(r, dtype=self.dtype)
        if l == 0:
            return self.coarsest(r)
        A, P = self.As[l], self.Ps[l]
        x = chebyshev(A, self.binv[l], self.lmax[l], self.ratio, self.degree, r)
        x = x + P @ self(P.T @ (r - A @ x), l - 1)
        return chebyshev(A, self.binv[l], self.lmax[l], self.ratio, self.degree, r, x)


def pcg(A, b, precondition, rtol, maxiter):
    """preconditioned conjugate gradients from x = 0 with the stopping rule of the device solvers, ‖r‖₂ ≤ rtol·‖r₀‖₂ → (x, iterations)"""
    x = np.zeros_like(b)
    r = b.copy()
    tol = rtol * np.linalg.norm(r)
    z = precondition(r)
    p, rz = z.copy(), r @ z
    it = 0
    while np.linalg.norm(r) > tol and it < maxiter:
        Ap = A @ p
        alpha = rz / (p @ Ap)
        x += alpha * p
        r -= alpha * Ap
        it += 1
        z = precondition(r)
        rz_new = r @ z
        p = z + (rz_new / rz) * p
        rz = rz_new
    return x, it


def block_jacobi(A, g):
    binv = block_inverse(A, g, mask=False)
    return lambda r: apply_blocks(binv, r)


def reference_deviation(problem, kind, degree, ratio, rhs_seed=41, n_rhs=3):
    """the float64 reference's own error: max |z − z_ld| / max |z_ld| over `n_rhs` right-hand sides, z from the float64 chain and cycle, z_ld from the
    chain and the cycle accumulated in np.longdouble with the coarsest solve refined; λmax = 1.05 λ* for both.  Returns (whole, cycle alone): `cycle
    alone` feeds both cycles the float64 chain, so it leaves out what the rounding of the coarse operators does to z"""
    lv = reference_levels(problem, kind)
    As, Ps, gs = lv["As"], lv["Ps"], lv["gs"]
    Al, _, _ = hierarchy(problem["gh"], problem["dhs"], lv["A"], lv["flags"], dtype=np.longdouble)
    lmax = [None if v is None else 1.05 * v for v in lambda_stars(As, gs)]
    c64 = Cycle(As, Ps, gs, lmax, degree, ratio)
    cld, cld_same_chain = Cycle(Al, Ps, gs, lmax, degree, ratio, dtype=np.longdouble), Cycle(As, Ps, gs, lmax, degree, ratio, dtype=np.longdouble)
    rng = np.random.default_rng(rhs_seed)
    whole = alone = 0.0
    for _ in range(n_rhs):
        r = rng.normal(size=len(lv["A"]))
        z, a, b = c64(r), cld(r), cld_same_chain(r)
        whole = max(whole, float(np.abs(z - a).max() / np.abs(a).max()))
        alone = max(alone, float(np.abs(z - b).max() / np.abs(b).max()))
    return whole, alone


def lambda_stars(As, gs):
    return [None] + [lambda_star(As[l], gs[l]) for l in range(1, len(As))]


# ---- the problems of the tests
def build_problem(tb, oracle, name):
    """grid hierarchy, per-level handlers and patterns (coarsest first) and the oracle's (M, Kᵢ, Kₑ) on the finest grid of mesh `name`"""
    nel, refinements, extent = MESHES[name]
    gh = tb.GridHierarchy(tb.generate_mesh(tb.Hexahedron, nel, (0.0, 0.0, 0.0), extent), refinements)
    dhs = [tb.DofHandler(g) for g in gh.grids]
    sps = [tb.allocate_matrix(d) for d in dhs]
    host = bref.oracle_matrices(tb, oracle, gh.grids[-1], dhs[-1], sps[-1])
    return dict(name=name, gh=gh, dhs=dhs, sps=sps, host=host, n=dhs[-1].ndofs)


def ground_dofs(problem, kind):
    return np.unique(scalar_dofs(problem["dhs"][-1])[ground_nodes(problem["gh"], kind)])


def reference_levels(problem, kind, dt=bref.DT):
    """the eliminated fine matrix and its hierarchy under ground `kind` → dict(A, As, Ps, gs, ground, ground_diag)"""
    sp, (M, Ki, Ke) = problem["sps"][-1], problem["host"]
    ground = ground_dofs(problem, kind)
    gd = bref.ground_diagonal(sp.rowptr, sp.colidx, Ki, Ke, dt)
    A = bref.block_matrix(sp.rowptr, sp.colidx, M, Ki, Ke, dt, ground, gd)
    flags = np.zeros(problem["n"], dtype=bool)
    flags[ground] = True
    As, Ps, gs = hierarchy(problem["gh"], problem["dhs"], A, flags)
    return dict(A=A, As=As, Ps=Ps, gs=gs, ground=ground, ground_diag=gd, flags=flags)
