"""SciPy restatement of the algebraic multigrid preconditioner of the bidomain block system (csrc/tb_bidomain_amg.hip, the method as include/tbhip.h
states it).  It composes amg_reference — the smoothed-aggregation hierarchy on the φₑφₑ plane with the elimination of the ground baked in — with
bidomain_mg_reference — the masked 2 × 2 block inverses, the Chebyshev recurrences on B⁻¹𝒜 and the V-cycle recursion: block transfer 𝒫 = P ⊗ I₂, coarse
operators 𝒫ᵀ𝒜𝒫, no ground below the finest level.  Both λmax per level are inputs, as in the restatements it is made of: λ(D⁻¹a₂₂) for the smoothing of P
(default 1.05 × the exact one) and λ(B⁻¹𝒜) for the smoother (default 1.05 × lambda_star).  Nothing here imports the package.  Unknowns are ordered
BLOCKED, (φₘ; φₑ), as in bidomain_reference; matrices are scipy.sparse, levels are listed finest first, as amg_reference does."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import amg_reference as aref
import bidomain_mg_reference as bmref


def block_system(rowptr, colidx, M, Ki, Ke, dt, ground, ground_diag=None):
    """the grounded block matrix [[M − ΔtKᵢ, −ΔtKᵢ], [−ΔtKᵢ, −Δt(Kᵢ + Kₑ)]] (CSR value arrays on one pattern, K negative semidefinite) as a sparse matrix
    whose four blocks keep the pattern (stored zeros stay) → (A, flags, ground_diag); ground_diag None: the mean diagonal of the φₑφₑ block"""
    n = len(rowptr) - 1
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    flags = np.zeros(n, dtype=bool)
    flags[np.asarray(ground, dtype=np.int64)] = True
    a11, a12, a22 = M - dt * Ki, -dt * Ki, -dt * (Ki + Ke)
    gd = float(np.mean(a22[rows == colidx])) if ground_diag is None else float(ground_diag)
    gi, gj = flags[rows], flags[colidx]
    a12c, a21 = np.where(gj, 0.0, a12), np.where(gi, 0.0, a12)
    a22 = np.where(gi | gj, 0.0, a22)
    a22[(rows == colidx) & gi] = gd
    return from_planes(rowptr, colidx, (a11, a12c, a21, a22)), flags, gd


def from_planes(rowptr, colidx, planes):
    n = len(rowptr) - 1
    blk = [sp.csr_matrix((np.asarray(p, dtype=np.float64), colidx, rowptr), shape=(n, n)) for p in planes]
    return sp.bmat([[blk[0], blk[1]], [blk[2], blk[3]]], format="csr")


def planes_of(A, pattern):
    """(a₁₁, a₁₂, a₂₁, a₂₂) of a block matrix as CSR values on the scalar `pattern` (rowptr, colidx)"""
    n = A.shape[0] // 2
    A = sp.csr_matrix(A)
    return [aref.on_pattern(A[a * n:(a + 1) * n, b * n:(b + 1) * n], pattern, (n, n)).data for a in (0, 1) for b in (0, 1)]


def auxiliary(A, pattern):
    """the φₑφₑ plane on the scalar pattern, stored zeros kept: what the scalar hierarchy is built on"""
    n = A.shape[0] // 2
    return aref.on_pattern(sp.csr_matrix(A)[n:, n:], pattern, (n, n))


def hierarchy(A, pattern, lam_scalar=None, theta=0.25, max_coarse=128, max_levels=16):
    """levels[l]: dict(A: the block operator, a22: the scalar level matrix, pattern, and — but for the last — agg, plan, P (scalar), PP = P ⊗ I₂, lam)"""
    scalar = aref.hierarchy(auxiliary(A, pattern), None, lam=lam_scalar, theta=theta, max_coarse=max_coarse, max_levels=max_levels)
    levels = []
    A = sp.csr_matrix(A)
    for l, s in enumerate(scalar):
        lev = dict(A=A, a22=s["A"], pattern=aref.pattern_of(aref.structure(s["A"])))
        levels.append(lev)
        if "P" not in s:
            break
        PP = sp.block_diag([s["P"], s["P"]], format="csr")
        lev.update(agg=s["agg"], plan=s["plan"], P=s["P"], PP=PP, lam=s["lam"])
        A = sp.csr_matrix(PP.T @ (A @ PP))
    return levels


def diagonal_blocks(A):
    n = A.shape[0] // 2
    d = A.diagonal()
    return d[:n], np.asarray(A[np.arange(n), n + np.arange(n)]).ravel(), d[n:]


def block_inverse(A, flags=None):
    """(b₁₁, b₁₂, b₂₂) of every node's diagonal block, zero in the φₑ row and column of a flagged node (bidomain_mg_reference.block_inverse, sparse)"""
    d11, d12, d22 = diagonal_blocks(A)
    det = d11 * d22 - d12 * d12
    b11, b12, b22 = d22 / det, -d12 / det, d11 / det
    if flags is not None and flags.any():
        b11 = np.where(flags, 1.0 / d11, b11)
        b12, b22 = np.where(flags, 0.0, b12), np.where(flags, 0.0, b22)
    return b11, b12, b22


def lambda_star(A):
    """λmax(B⁻¹𝒜): the largest eigenvalue of B^-½ 𝒜 B^-½ (bidomain_mg_reference.lambda_star on a sparse operator)"""
    n = A.shape[0] // 2
    d11, d12, d22 = diagonal_blocks(A)
    B = np.empty((n, 2, 2))
    B[:, 0, 0], B[:, 1, 1], B[:, 0, 1], B[:, 1, 0] = d11, d22, d12, d12
    w, V = np.linalg.eigh(B)
    assert (w > 0.0).all()
    R = np.einsum("nij,nj,nkj->nik", V, 1.0 / np.sqrt(w), V)
    S = sp.bmat([[sp.diags(R[:, 0, 0]), sp.diags(R[:, 0, 1])], [sp.diags(R[:, 0, 1]), sp.diags(R[:, 1, 1])]], format="csr")
    Cm = S @ A @ S
    Cm = 0.5 * (Cm + Cm.T)
    if 2 * n <= 1600:
        return float(np.linalg.eigvalsh(Cm.toarray())[-1])
    return float(spla.eigsh(Cm, k=1, which="LA", tol=1e-12)[0][0])


def lambda_stars(levels):
    return [lambda_star(lev["A"]) for lev in levels[:-1]]


class Cycle:
    """ℳ⁻¹: V(degree, degree) from zero — bidomain_mg_reference.Cycle's recursion, finest level first, the ground masked on level 0 only.  `lmax`: the
    block λmax per smoothed level (None: 1.05 × lambda_star).  dtype np.longdouble: operators, transfers and every sum in extended precision and the last
    level's solve refined — what the float64 cycle is measured against."""

    def __init__(self, levels, flags, lmax=None, degree=2, ratio=4.0, dtype=np.float64):
        self.levels, self.degree, self.ratio, self.dtype = levels, degree, ratio, dtype
        self.lmax = [1.05 * v for v in lambda_stars(levels)] if lmax is None else list(lmax)
        self.binv = [tuple(b.astype(dtype) for b in block_inverse(lev["A"], flags if l == 0 else None)) for l, lev in enumerate(levels[:-1])]
        self.last = levels[-1]["A"].toarray()
        if dtype is np.float64:
            self.As, self.Ps = [lev["A"] for lev in levels], [lev["PP"] for lev in levels[:-1]]
        else:
            self.As, self.Ps = [lev["A"].toarray().astype(dtype) for lev in levels], [lev["PP"].toarray().astype(dtype) for lev in levels[:-1]]

    def coarsest(self, r):
        if self.dtype is np.float64:
            return np.linalg.solve(self.last, r)
        x = np.linalg.solve(self.last, r.astype(np.float64)).astype(self.dtype)
        for _ in range(4):
            x = x + np.linalg.solve(self.last, (r - self.As[-1] @ x).astype(np.float64)).astype(self.dtype)
        return x

    def __call__(self, r, l=0):
        r = np.asarray(r, dtype=self.dtype)
        if l == len(self.levels) - 1:
            return self.coarsest(r)
        A, P = self.As[l], self.Ps[l]
        x = bmref.chebyshev(A, self.binv[l], self.lmax[l], self.ratio, self.degree, r)
        x = x + P @ self(P.T @ (r - A @ x), l + 1)
        return bmref.chebyshev(A, self.binv[l], self.lmax[l], self.ratio, self.degree, r, x)


def block_jacobi(A):
    binv = block_inverse(A)
    return lambda r: bmref.apply_blocks(binv, r)


def pcg(A, b, M, rtol=1e-8, maxiter=1000):
    """amg_reference.pcg (the loop and the stopping rule of the device solvers) from x = 0 → (x, iterations)"""
    x, it, _ = aref.pcg(A, b, M, rtol=rtol, atol=0.0, maxiter=maxiter)
    return x, it


def reference_deviation(levels, flags, lmax, degree, ratio, rhs_seed=41, n_rhs=3):
    """the float64 cycle's own error: max |z − z_ld| / max |z_ld| over `n_rhs` right-hand sides, z_ld from the same hierarchy with every sum of the cycle
    in np.longdouble and the last solve refined (bidomain_mg_reference.reference_deviation, `cycle alone`)"""
    c64, cld = Cycle(levels, flags, lmax, degree, ratio), Cycle(levels, flags, lmax, degree, ratio, dtype=np.longdouble)
    rng = np.random.default_rng(rhs_seed)
    dev = 0.0
    for _ in range(n_rhs):
        r = rng.normal(size=levels[0]["A"].shape[0])
        if flags.any():
            r[len(flags):][flags] = 0.0
        z, a = c64(r), cld(r)
        dev = max(dev, float(np.abs(z - a).max() / np.abs(a).max()))
    return dev


# ---- the systems of the CPU tests: Q1 boxes, no package needed
TENSORS = {"aniso": ((1.0, 0.2, 0.2), (1.0, 0.5, 0.5)), "iso": ((1.0, 1.0, 1.0), (1.0, 1.0, 1.0))}
DTS = (0.1, 1.0, 10.0)
GROUNDS = ("vertex", "two", "face")


def box_ground(n_nodes, kind):
    if kind == "vertex":
        return np.array([0])
    if kind == "two":
        return np.array([n_nodes ** 3 // 2, n_nodes ** 3 - 2])          # one in the interior, one more
    if kind == "face":
        return np.flatnonzero(np.arange(n_nodes ** 3) % n_nodes == 0)    # x = 0
    raise KeyError(kind)


def box_system(n_nodes, tensors, dt, ground_kind):
    """(A, pattern, flags) of the Q1 box with n_nodes³ nodes: M the mass, Kᵢ, Kₑ minus the stiffness of diag(tensor) (the sign of heat_system_matrix)"""
    Mm = aref.q1_box(n_nodes, (0.0, 0.0, 0.0), mass=1.0)
    Ki, Ke = aref.q1_box(n_nodes, tensors[0]), aref.q1_box(n_nodes, tensors[1])
    pattern = aref.pattern_of(aref.structure(Ki))
    vals = lambda B: aref.on_pattern(B, pattern, B.shape).data
    A, flags, _ = block_system(pattern[0], pattern[1], vals(Mm), -vals(Ki), -vals(Ke), dt, box_ground(n_nodes, ground_kind))
    return A, pattern, flags
