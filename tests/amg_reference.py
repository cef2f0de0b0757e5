"""SciPy restatement of the smoothed-aggregation multigrid of csrc/tb_amg.hip (the method as include/tbhip.h states it): strength of connection,
the three aggregation passes, the tentative and smoothed prolongators, the Galerkin operators, the V(degree, degree) Chebyshev–Jacobi cycle and a plain
preconditioned CG.  λmax(D⁻¹A) per level is an input (a list, or a callable A → λ), as multigrid_reference.vcycle takes it.  Patterns are structural:
stored zeros count (an eliminated row keeps its entries)."""
import numpy as np
import scipy.sparse as sp


# ------------------------------------------------------------------------------------------------ matrices of the tests (host only)
def q1_1d(n_nodes, h):
    """1-D linear-element stiffness and mass matrices on n_nodes equidistant nodes"""
    e = np.ones(n_nodes)
    K = sp.diags([-e[:-1], 2 * e, -e[:-1]], [-1, 0, 1]).tolil()
    M = sp.diags([e[:-1], 4 * e, e[:-1]], [-1, 0, 1]).tolil()
    K[0, 0] = K[-1, -1] = 1.0
    M[0, 0] = M[-1, -1] = 2.0
    return sp.csr_matrix(K) / h, sp.csr_matrix(M) * (h / 6.0)


def q1_box(n_nodes, tensor=(1.0, 1.0, 1.0), mass=0.0):
    """the trilinear stiffness matrix of −∇·(diag(tensor)∇) on the unit cube with n_nodes³ nodes (x fastest), plus mass·M"""
    K1, M1 = q1_1d(n_nodes, 1.0 / (n_nodes - 1))
    k3 = lambda a, b, c: sp.kron(sp.kron(c, b), a)
    A = tensor[0] * k3(K1, M1, M1) + tensor[1] * k3(M1, K1, M1) + tensor[2] * k3(M1, M1, K1) + mass * k3(M1, M1, M1)
    return canonical(A)


def p1_stiffness(xyz, conn):
    """linear-tetrahedron stiffness matrix of the Laplacian"""
    X = xyz[conn]                                            # (nc, 4, 3)
    J = np.stack([X[:, 1] - X[:, 0], X[:, 2] - X[:, 0], X[:, 3] - X[:, 0]], axis=2)
    vol = np.abs(np.linalg.det(J)) / 6.0
    Ji = np.linalg.inv(J)                                    # rows: gradients of λ1, λ2, λ3
    G = np.concatenate([-Ji.sum(axis=1, keepdims=True), Ji], axis=1)   # (nc, 4, 3)
    Ke = np.einsum("cik,cjk,c->cij", G, G, vol)
    rows = np.repeat(conn, 4, axis=1).ravel()
    cols = np.tile(conn, (1, 4)).ravel()
    return canonical(sp.csr_matrix((Ke.ravel(), (rows, cols)), shape=(len(xyz), len(xyz))))


def canonical(A):
    A = sp.csr_matrix(A)
    A.sum_duplicates()
    A.sort_indices()
    return A


def eliminate(A, dofs):
    """apply_zero: rows and columns of `dofs` zeroed in place of the pattern (stored zeros stay), the mean diagonal on theirs"""
    A = canonical(A).copy()
    flag = np.zeros(A.shape[0], dtype=bool)
    flag[dofs] = True
    rows = np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))
    mean = A.diagonal().mean()
    A.data[flag[rows] | flag[A.indices]] = 0.0
    A.data[(rows == A.indices) & flag[rows]] = mean
    return A


# ------------------------------------------------------------------------------------------------ steps 1, 2: strength, aggregates
def rows_of(A):
    return np.repeat(np.arange(A.shape[0]), np.diff(A.indptr))


def strength_margin(A, comp, theta):
    """smallest relative distance of any |a_ij| (off the diagonal, same component) from θ·m_i: the tests' matrices have no ties"""
    A = canonical(A)
    m, same, rows = _rowmax(A, comp)
    t = theta * m[rows]
    sel = same & (m[rows] > 0)
    return float(np.min(np.abs(np.abs(A.data[sel]) - t[sel]) / t[sel])) if sel.any() else np.inf


def _rowmax(A, comp):
    n = A.shape[0]
    comp = np.zeros(n, dtype=np.int8) if comp is None else np.asarray(comp)
    rows = rows_of(A)
    same = (rows != A.indices) & (comp[rows] == comp[A.indices])
    m = np.zeros(n)
    np.maximum.at(m, rows[same], np.abs(A.data[same]))
    return m, same, rows


def strength(A, comp=None, theta=0.25):
    """one byte per stored entry of A (canonical order): strong from i or from j"""
    A = canonical(A)
    m, same, rows = _rowmax(A, comp)
    from_i = same & (m[rows] > 0) & (np.abs(A.data) >= theta * m[rows])
    S = sp.csr_matrix((from_i.astype(np.int8), A.indices, A.indptr), shape=A.shape)
    St = canonical(S.T)                                      # symmetric pattern: the transpose has A's pattern, entry for entry
    assert np.array_equal(St.indptr, A.indptr) and np.array_equal(St.indices, A.indices), "the pattern is not structurally symmetric"
    return ((from_i != 0) | (St.data != 0)).astype(np.uint8)


def aggregate(indptr, indices, S):
    n = len(indptr) - 1
    nbrs = [indices[indptr[i]:indptr[i + 1]][S[indptr[i]:indptr[i + 1]] != 0] for i in range(n)]
    agg = np.full(n, -1, dtype=np.int32)
    na = 0
    for i in range(n):                                       # pass 1
        if agg[i] < 0 and len(nbrs[i]) and (agg[nbrs[i]] < 0).all():
            agg[i] = na
            agg[nbrs[i]] = na
            na += 1
    snap = agg.copy()
    for i in range(n):                                       # pass 2
        if snap[i] < 0:
            done = nbrs[i][snap[nbrs[i]] >= 0]
            if len(done):
                agg[i] = snap[done.min()]
    for i in range(n):                                       # pass 3
        if agg[i] < 0 and len(nbrs[i]):
            agg[i] = na
            free = nbrs[i][agg[nbrs[i]] < 0]
            agg[free] = na
            na += 1
    return agg, na


# ------------------------------------------------------------------------------------------------ steps 3 – 5: transfers and coarse operator
def structure(A):
    A = canonical(A)
    return sp.csr_matrix((np.ones(len(A.indices)), A.indices.copy(), A.indptr.copy()), shape=A.shape)


def pattern_of(B):
    B = canonical(B)
    return B.indptr.astype(np.int64), B.indices.astype(np.int32)


def tentative(agg, na):
    inside = np.flatnonzero(agg >= 0)
    size = np.bincount(agg[inside], minlength=na)
    return sp.csr_matrix((1.0 / np.sqrt(size[agg[inside]]), (inside, agg[inside])), shape=(len(agg), na)), size


def plan(A, comp, S):
    """aggregates and the structural patterns of P, R (with the permutation from P's values), A·P and A_c, as the host planner records them"""
    A = canonical(A)
    agg, na = aggregate(A.indptr, A.indices, S)
    T, size = tentative(agg, na)
    inside = sp.diags((agg >= 0).astype(float))
    sA = structure(A)
    P = canonical(inside @ (sA @ structure(T)))
    P.eliminate_zeros()
    P = structure(P)
    numbered = sp.csr_matrix((np.arange(1, P.nnz + 1, dtype=np.float64), P.indices, P.indptr), shape=P.shape)
    R = canonical(numbered.T)
    AP = structure(canonical(sA @ P))
    Ac = structure(canonical(structure(R) @ AP))
    ccomp = np.zeros(na, dtype=np.int8)
    if comp is not None:
        ccomp[agg[agg >= 0]] = np.asarray(comp)[agg >= 0]
    return dict(agg=agg, na=na, size=size, ccomp=ccomp, P=pattern_of(P), R=pattern_of(R), r_perm=(R.data - 1).astype(np.int64), AP=pattern_of(AP),
                Ac=pattern_of(Ac))


def inverse_diagonal(A):
    d = A.diagonal()
    return np.where(d != 0.0, 1.0 / np.where(d != 0.0, d, 1.0), 0.0)


def on_pattern(B, pattern, shape):
    """the values of B at the positions of a structural pattern (stored zeros where B has none)"""
    ptr, col = pattern
    rows = np.repeat(np.arange(shape[0]), np.diff(ptr))
    vals = np.asarray(sp.csr_matrix(B)[rows, col]).ravel() if len(col) else np.zeros(0)
    return sp.csr_matrix((vals, col, ptr), shape=shape)


def lambda_max_exact(A):
    """λmax(D⁻¹A) of the rows that have a diagonal"""
    dinv = inverse_diagonal(A)
    s = np.sqrt(np.abs(dinv))
    B = sp.diags(s) @ A @ sp.diags(s)
    if A.shape[0] <= 1500:
        return float(np.linalg.eigvalsh(B.toarray())[-1])
    import scipy.sparse.linalg as spla
    return float(spla.eigsh(B, k=1, which="LA", tol=1e-10)[0][0])


def hierarchy(A, comp=None, lam=None, theta=0.25, max_coarse=1024, max_levels=16):
    """levels[l]: dict(A, comp, lam, and — but for the last — S, agg, plan, P).  lam: list of λ per level, or a callable A → λ (default: 1.05 × the exact one)"""
    lam_of = (lambda l, M: lam[l]) if isinstance(lam, (list, tuple)) else (lambda l, M: (lam or (lambda B: 1.05 * lambda_max_exact(B)))(M))
    levels = []
    A = canonical(A)
    while True:
        l = len(levels)
        lev = dict(A=A, comp=comp)
        levels.append(lev)
        n = A.shape[0]
        if n <= max_coarse or l + 1 >= max_levels:
            break
        S = strength(A, comp, theta)
        pl = plan(A, comp, S)
        if pl["na"] == 0 or pl["na"] >= n:
            break
        lev.update(S=S, agg=pl["agg"], plan=pl, lam=lam_of(l, A))
        T, _ = tentative(pl["agg"], pl["na"])
        inside = sp.diags((pl["agg"] >= 0).astype(float))
        omega = 4.0 / (3.0 * lev["lam"])
        P = on_pattern(inside @ (T - omega * (sp.diags(inverse_diagonal(A)) @ (A @ T))), pl["P"], (n, pl["na"]))
        lev["P"] = P
        A = on_pattern(P.T @ (A @ P), pl["Ac"], (pl["na"], pl["na"]))
        comp = pl["ccomp"] if comp is not None else None
    return levels


# ------------------------------------------------------------------------------------------------ step 7: the cycle, and CG
def chebyshev(A, dinv, lmax, ratio, degree, r, x=None):
    """the smoother of tb_multigrid.hip's smooth(): `degree` Chebyshev steps on D⁻¹A over [lmax / ratio, lmax] (Saad, Alg. 12.1)"""
    lmin = lmax / ratio
    theta, delta = 0.5 * (lmax + lmin), 0.5 * (lmax - lmin)
    sigma1 = theta / delta
    rho = 1.0 / sigma1
    if x is None:
        d = dinv * r / theta
        x = d.copy()
    else:
        d = dinv * (r - A @ x) / theta
        x = x + d
    for _ in range(1, degree):
        rho_new = 1.0 / (2.0 * sigma1 - rho)
        d = rho_new * rho * d + 2.0 * rho_new / delta * dinv * (r - A @ x)
        x = x + d
        rho = rho_new
    return x


def vcycle(levels, r, degree=2, ratio=4.0, l=0):
    lev = levels[l]
    A = lev["A"]
    if l == len(levels) - 1:
        return np.linalg.solve(A.toarray(), r)
    dinv = inverse_diagonal(A)
    x = chebyshev(A, dinv, lev["lam"], ratio, degree, r)
    P = lev["P"]
    x = x + P @ vcycle(levels, P.T @ (r - A @ x), degree, ratio, l + 1)
    return chebyshev(A, dinv, lev["lam"], ratio, degree, r, x)


def pcg(A, b, M=None, rtol=1e-8, atol=0.0, maxiter=1000, x0=None):
    """plain preconditioned CG with the stopping rule of tb_pcg_solve: ‖r‖ ≤ atol + rtol·‖r₀‖ → (x, iterations, ‖r‖)"""
    x = np.zeros_like(b) if x0 is None else x0.copy()
    r = b - A @ x
    rnorm = np.linalg.norm(r)
    tol = atol + rtol * rnorm
    p = np.zeros_like(b)
    rz = 0.0
    it = 0
    while rnorm > tol and it < maxiter:
        z = M(r) if M is not None else r.copy()
        rz_new = r @ z
        p = z + (rz_new / rz if rz > 0 else 0.0) * p
        Ap = A @ p
        alpha = rz_new / (p @ Ap)
        x += alpha * p
        r -= alpha * Ap
        rz = rz_new
        rnorm = np.linalg.norm(r)
        it += 1
    return x, it, rnorm


def jacobi(A):
    dinv = inverse_diagonal(A)
    return lambda r: dinv * r
