"""Textbook restatements of the Krylov layer (csrc/tb_krylov.hip) in extended precision, for tests/test_krylov_reference_cpu.py and
tests/test_krylov_iterates_gpu.py: pure numpy, `np.longdouble` unless a `dtype` says otherwise, no device and no scipy products.

Every recurrence is written the way the layer documents it (not the way its kernels compute it) and returns every iterate x_k, the residual norm the
solver would report at k and the scalars.  `dtype=np.float64` with `order="natural"` / `"reversed"` runs the same code in double in two summation
orders (the tolerance of the device comparison comes from their deviation, `Reference` / `tolerance`); `dtype=object` runs it on mpmath numbers (the reference's
own rounding).  `mutant=` builds one of six defects a self-correcting solver survives into a recurrence; only the CPU test uses them.

Also here, because the CPU and the device test must agree on them: the synthetic systems (`spd_system`, `gmres_system`, `diagonal_system`), the case
table (`CASES`), the metric and the tolerance rule."""
import functools

import numpy as np

LD = np.longdouble
KS = (1, 2, 3, 4, 5, 7)            # iterates compared (maxiter = k with rtol = atol = 0); k = 7 takes launch_cg's three-group rotation round twice
KS_SMALL = (1, 2, 3)               # the 8-dof and the large system
LANCZOS_STEPS = 24
FLOOR = 2.0 ** -50
FACTOR = 16.0
MUTANTS = ("beta_retired", "alpha_previous", "slot_not_zeroed", "direction_from_r", "chebyshev_off_by_one", "givens_wrong_pair")


# ------------------------------------------------------------------------------------------------ arithmetic
def cast(a, dtype=LD):
    """array `a` (doubles: exact in every target) in the arithmetic `dtype`: np.longdouble, np.float64, or object = mpmath numbers"""
    a = np.asarray(a)
    if dtype is object:
        if a.dtype == object:
            return a
        import mpmath
        out = np.empty(a.shape, dtype=object)
        out.ravel()[:] = [mpmath.mpf(float(v)) for v in a.ravel()]
        return out
    return a.astype(dtype)


def to_mp(a):
    """longdouble scalar or array → mpmath numbers, exactly (a 64-bit significand is the sum of two doubles)"""
    import mpmath
    a = np.asarray(a, dtype=LD)
    hi = a.astype(np.float64)
    lo = (a - hi).astype(np.float64)
    out = np.empty(a.shape, dtype=object)
    out.ravel()[:] = [mpmath.mpf(float(h)) + mpmath.mpf(float(l)) for h, l in zip(hi.ravel(), lo.ravel())]
    return out if a.ndim else out[()]


def _sqrt(s):
    if isinstance(s, (float, np.floating)):
        return np.sqrt(s)
    import mpmath
    return mpmath.sqrt(s)


def _sum(t, order):
    return np.sum(t) if order == "natural" else np.sum(np.ascontiguousarray(t[::-1]))


def csr_matvec(rowptr, colidx, vals, x, dtype=LD, order="natural"):
    """y = A·x of a CSR matrix without empty rows; order "reversed": every row summed from its last entry to its first"""
    prod = cast(vals, dtype) * cast(x, dtype)[colidx]
    if order == "natural":
        return np.add.reduceat(prod, rowptr[:-1])
    nnz = len(prod)
    return np.add.reduceat(np.ascontiguousarray(prod[::-1]), np.ascontiguousarray((nnz - rowptr[1:])[::-1]))[::-1].copy()


class Operator:
    """a CSR matrix held in one arithmetic and one summation order"""

    def __init__(self, rowptr, colidx, vals, dtype=LD, order="natural"):
        self.rowptr, self.colidx = np.asarray(rowptr, dtype=np.int64), np.asarray(colidx, dtype=np.int64)
        self.vals, self.dtype, self.order = cast(vals, dtype), dtype, order
        self.n = len(self.rowptr) - 1
        self.rows = np.repeat(np.arange(self.n), np.diff(self.rowptr))
        self.diag = self.vals[self.rows == self.colidx]
        assert len(self.diag) == self.n

    def vec(self, a):
        return cast(a, self.dtype)

    def mv(self, x):
        return csr_matvec(self.rowptr, self.colidx, self.vals, x, self.dtype, self.order)

    def dot(self, a, b):
        return _sum(a * b, self.order)

    def norm(self, a):
        return _sqrt(self.dot(a, a))

    def abs_row_sums(self):
        a = np.abs(self.vals)
        if self.order == "natural":
            return np.add.reduceat(a, self.rowptr[:-1])
        return np.add.reduceat(np.ascontiguousarray(a[::-1]), np.ascontiguousarray((len(a) - self.rowptr[1:])[::-1]))[::-1].copy()


# ------------------------------------------------------------------------------------------------ preconditioners
def jacobi(op):
    dinv = 1 / op.diag
    return lambda r: dinv * r


def l1gs(op, ps):
    """symmetric ℓ₁ Gauss–Seidel on partitions of `ps` consecutive rows: D̃_ii = a_ii + Σ_{j ∉ part(i)} |a_ij|, forward sweep (D̃ + L_p) y = r, then
    backward sweep (D̃ + U_p) z = D̃ y; M = (D̃ + L_p) D̃⁻¹ (D̃ + U_p)"""
    part_r, part_c = op.rows // ps, op.colidx // ps
    outside = np.where(part_r != part_c, np.abs(op.vals), 0 * op.vals)
    dt = op.diag + np.add.reduceat(outside, op.rowptr[:-1])
    lower, upper = [], []
    for i in range(op.n):
        k = np.arange(op.rowptr[i], op.rowptr[i + 1])
        c = op.colidx[k]
        same = c // ps == i // ps
        lower.append((k[same & (c < i)], c[same & (c < i)]))
        upper.append((k[same & (c > i)], c[same & (c > i)]))

    def apply(r):
        y = 0 * r
        for i in range(op.n):
            k, c = lower[i]
            y[i] = (r[i] - op.dot(op.vals[k], y[c])) / dt[i]
        for i in range(op.n - 1, -1, -1):
            k, c = upper[i]
            y[i] = y[i] - op.dot(op.vals[k], y[c]) / dt[i]
        return y
    return apply


def largest_ritz_value(alpha, beta):
    """largest eigenvalue of the symmetric tridiagonal matrix (diagonal alpha[0:m], off-diagonal beta[1:m]).  mpmath numbers: mpmath.eigsy.
    Otherwise LAPACK's symmetric solver in double, and the Rayleigh quotient of its eigenvector in the arithmetic of the entries — the error of a
    Rayleigh quotient is the square of the eigenvector's, so the double eigenvector serves the extended run too"""
    m = len(alpha)
    if not isinstance(alpha[0], (float, np.floating)):
        import mpmath
        T = mpmath.zeros(m, m)
        for k in range(m):
            T[k, k] = alpha[k]
            if k + 1 < m:
                T[k, k + 1] = T[k + 1, k] = beta[k + 1]
        return max(mpmath.eigsy(T, eigvals_only=True))
    a, b = np.array(alpha), np.array(beta[1:m])
    T = np.diag(a.astype(np.float64)) + np.diag(b.astype(np.float64), 1) + np.diag(b.astype(np.float64), -1)
    v = np.linalg.eigh(T)[1][:, -1].astype(a.dtype)
    Tv = a * v
    Tv[:-1] += b * v[1:]
    Tv[1:] += b * v[:-1]
    return np.sum(v * Tv) / np.sum(v * v)


def lambda_max(op, steps=LANCZOS_STEPS):
    """λmax(D⁻¹A) as the layer defines it → dict(lmax, gersh, theta, alpha, beta): the Gershgorin bound of D⁻¹A; `steps` Lanczos steps on
    D^-½ A D^-½ without reorthogonalisation from the Gershgorin row sums times 1 + 0.37·((i·2654435761) & 1023)/1024; min(gersh, 1.05·θmax)"""
    dinv = 1 / op.diag
    rowsum = op.abs_row_sums() * np.abs(dinv)
    gersh = rowsum.max()
    i = np.arange(op.n, dtype=np.uint64)
    pert = ((i * np.uint64(2654435761)) & np.uint64(1023)).astype(np.float64)
    v = rowsum * (1 + op.vec(np.float64(0.37)) * op.vec(pert) / 1024)
    sq = np.array([_sqrt(d) for d in np.abs(dinv)], dtype=op.vals.dtype)
    v = v / op.norm(v)
    vp = 0 * v
    al, be = [], [0 * gersh]
    for k in range(steps):
        w = sq * op.mv(sq * v) - be[k] * vp
        al.append(op.dot(w, v))
        w = w - al[k] * v
        be.append(op.norm(w))
        vp, v = v, w / be[k + 1]                              # (the tests use inputs on which no β comes near zero)
    theta = largest_ritz_value(al, be)
    lmax = min(gersh, op.vec(np.float64(1.05))[()] * theta)
    return dict(lmax=lmax, gersh=gersh, theta=theta, alpha=al, beta=be)


def chebyshev(op, degree, lmax=None, mutant=None):
    """z = p_m(D⁻¹A) D⁻¹ r: Saad, Iterative Methods, Alg. 12.1 started from zero on [λmax / max(4, 1.8 m²), λmax]"""
    dinv = 1 / op.diag
    if lmax is None:
        lmax = lambda_max(op)["lmax"]
    m = max(1, degree)
    lmin = lmax / max(op.vec(np.float64(4.0))[()], op.vec(np.float64(1.8))[()] * m * m)
    theta, delta = (lmax + lmin) / 2, (lmax - lmin) / 2
    sigma1 = theta / delta

    def apply(r):
        rho = 1 / sigma1
        d = dinv * r / theta
        z = d.copy()
        for _ in range(1, m):
            rho_new = 1 / (2 * sigma1 - rho)
            c2 = 2 * (rho if mutant == "chebyshev_off_by_one" else rho_new) / delta
            d = rho_new * rho * d + c2 * (dinv * (r - op.mv(z)))
            z = z + d
            rho = rho_new
        return z
    return apply


# ------------------------------------------------------------------------------------------------ recurrences
def pcg(op, b, x0, k, precond=None, r0=None, mutant=None):
    """Preconditioned CG, k iterations from x0: r = b − A x0 (or the given r0), z = M⁻¹ r, p = z; then α = r·z / pᵀAp, x += α p, r −= α Ap,
    z = M⁻¹ r, β = (r·z)_new / r·z, p = z + β p.  → dict(x = [x_1 … x_k], res = [‖r_0‖ … ‖r_k‖], alpha, beta, rz, pAp)"""
    apply = precond if precond is not None else (lambda r: r)
    x = op.vec(x0)
    r = op.vec(r0) if r0 is not None else op.vec(b) - op.mv(x)
    z = apply(r)
    p = r.copy() if mutant == "direction_from_r" else z.copy()
    rz = [op.dot(r, z)]
    out = dict(x=[], res=[op.norm(r)], alpha=[], beta=[], rz=rz, pAp=[])
    for it in range(k):
        Ap = op.mv(p)
        pAp = op.dot(p, Ap)
        if mutant == "slot_not_zeroed" and it > 0:
            pAp = pAp + out["pAp"][-1]                        # the pᵀAp accumulator was not cleared
        out["pAp"].append(pAp)
        alpha = rz[it] / (out["pAp"][it - 1] if mutant == "alpha_previous" and it > 0 else pAp)
        x = x + alpha * p
        r = r - alpha * Ap
        z = apply(r)
        rz.append(op.dot(r, z))
        beta = rz[it + 1] / (rz[it - 1] if mutant == "beta_retired" and it > 0 else rz[it])
        p = (r if mutant == "direction_from_r" else z) + beta * p
        out["x"].append(x)
        out["res"].append(op.norm(r))
        out["alpha"].append(alpha)
        out["beta"].append(beta)
    return out


def cg_single_reduction(op, b, x0, k):
    """Chronopoulos–Gear CG with Jacobi: u = D⁻¹ r, w = A u, γ = r·u, δ = uᵀA u, ρ = r·r; β = γ/γ_prev (0 first), α = γ / (δ − β γ/α_prev);
    p = u + β p, s = w + β s, x += α p, r −= α s.  → dict(x, res, gamma, delta, rho): entry k of the scalars is their value after k steps"""
    dinv = 1 / op.diag
    x = op.vec(x0)
    r = op.vec(b) - op.mv(x)
    u = dinv * r
    w = op.mv(u)
    gam, dl, rho = op.dot(r, u), op.dot(u, w), op.dot(r, r)
    p, s = 0 * x, 0 * x
    gam_prev = alpha_prev = None
    out = dict(x=[], res=[_sqrt(rho)], gamma=[gam], delta=[dl], rho=[rho])
    for it in range(k):
        beta = gam / gam_prev if it > 0 else 0 * gam
        den = dl - beta * gam / alpha_prev if it > 0 else dl
        alpha = gam / den
        p = u + beta * p
        s = w + beta * s
        x = x + alpha * p
        r = r - alpha * s
        u = dinv * r
        w = op.mv(u)
        gam_prev, alpha_prev = gam, alpha
        gam, dl, rho = op.dot(r, u), op.dot(u, w), op.dot(r, r)
        out["x"].append(x)
        out["res"].append(_sqrt(rho))
        out["gamma"].append(gam)
        out["delta"].append(dl)
        out["rho"].append(rho)
    return out


def _hypot(a, b):
    return _sqrt(a * a + b * b)


def gmres(op, b, x0, k, restart, use_jacobi=True, mutant=None):
    """Restarted GMRES(restart) with right Jacobi preconditioning (A D⁻¹ y = b, x = D⁻¹ y), Gram–Schmidt with one reorthogonalisation pass, Givens
    rotations; x is updated at the end of a cycle and the true residual recomputed there.  x[k − 1] is what a solve limited to k iterations returns
    (its last cycle ends at k), res[k] the true residual norm of that iterate, est[k] the rotated right-hand side's estimate of it, hdiag the
    Hessenberg diagonals after rotation."""
    dinv = 1 / op.diag if use_jacobi else None
    bb = op.vec(b)
    x = op.vec(x0)
    r = bb - op.mv(x)
    rn = op.norm(r)
    out = dict(x=[], res=[rn], est=[rn], hdiag=[])
    it = 0
    while it < k:
        V = [r / rn]
        H, cs, sn, g = [], [], [], [rn]
        for j in range(restart):
            if it >= k:
                break
            w = op.mv(dinv * V[j] if use_jacobi else V[j])
            h1 = [op.dot(v, w) for v in V]
            for c, v in zip(h1, V):
                w = w - c * v
            h2 = [op.dot(v, w) for v in V]
            for c, v in zip(h2, V):
                w = w - c * v
            col = [a + c for a, c in zip(h1, h2)]
            wn = op.norm(w)
            col.append(wn)
            for i in range(j):
                q = j - 1 - i if mutant == "givens_wrong_pair" else i
                col[i], col[i + 1] = cs[q] * col[i] + sn[q] * col[i + 1], -sn[q] * col[i] + cs[q] * col[i + 1]
            den = _hypot(col[j], col[j + 1])
            cs.append(col[j] / den)
            sn.append(col[j + 1] / den)
            col[j], col[j + 1] = den, 0 * den
            g.append(-sn[j] * g[j])
            g[j] = cs[j] * g[j]
            H.append(col)
            out["hdiag"].append(den)
            V.append(w / wn if wn > 0 else w)
            it += 1
            # the iterate a cycle ending here leaves: y = H⁻¹ g (upper triangular), x + D⁻¹ V y
            m = j + 1
            y = [None] * m
            for i in range(m - 1, -1, -1):
                acc = g[i]
                for l in range(i + 1, m):
                    acc = acc - H[l][i] * y[l]
                y[i] = acc / H[i][i]
            t = 0 * x
            for c, v in zip(y, V):
                t = t + c * v
            xk = x + (dinv * t if use_jacobi else t)
            out["x"].append(xk)
            out["res"].append(op.norm(bb - op.mv(xk)))
            out["est"].append(abs(g[m]))
            if not wn > 0:
                break
        x = out["x"][-1]
        r = bb - op.mv(x)
        rn = op.norm(r)
        if not rn > 0:
            break
    return out


# ------------------------------------------------------------------------------------------------ systems
class System:
    """rowptr, colidx, vals of A; b; the two initial guesses x0[False] = 0 and x0[True] = solution-sized random"""

    def __init__(self, name, rowptr, colidx, vals, b, xrand):
        self.name, self.rowptr, self.colidx, self.vals, self.b = name, rowptr, colidx, vals, b
        self.n = len(rowptr) - 1
        self.x0 = {False: np.zeros(self.n), True: xrand}

    @functools.lru_cache(maxsize=None)
    def op(self, dtype=LD, order="natural"):
        return Operator(self.rowptr, self.colidx, self.vals, dtype, order)

    def f32(self):
        """the same system with every input rounded to float32 (held in doubles)"""
        r = lambda a: a.astype(np.float32).astype(np.float64)  # noqa: E731
        return System(self.name + "_f32", self.rowptr, self.colidx, r(self.vals), r(self.b), r(self.x0[True]))


def _transpose_permutation(rowptr, colidx):
    """position of entry (j, i) for every entry (i, j) of a structurally symmetric CSR pattern with sorted rows"""
    n = len(rowptr) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr))
    perm = np.lexsort((rows, colidx))
    assert np.array_equal(colidx[perm], rows) and np.array_equal(rows[perm], colidx), "pattern is not structurally symmetric"
    return rows, perm


def _rhs(rowptr, colidx, vals, xs):
    return csr_matvec(rowptr, colidx, vals, xs).astype(np.float64)


def spd_system(name, rowptr, colidx, seed):
    """symmetrised N(0, 0.3²) off-diagonals, diagonal = Σ|off-diagonal| · U(1.02, 1.5), then two-sided scaling by powers of two 2^randint(−5, 5)
    (exact: the matrix stays exactly symmetric, and Jacobi on or off gives clearly different iterates)"""
    rng = np.random.default_rng(seed)
    colidx = np.asarray(colidx, dtype=np.int64)
    n = len(rowptr) - 1
    rows, perm = _transpose_permutation(rowptr, colidx)
    g = rng.normal(0.0, 0.3, size=len(colidx))
    v = (g + g[perm]) * np.sqrt(0.5)                         # a + b = b + a in floating point: exactly symmetric
    isdiag = rows == colidx
    v[isdiag] = 0.0
    offsum = np.add.reduceat(np.abs(v), rowptr[:-1])
    v[isdiag] = offsum * rng.uniform(1.02, 1.5, size=n) if n > 1 else 1.0
    s = 2.0 ** rng.integers(-5, 5, size=n, endpoint=True)
    v = v * s[rows] * s[colidx]
    xs = rng.normal(size=n) / s
    return System(name, rowptr, colidx, v, _rhs(rowptr, colidx, v, xs), rng.normal(size=n) / s)


def gmres_system(name, rowptr, colidx, seed):
    """non-symmetric and indefinite: N(0, 1) entries, diagonal ±(6 + U(0, 2)) with the minus sign on every third row, rows scaled by powers of two"""
    rng = np.random.default_rng(seed)
    colidx = np.asarray(colidx, dtype=np.int64)
    n = len(rowptr) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr))
    v = rng.normal(size=len(colidx))
    v[rows == colidx] = np.where(np.arange(n) % 3 == 0, -1.0, 1.0) * (6.0 + rng.uniform(0, 2, n))
    s = 2.0 ** rng.integers(-5, 5, size=n, endpoint=True)
    v = v * s[rows]
    xs = rng.normal(size=n)
    return System(name, rowptr, colidx, v, _rhs(rowptr, colidx, v, xs), rng.normal(size=n))


def diagonal_system(name, rowptr, colidx, seed):
    """a diagonal of powers of two stored in the pattern, every off-diagonal zero; b arbitrary"""
    rng = np.random.default_rng(seed)
    colidx = np.asarray(colidx, dtype=np.int64)
    n = len(rowptr) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rowptr))
    v = np.zeros(len(colidx))
    v[rows == colidx] = 2.0 ** rng.integers(-5, 5, size=n, endpoint=True)
    return System(name, rowptr, colidx, v, rng.normal(size=n), np.zeros(n))


LARGE_SEED = 3000
MESHES = {"n8": (1, 1, 1), "n120": (5, 4, 3), "n1716": (12, 11, 10)}      # cells → (nx + 1)(ny + 1)(nz + 1) Q1 dofs
LAMBDA_MESHES = {"mg175": (3, 2, 2), "mg1573": (6, 5, 5)}                 # coarse cells of the two-level hierarchies the λmax check is read through


def large_cube_nodes(n_cu):
    """nodes per edge of the smallest cube with more than max(262 144, 8·n_cu·256) nodes: every grid-stride loop takes a second trip and launch_cg
    looks every iteration"""
    m = 2
    while m ** 3 <= max(262144, 8 * n_cu * 256):
        m += 1
    return m


# ------------------------------------------------------------------------------------------------ cases
class Case:
    """one (system, solver) pair: `run(dtype, order, mutant)` → the recurrence's dict for kmax iterations (the largest checked k)"""

    def __init__(self, system, solver, ks, random_x0, **kw):
        self.system, self.solver, self.ks, self.random_x0, self.kw = system, solver, tuple(ks), bool(random_x0), kw
        self.kmax = max(self.ks)
        self.id = "-".join([system, solver] + ["%s%s" % (a, kw[a]) for a in sorted(kw)] + (["k%d" % ks[0]] if solver == "gmres" else [])
                           + ["x0rand" if random_x0 else "x0zero"])

    def mutants(self):
        """the defects that can act in this case"""
        if self.solver == "gmres":
            return ("givens_wrong_pair",) if self.kw["restart"] >= 3 else ()
        if self.solver == "cg1":
            return ()
        m = ["beta_retired", "alpha_previous", "slot_not_zeroed"]
        if self.solver in ("jacobi", "from_residual", "f32"):
            m.append("direction_from_r")
        if self.solver == "chebyshev" and self.kw["degree"] >= 2:
            m.append("chebyshev_off_by_one")
        return tuple(m)

    def run(self, sysm, dtype=LD, order="natural", mutant=None):
        if self.solver == "f32":
            sysm = sysm.f32()
        op = sysm.op(dtype, order)
        x0, k = sysm.x0[self.random_x0], self.kmax
        if self.solver == "gmres":
            return gmres(op, sysm.b, x0, k, self.kw["restart"], bool(self.kw["jacobi"]), mutant)
        if self.solver == "cg1":
            return cg_single_reduction(op, sysm.b, x0, k)
        if self.solver == "from_residual":
            return pcg(op, None, x0, k, jacobi(op), r0=host_residual(sysm, x0), mutant=mutant)
        pre = {"none": lambda: None, "jacobi": lambda: jacobi(op), "f32": lambda: jacobi(op), "dcg": lambda: jacobi(op), "l1gs": lambda: l1gs(op, self.kw["ps"]),
               "chebyshev": lambda: chebyshev(op, self.kw["degree"], mutant=mutant)}[self.solver]()
        return pcg(op, sysm.b, x0, k, pre, mutant=mutant)


def host_residual(sysm, x0):
    """b − A·x₀ as the caller of tb_cg_solve_from_residual forms it on the host, rounded to double: that rounded vector is the solver's input"""
    return (sysm.b.astype(LD) - csr_matvec(sysm.rowptr, sysm.colidx, sysm.vals, x0)).astype(np.float64)


def _cases():
    """x₀ is zero in half the cases and solution-sized random in the other half, alternating from case to case within a system and starting the
    other way round on the next system, so that every solver sees both starts; tb_cg_solve_from_residual always starts from a random x₀ (with
    x₀ = 0 its input is b itself and it could not be told from the plain solve)"""
    out, flip = [], [False]

    def add(system, solver, ks, **kw):
        out.append(Case(system, solver, ks, flip[0] or solver == "from_residual", **kw))
        flip[0] = not flip[0]
    for start, (s, ks) in enumerate((("n8", KS_SMALL), ("n120", KS), ("n1716", KS))):
        n = {"n8": 8, "n120": 120, "n1716": 1716}[s]
        flip[0] = start % 2 == 1
        add(s, "none", ks)
        add(s, "jacobi", ks)
        add(s, "from_residual", ks)
        for ps in (7, 64, min(n + 5, 1024)):                 # one partition over 120 rows is an exact symmetric Gauss–Seidel: at convergence after k = 4
            add(s, "l1gs", tuple(k for k in ks if k <= 4) if s == "n120" and ps >= n else ks, ps=ps)
        if s != "n8":                                         # 24 Lanczos steps need more than 8 dofs
            for degree in (1, 4):
                add(s, "chebyshev", ks, degree=degree)
        add(s, "f32", ks)
        add(s, "cg1", ks)
        for jac in (0, 1):
            for restart, k in ((4, 3), (4, 4), (4, 6), (1, 3), (30, 7)):
                if s == "n8" and k > 3:
                    continue
                add(s + "g", "gmres", (k,), restart=restart, jacobi=jac)
    add("large", "jacobi", KS_SMALL)
    return out


CASES = _cases()


def case(system, solver, **kw):
    hits = [c for c in CASES if c.system == system and c.solver == solver and c.kw == kw]
    assert len(hits) == 1, (system, solver, kw)
    return hits[0]


# ------------------------------------------------------------------------------------------------ metric and tolerance
def deviation(dx, dx_ref):
    """‖dx − dx_ref‖∞ / ‖dx_ref‖∞ in extended precision"""
    a, r = cast(dx, LD), cast(dx_ref, LD)
    return float(np.abs(a - r).max() / np.abs(r).max())


def relative(a, ref):
    return float(abs(LD(a) - LD(ref)) / abs(LD(ref)))


def tolerance(eps_ref):
    """16 · max(ε_ref, 2⁻⁵⁰): four bits over what double arithmetic in an arbitrary summation order costs on this input (the device's sums are trees
    ending in slot atomics, whose first-order bound is that of a recursive sum in any order); the floor keeps a lucky ε_ref ≈ 0 from demanding bits"""
    return FACTOR * max(eps_ref, FLOOR)


class Reference:
    """the extended-precision run of a case and ε_ref per k: the larger deviation of the two float64 runs (natural and reversed sums) from it"""

    def __init__(self, c, sysm):
        self.case, self.system = c, sysm.f32() if c.solver == "f32" else sysm
        self.x0 = self.system.x0[c.random_x0]
        self.ld = c.run(sysm)
        self.f64 = [c.run(sysm, np.float64, order) for order in ("natural", "reversed")]

    def dx(self, k, run=None):
        return cast((self.ld if run is None else run)["x"][k - 1], LD) - cast(self.x0, LD)

    def eps_x(self, k):
        return max(deviation(self.dx(k, f), self.dx(k)) for f in self.f64)

    def eps_scalar(self, key, k):
        return max(relative(f[key][k], self.ld[key][k]) for f in self.f64)

    def tol_x(self, k):
        return tolerance(self.eps_x(k))

    def tol_scalar(self, key, k):
        return tolerance(self.eps_scalar(key, k))


def rtol_for(res, kstar):
    """a relative tolerance the residual history `res` first meets at iteration kstar: midway (geometrically) between ‖r_{k*−1}‖ and ‖r_{k*}‖"""
    return float(_sqrt(res[kstar - 1] * res[kstar]) / res[0])


# ------------------------------------------------------------------------------------------------ iteration counts
class CountCase(Case):
    """a solve with rtol > 0 that the reference first satisfies at iteration kstar; `returned`: the count the solver must report — launch_cg below
    262 144 rows looks every fourth iteration (min(maxiter, 4·⌈k*/4⌉) for k* ≤ 32), every other solver and the large system look every iteration"""

    def __init__(self, system, solver, kstar, maxiter=50, **kw):
        coarse = solver in ("none", "jacobi", "from_residual", "f32") and system != "large"
        self.kstar, self.maxiter = kstar, maxiter
        self.returned = min(maxiter, 4 * -(-kstar // 4)) if coarse else kstar
        Case.__init__(self, system, solver, (self.returned,), system != "large" and kstar % 2 == 1, **kw)
        self.kmax = max(kstar, self.returned)
        self.id = "%s-kstar%d-maxiter%d" % (self.id, kstar, maxiter)


COUNT_CASES = [CountCase("n1716", "jacobi", 3), CountCase("n1716", "jacobi", 7), CountCase("n1716", "jacobi", 7, maxiter=6),
               CountCase("n120", "from_residual", 3), CountCase("n1716", "f32", 3), CountCase("large", "jacobi", 3),
               CountCase("n120", "l1gs", 3, ps=125), CountCase("n1716", "chebyshev", 3, degree=4),
               CountCase("n8g", "gmres", 3, restart=4, jacobi=1), CountCase("n8g", "gmres", 4, restart=30, jacobi=1),
               CountCase("n120", "gmres", 6, restart=30, jacobi=1), CountCase("n120", "gmres", 6, restart=4, jacobi=1),
               CountCase("n1716", "dcg", 3), CountCase("n1716", "cg1", 3)]


def meshes(tb):
    """name → (DofHandler, SparsityPattern, GridHierarchy or None) of the package `tb` (host work only): the Q1 patterns of MESHES, and for
    LAMBDA_MESHES the finest grid of a two-level hierarchy"""
    out = {}
    for name, nel in MESHES.items():
        dh = tb.DofHandler(tb.generate_mesh(tb.Hexahedron, nel, (0, 0, 0), (1, 1, 1)))
        out[name] = (dh, tb.allocate_matrix(dh), None)
    for name, nel in LAMBDA_MESHES.items():
        gh = tb.GridHierarchy(tb.generate_mesh(tb.Hexahedron, nel, (0, 0, 0), (1, 1, 1)), 1)
        dh = tb.DofHandler(gh.grids[-1])
        out[name] = (dh, tb.allocate_matrix(dh), gh)
    return out


def large_mesh(tb, n_cu):
    m = large_cube_nodes(n_cu)
    dh = tb.DofHandler(tb.generate_mesh(tb.Hexahedron, (m - 1,) * 3, (0, 0, 0), (1, 1, 1)))
    return dh, tb.allocate_matrix(dh), None


def build_systems(msh):
    """msh: `meshes(tb)`, optionally with "large" → every system of the tests on those patterns"""
    out = {}
    for i, name in enumerate(sorted(MESHES)):
        sp = msh[name][1]
        out[name] = spd_system(name, sp.rowptr, sp.colidx, 1000 + i)
        out[name + "g"] = gmres_system(name + "g", sp.rowptr, sp.colidx, 2000 + i)
    for i, name in enumerate(sorted(LAMBDA_MESHES)):
        out[name] = spd_system(name, msh[name][1].rowptr, msh[name][1].colidx, 4000 + i)
    if "large" in msh:
        out["large"] = spd_system("large", msh["large"][1].rowptr, msh["large"][1].colidx, LARGE_SEED)
    return out


_REFERENCES = {}


def reference(c, systems):
    """the Reference of a case, computed once per process"""
    if c.id not in _REFERENCES:
        _REFERENCES[c.id] = Reference(c, systems[c.system])
    return _REFERENCES[c.id]

