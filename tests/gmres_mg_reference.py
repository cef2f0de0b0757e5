"""Restarted GMRES with a fixed right preconditioner given as a callable (launch_gmres_apply of csrc/tb_krylov.hip: tb_gmres_solve_mg, tb_gmres_solve_amg)
in extended precision, in the style of tests/krylov_reference.py, whose arithmetic helpers, metric and tolerance rule it imports: pure numpy,
`np.longdouble` unless a `dtype` says otherwise, `dtype=np.float64` with `order="natural"` / `"reversed"` for the two double runs the tolerance of a
device comparison comes from.

`apply_M(v)` → M⁻¹ v is any callable.  In the CPU test it is a dense matrix.  In the device test it rounds v to double, runs the hierarchy's own `apply`
on the device and returns the result: the reference then uses the very operator the device solver uses, rounding included, and nothing has to be
probed out of M.  Also here, because several device tests share them: the skewed test matrices and the helpers that read a CSR."""
import numpy as np

import krylov_reference as kr

LD = kr.LD


def right_gmres(matvec, apply_M, b, x0, k, restart, dtype=LD, order="natural"):
    """k Arnoldi steps of GMRES(restart) on A M⁻¹ y = b, x = M⁻¹ y, from x0: per step z = M⁻¹ v_j, w = A z, Gram–Schmidt with one reorthogonalisation
    pass, Givens rotations; x is updated at the end of a cycle by x += M⁻¹(V y) and the true residual recomputed there.  `matvec(x)` → A·x in `dtype`.
    → dict(x, res, est, hdiag) as krylov_reference.gmres: x[k − 1] is what a solve limited to k steps returns (its last cycle ends at k), res[k] the
    true residual norm of that iterate, est[k] the estimate |g_{k+1}| the solver compares with its threshold at step k."""
    vec = lambda a: kr.cast(a, dtype)                         # noqa: E731
    dot = lambda a, c: kr._sum(a * c, order)                  # noqa: E731
    norm = lambda a: kr._sqrt(dot(a, a))                      # noqa: E731
    M = lambda v: vec(apply_M(v))                             # noqa: E731
    bb, x = vec(b), vec(x0)
    r = bb - matvec(x)
    rn = norm(r)
    out = dict(x=[], res=[rn], est=[rn], hdiag=[])
    it = 0
    while it < k:
        V = [r / rn]
        H, cs, sn, g = [], [], [], [rn]
        for j in range(restart):
            if it >= k:
                break
            w = matvec(M(V[j]))
            h1 = [dot(v, w) for v in V]
            for c, v in zip(h1, V):
                w = w - c * v
            h2 = [dot(v, w) for v in V]
            for c, v in zip(h2, V):
                w = w - c * v
            col = [a + c for a, c in zip(h1, h2)]
            wn = norm(w)
            col.append(wn)
            for i in range(j):
                col[i], col[i + 1] = cs[i] * col[i] + sn[i] * col[i + 1], -sn[i] * col[i] + cs[i] * col[i + 1]
            den = kr._hypot(col[j], col[j + 1])
            cs.append(col[j] / den)
            sn.append(col[j + 1] / den)
            col[j], col[j + 1] = den, 0 * den
            g.append(-sn[j] * g[j])
            g[j] = cs[j] * g[j]
            H.append(col)
            out["hdiag"].append(den)
            V.append(w / wn if wn > 0 else w)
            it += 1
            m = j + 1                                         # the iterate a cycle ending here leaves: y = H⁻¹ g, x + M⁻¹(V y)
            y = [None] * m
            for i in range(m - 1, -1, -1):
                acc = g[i]
                for l in range(i + 1, m):
                    acc = acc - H[l][i] * y[l]
                y[i] = acc / H[i][i]
            t = 0 * x
            for c, v in zip(y, V):
                t = t + c * v
            xk = x + M(t)
            out["x"].append(xk)
            out["res"].append(norm(bb - matvec(xk)))
            out["est"].append(abs(g[m]))
            if not wn > 0:
                break
        x = out["x"][-1]
        r = bb - matvec(x)
        rn = norm(r)
        if not rn > 0:
            break
    return out


class Reference:
    """the extended-precision run of one (matrix, M⁻¹, b, x0, kmax, restart) and the two float64 runs; ε_ref per k as krylov_reference.Reference"""

    def __init__(self, rowptr, colidx, vals, apply_M, b, x0, kmax, restart):
        self.x0 = x0
        runs = []
        for dtype, order in ((LD, "natural"), (np.float64, "natural"), (np.float64, "reversed")):
            op = kr.Operator(rowptr, colidx, vals, dtype, order)
            runs.append(right_gmres(op.mv, apply_M, b, x0, kmax, restart, dtype, order))
        self.ld, self.f64 = runs[0], runs[1:]

    def dx(self, k, run=None):
        return kr.cast((self.ld if run is None else run)["x"][k - 1], LD) - kr.cast(self.x0, LD)

    def eps_x(self, k):
        return max(kr.deviation(self.dx(k, f), self.dx(k)) for f in self.f64)

    def tol_x(self, k):
        return kr.tolerance(self.eps_x(k))

    def tol_scalar(self, key, k):
        return kr.tolerance(max(kr.relative(f[key][k], self.ld[key][k]) for f in self.f64))


# ------------------------------------------------------------------------------------------------ matrices
def skewed(rowptr, colidx, vals, seed, s=0.1, untouched=()):
    """vals with a seeded skew term on the stored pattern: A_ij += s·σ_ij·√(A_ii A_jj), σ antisymmetric in [−1, 1] (σ_ii = 0); rows and columns of the
    dofs in `untouched` (eliminated Dirichlet rows) stay as they are.  The pattern must be structurally symmetric with a stored diagonal."""
    rowptr, colidx = np.asarray(rowptr, dtype=np.int64), np.asarray(colidx, dtype=np.int64)
    rows, perm = kr._transpose_permutation(rowptr, colidx)
    n = len(rowptr) - 1
    diag = np.zeros(n)
    diag[rows[rows == colidx]] = vals[rows == colidx]
    assert (diag > 0).all(), "the skew term scales with the square roots of the diagonal"
    u = np.random.default_rng(seed).uniform(-1.0, 1.0, size=len(colidx))
    upper = rows < colidx
    sigma = np.where(upper, u, 0.0)
    sigma = sigma - sigma[perm]                               # σ_ji = −σ_ij exactly, σ_ii = 0
    keep = np.ones(n, dtype=bool)
    keep[np.asarray(untouched, dtype=np.int64)] = False
    sigma = np.where(keep[rows] & keep[colidx], sigma, 0.0)
    return vals + s * sigma * np.sqrt(diag[rows] * diag[colidx])


def dense(rowptr, colidx, vals, dtype=np.float64):
    n = len(rowptr) - 1
    A = np.zeros((n, n), dtype=dtype)
    rows = np.repeat(np.arange(n), np.diff(rowptr))
    A[rows, np.asarray(colidx, dtype=np.int64)] = vals
    return A


def max_row_entries(rowptr):
    return int(np.diff(rowptr).max())
