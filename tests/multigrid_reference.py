"""numpy-only restatement of the geometric multigrid (tb_multigrid.hip, tb_mg_planners.cpp) for the tests: dense P from the parent lists of a
GridHierarchy, dense PᵀAP, and the same V(degree, degree) cycle — Chebyshev–Jacobi smoother on [λmax/ratio, λmax], exact coarsest solve — with
the λmax per level handed in (the tests pass what the device reports, so the comparison is of the arithmetic, not of the eigenvalue estimate)."""
import numpy as np


def node_dofs(dh):
    """(n_nodes, ncomp): dof of every (node, component) of a first-order field"""
    nc = dh.ip.ncomp
    out = np.full((dh.grid.n_nodes, nc), -1, dtype=np.int64)
    for c in range(nc):
        out[dh.grid.conn.ravel(), c] = dh.cell_dofs[:, c::nc].ravel()
    assert (out >= 0).all()
    return out


def nodal_P(parents, n_coarse_nodes):
    """(n_fine_nodes, n_coarse_nodes): weight 1/#parents at every parent"""
    pptr, pidx = parents
    n = len(pptr) - 1
    P = np.zeros((n, n_coarse_nodes))
    for v in range(n):
        ps = pidx[pptr[v]:pptr[v + 1]]
        P[v, ps] = 1.0 / len(ps)
    return P


def dense_P(parents, dh_fine, dh_coarse, prescribed_fine=None):
    """P (fine dofs × coarse dofs) and the flags of the prescribed coarse dofs: a coarse dof is prescribed iff the fine dof it coincides with is;
    rows of prescribed fine dofs and columns of prescribed coarse dofs are zero"""
    nf, ncs = node_dofs(dh_fine), node_dofs(dh_coarse)
    Pn = nodal_P(parents, dh_coarse.grid.n_nodes)
    P = np.zeros((dh_fine.ndofs, dh_coarse.ndofs))
    for c in range(dh_fine.ip.ncomp):
        P[np.ix_(nf[:, c], ncs[:, c])] = Pn
    cpre = np.zeros(dh_coarse.ndofs, dtype=bool)
    if prescribed_fine is not None:
        pf = np.asarray(prescribed_fine, dtype=bool)
        cpre[ncs.ravel()] = pf[nf[:dh_coarse.grid.n_nodes].ravel()]
        P[pf, :] = 0.0
        P[:, cpre] = 0.0
    return P, cpre


def csr_to_dense(sp, nz):
    n = len(sp.rowptr) - 1
    A = np.zeros((n, n))
    rows = np.repeat(np.arange(n), np.diff(sp.rowptr))
    A[rows, sp.colidx] = nz
    return A


def dense_to_csr(sp, A):
    rows = np.repeat(np.arange(len(sp.rowptr) - 1), np.diff(sp.rowptr))
    return A[rows, sp.colidx]


def galerkin(P, A, coarse_prescribed):
    """PᵀAP; the diagonal of a prescribed coarse dof (row and column are empty) is the mean |diagonal| of the free ones"""
    Ac = P.T @ A @ P
    if coarse_prescribed.any():
        d = np.abs(np.diag(Ac))[~coarse_prescribed]
        Ac[coarse_prescribed, coarse_prescribed] = d.mean() if len(d) else 1.0
    return Ac


def chebyshev(A, dinv, lmax, ratio, degree, r, x=None):
    """`degree` steps of the Chebyshev iteration on D⁻¹A for A x = r (Saad, Alg. 12.1), from x (None: zero)"""
    lmin = lmax / ratio
    theta, delta = 0.5 * (lmax + lmin), 0.5 * (lmax - lmin)
    sigma1 = theta / delta
    rho = 1.0 / sigma1
    x = np.zeros_like(r) if x is None else x.copy()
    d = dinv * (r - A @ x) / theta
    x += d
    for _ in range(1, degree):
        rho_new = 1.0 / (2.0 * sigma1 - rho)
        d = rho_new * rho * d + 2.0 * rho_new / delta * dinv * (r - A @ x)
        x += d
        rho = rho_new
    return x


def vcycle(As, Ps, prescribed, lmax, degree, ratio, r, level=None):
    """x = M⁻¹ r.  As[l]: dense level operators, coarsest first; Ps[l]: P from level l − 1 to l (Ps[0] unused); prescribed[l]: flags; lmax[l]"""
    l = len(As) - 1 if level is None else level
    if l == 0:
        return np.linalg.solve(As[0], r)
    dinv = np.where(prescribed[l], 0.0, 1.0 / np.diag(As[l]))
    x = chebyshev(As[l], dinv, lmax[l], ratio, degree, r)
    rc = Ps[l].T @ (r - As[l] @ x)
    x = x + Ps[l] @ vcycle(As, Ps, prescribed, lmax, degree, ratio, rc, l - 1)
    return chebyshev(As[l], dinv, lmax[l], ratio, degree, r, x)


def hierarchy(gh, dhs, A_fine, prescribed_fine=None):
    """dense level operators, transfers and flags of a grid hierarchy with per-level handlers `dhs` (coarsest first) → (As, Ps, prescribed)"""
    nl = len(dhs)
    As, Ps, pres = [None] * nl, [None] * nl, [None] * nl
    As[-1] = A_fine
    pres[-1] = np.zeros(dhs[-1].ndofs, dtype=bool) if prescribed_fine is None else np.asarray(prescribed_fine, dtype=bool)
    for l in range(nl - 1, 0, -1):
        Ps[l], pres[l - 1] = dense_P(gh.parents[l - 1], dhs[l], dhs[l - 1], pres[l] if pres[l].any() else None)
        As[l - 1] = galerkin(Ps[l], As[l], pres[l - 1])
    return As, Ps, pres
