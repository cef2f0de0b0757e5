"""NumPy reference of the Newmark elastodynamics arithmetic (test infrastructure of tests/test_newmark_*.py; no device, no library).

Written independently of the device code: the element mass Mₑ[(i,c),(j,d)] = ρ NᵢNⱼ δ_cd dΩ by quadrature for the four field kinds (trilinear / triquadratic
hexahedra on trilinear geometry, P1 / P2 tetrahedra on affine geometry) scattered through the caller's dof table, the predictor and corrector of
src/solver/time/newmark.jl:580-581, 91-95, 171-180 and the Hermite weights of newmark.jl:369-379."""
import itertools

import numpy as np

HEX8_SIGNS = np.array([(-1, -1, -1), (1, -1, -1), (1, 1, -1), (-1, 1, -1), (-1, -1, 1), (1, -1, 1), (1, 1, 1), (-1, 1, 1)], dtype=float)
HEX27_TIX = np.array([(0, 0, 0), (2, 0, 0), (2, 2, 0), (0, 2, 0), (0, 0, 2), (2, 0, 2), (2, 2, 2), (0, 2, 2), (1, 0, 0), (2, 1, 0), (1, 2, 0), (0, 1, 0), (1, 0, 2),
                      (2, 1, 2), (1, 2, 2), (0, 1, 2), (0, 0, 1), (2, 0, 1), (2, 2, 1), (0, 2, 1), (1, 1, 0), (1, 0, 1), (2, 1, 1), (1, 2, 1), (0, 1, 1), (1, 1, 2), (1, 1, 1)])
TET_EDGES = ((0, 1), (1, 2), (2, 0), (0, 3), (1, 3), (2, 3))


def gauss(n):
    x, w = np.polynomial.legendre.leggauss(n)
    return x, w


def hex_rule(n):
    """tensor Gauss rule on [−1, 1]³, first coordinate fastest: (points (n³, 3), weights)"""
    x, w = gauss(n)
    pts = np.array([(x[i], x[j], x[k]) for k in range(n) for j in range(n) for i in range(n)])
    wts = np.array([w[i] * w[j] * w[k] for k in range(n) for j in range(n) for i in range(n)])
    return pts, wts


def tet_mass_rule(order):
    """(barycentric points, weights summing to 1/6) exact for degree 2·order: the 4-point degree-2 rule; Keast's 11-point degree-4 rule (Keast 1986)"""
    if order == 1:
        a = (5.0 - np.sqrt(5.0)) / 20.0
        return np.full((4, 4), a) + (1.0 - 4.0 * a) * np.eye(4), np.full(4, 1.0 / 24.0)
    pts, w = [(0.25, 0.25, 0.25, 0.25)], [-74.0 / 5625.0]
    a = 1.0 / 14.0
    for v in range(4):
        pts.append(tuple(1.0 - 3.0 * a if k == v else a for k in range(4)))
        w.append(343.0 / 45000.0)
    s = np.sqrt(5.0 / 14.0)
    b, c = 0.25 * (1.0 + s), 0.25 * (1.0 - s)
    for i, j in itertools.combinations(range(4), 2):
        pts.append(tuple(b if k in (i, j) else c for k in range(4)))
        w.append(56.0 / 2250.0)
    return np.array(pts), np.array(w)


def hex8_shape(xi):
    return 0.125 * np.prod(1.0 + HEX8_SIGNS * np.asarray(xi)[None, :], axis=1)


def hex8_dshape(xi):
    f = 1.0 + HEX8_SIGNS * np.asarray(xi)[None, :]
    d = np.empty((8, 3))
    for k in range(3):
        g = f.copy()
        g[:, k] = HEX8_SIGNS[:, k]
        d[:, k] = 0.125 * np.prod(g, axis=1)
    return d


def _q1d(i, x):
    return (0.5 * x * (x - 1.0), 1.0 - x * x, 0.5 * x * (x + 1.0))[i]


def hex27_shape(xi):
    return np.array([_q1d(t[0], xi[0]) * _q1d(t[1], xi[1]) * _q1d(t[2], xi[2]) for t in HEX27_TIX])


def tet_shape(order, lam):
    lam = np.asarray(lam, dtype=float)
    if order == 1:
        return lam.copy()
    return np.concatenate([lam * (2.0 * lam - 1.0), [4.0 * lam[i] * lam[j] for i, j in TET_EDGES]])


def element_scalar_mass(kind, X, rho, qorder=0):
    """Σ_q ρ(ξ_q) NᵢNⱼ detJ w_q of one cell.  kind: "hex8" | "hex27" | "tet4" | "tet10"; X: vertex coordinates (8 or 4, 3); rho: a number or the first-order
    nodal densities of the cell (8 or 4).  qorder: Gauss points per direction on hexahedra, 0 → max(2p − 1, 2)."""
    nodal = np.ndim(rho) > 0
    if kind in ("hex8", "hex27"):
        p = 1 if kind == "hex8" else 2
        pts, wts = hex_rule(qorder or max(2 * p - 1, 2))
        nb = 8 if p == 1 else 27
        Me = np.zeros((nb, nb))
        for xi, w in zip(pts, wts):
            Mg = hex8_shape(xi)
            J = X.T @ hex8_dshape(xi)
            N = Mg if p == 1 else hex27_shape(xi)
            r = float(Mg @ rho) if nodal else float(rho)
            Me += r * np.linalg.det(J) * w * np.outer(N, N)
        return Me
    p = 1 if kind == "tet4" else 2
    pts, wts = tet_mass_rule(p)
    det = np.linalg.det(np.array([X[1] - X[0], X[2] - X[0], X[3] - X[0]]).T)
    nb = 4 if p == 1 else 10
    Me = np.zeros((nb, nb))
    for lam, w in zip(pts, wts):
        N = tet_shape(p, lam)
        r = float(lam @ rho) if nodal else float(rho)
        Me += r * det * w * np.outer(N, N)
    return Me


def csr_positions(rowptr, colidx, rows, cols):
    """nz index of every (row, col) pair (columns sorted within a row)"""
    out = np.empty(len(rows), dtype=np.int64)
    for k, (r, c) in enumerate(zip(rows, cols)):
        lo, hi = rowptr[r], rowptr[r + 1]
        pos = lo + np.searchsorted(colidx[lo:hi], c)
        assert pos < hi and colidx[pos] == c, (r, c)
        out[k] = pos
    return out


def assemble_vector_mass(kind, xyz, conn, cell_dofs, rowptr, colidx, rho, qorder=0):
    """CSR values of the mass of the 3-component field: per cell the scalar element mass at the three same-component positions of every node pair,
    through the dof table as given (local dof = 3·node + component).  rho: a number or nodal densities (n_cells, 8 | 4)."""
    nz = np.zeros(int(rowptr[-1]))
    nodal = np.ndim(rho) > 0
    for cell in range(len(conn)):
        Me = element_scalar_mass(kind, xyz[conn[cell]], rho[cell] if nodal else rho, qorder)
        nb = Me.shape[0]
        d = cell_dofs[cell]
        for c in range(3):
            rows = np.repeat(d[c::3], nb)
            cols = np.tile(d[c::3], nb)
            np.add.at(nz, csr_positions(rowptr, colidx, rows, cols), Me.ravel())
    return nz


def same_component_mask(cell_dofs, rowptr, colidx):
    """True at the nz positions that couple two dofs of the same component in some cell (everything else must stay exactly 0.0)"""
    mask = np.zeros(int(rowptr[-1]), dtype=bool)
    nb = cell_dofs.shape[1] // 3
    for d in cell_dofs:
        for c in range(3):
            mask[csr_positions(rowptr, colidx, np.repeat(d[c::3], nb), np.tile(d[c::3], nb))] = True
    return mask


def csr_matvec(rowptr, colidx, nz, v):
    out = np.zeros(len(rowptr) - 1)
    np.add.at(out, np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr)), nz * v[colidx])
    return out


# ----------------------------------------------------------------------------------------------- the scheme
def predict(u, v, a, dt, beta, gamma):
    """ũ = uₙ + Δt vₙ + (½ − β)Δt² aₙ,  ṽ = vₙ + (1 − γ)Δt aₙ"""
    return u + dt * v + (0.5 - beta) * dt * dt * a, v + (1.0 - gamma) * dt * a


def correct(u, utilde, vtilde, dt, beta, gamma):
    """aₙ₊₁ = (u − ũ)/(βΔt²),  vₙ₊₁ = ṽ + γΔt aₙ₊₁"""
    a = (u - utilde) / (beta * dt * dt)
    return a, vtilde + gamma * dt * a


def hermite_weights(theta, dt, D):
    """weights of (uprev, vprev, u, v) in the D-th time derivative of the cubic Hermite interpolant at θ = (t − tprev)/Δt"""
    th, th2, th3 = theta, theta * theta, theta ** 3
    if D == 0:
        return (2 * th3 - 3 * th2 + 1, dt * (th3 - 2 * th2 + th), -2 * th3 + 3 * th2, dt * (th3 - th2))
    if D == 1:
        return ((6 * th2 - 6 * th) / dt, 3 * th2 - 4 * th + 1, (-6 * th2 + 6 * th) / dt, 3 * th2 - 2 * th)
    if D == 2:
        return ((12 * th - 6) / dt ** 2, (6 * th - 4) / dt, (-12 * th + 6) / dt ** 2, (6 * th - 2) / dt)
    raise ValueError(D)


def hermite(theta, dt, D, u0, v0, u1, v1):
    c = hermite_weights(theta, dt, D)
    return c[0] * u0 + c[1] * v0 + c[2] * u1 + c[3] * v1
