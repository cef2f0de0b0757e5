"""Plain NumPy restatement of the pseudo-ECG formulas, written from the formulas (no device code, no reference code): quadrature geometry of
first-order hexahedra (2×2×2 Gauss) and tetrahedra (4-point rule), the fluxes κ∇φ at the quadrature points, the Plonsey sum and its Σ|terms|,
the diffusion matrix with the project's sign (K[i,j] = −∫ ∇Nᵢ·D∇Nⱼ), a Poisson solve with a grounded dof and lead fields.

Point order: point = cell · n_qp + q; hexahedra: q = i₀ + 2 i₁ + 4 i₂ over ξ = ∓1/√3 per direction; tetrahedra: q = 0 … 3 with ξ_d = a if q == d + 1 else b."""
import numpy as np

HEX_SIGNS = np.array([[-1, -1, -1], [1, -1, -1], [1, 1, -1], [-1, 1, -1], [-1, -1, 1], [1, -1, 1], [1, 1, 1], [-1, 1, 1]], dtype=np.float64)
TET_A, TET_B = 0.5854101966249685, 0.1381966011250105


def reference_element(n_vertices):
    """(ξ (nq, 3), w (nq,), N (nq, nv), dN/dξ (nq, nv, 3))"""
    if n_vertices == 8:
        g = 1.0 / np.sqrt(3.0)
        xi = np.array([[(-g, g)[q & 1], (-g, g)[(q >> 1) & 1], (-g, g)[(q >> 2) & 1]] for q in range(8)])
        f = 1.0 + HEX_SIGNS[None, :, :] * xi[:, None, :]                      # (q, a, d)
        N = 0.125 * f.prod(axis=2)
        dN = np.empty((8, 8, 3))
        for d in range(3):
            o = [k for k in range(3) if k != d]
            dN[:, :, d] = 0.125 * HEX_SIGNS[None, :, d] * f[:, :, o[0]] * f[:, :, o[1]]
        return xi, np.ones(8), N, dN
    assert n_vertices == 4
    xi = np.array([[TET_A if q == d + 1 else TET_B for d in range(3)] for q in range(4)])
    N = np.concatenate([1.0 - xi.sum(axis=1, keepdims=True), xi], axis=1)
    dN = np.broadcast_to(np.array([[-1.0, -1.0, -1.0], [1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0]]), (4, 4, 3)).copy()
    return xi, np.full(4, 1.0 / 24.0), N, dN


def quadrature_geometry(xyz, conn):
    """x̃ (nc, nq, 3), dΩ = detJ·w (nc, nq), ∇N (nc, nq, nv, 3), N (nq, nv)"""
    _, w, N, dN = reference_element(conn.shape[1])
    X = xyz[conn]                                                              # (c, a, i)
    J = np.einsum("cai,qak->cqik", X, dN)                                      # J[i,k] = Σ Xₐᵢ ∂Nₐ/∂ξₖ
    det = np.linalg.det(J)
    grad = np.einsum("qam,cqmk->cqak", dN, np.linalg.inv(J))                   # ∇N = ∂N/∂ξ · J⁻¹
    return np.einsum("qa,cai->cqi", N, X), det * w[None, :], grad, N


def tensor_at_points(D, n_cells, nq):
    D = np.asarray(D, dtype=np.float64)
    if D.ndim == 0:
        D = D * np.eye(3)
    return np.broadcast_to(D, (n_cells, nq, 3, 3)) if D.ndim == 2 else D


def fluxes(xyz, conn, cell_dofs, phi, D):
    """flux[c, q] = Σᵢ (D·∇Nᵢ) φ[dof(c, i)]; D: scalar, (3, 3) or (nc, nq, 3, 3)"""
    _, _, grad, _ = quadrature_geometry(xyz, conn)
    Dq = tensor_at_points(D, conn.shape[0], grad.shape[1])
    return np.einsum("cqrs,cqas,ca->cqr", Dq, grad, phi[cell_dofs])


def plonsey(flux, xq, dO, electrodes, kappa_t=1.0):
    """(φₑ (ne,), Σ|terms| (ne,), both including the factor 1/(4πκₜ))"""
    f, x, w = flux.reshape(-1, 3), xq.reshape(-1, 3), dO.ravel()
    out, mag = [], []
    for e in np.atleast_2d(np.asarray(electrodes, dtype=np.float64)):
        d = x - e
        terms = (f * d).sum(axis=1) / np.linalg.norm(d, axis=1) ** 3 * w
        out.append(-terms.sum() / (4.0 * np.pi * kappa_t))
        mag.append(np.abs(terms).sum() / (4.0 * np.pi * kappa_t))
    return np.array(out), np.array(mag)


def spectral_tensor(fsn_nodal, lam, N, scale=1.0):
    """D at the points from nodal frames (nc, nv, 3 vectors, 3): interpolate, normalise, Gram–Schmidt, Σ λ v⊗v"""
    v = np.einsum("qa,cakd->cqkd", N, fsn_nodal)
    f, s, n = v[:, :, 0], v[:, :, 1], v[:, :, 2]
    f = f / np.linalg.norm(f, axis=2, keepdims=True)
    s = s / np.linalg.norm(s, axis=2, keepdims=True)
    n = n / np.linalg.norm(n, axis=2, keepdims=True)
    s = s - (f * s).sum(axis=2, keepdims=True) * f
    n = n - (f * n).sum(axis=2, keepdims=True) * f - (s * n).sum(axis=2, keepdims=True) * s
    return scale * sum(l * np.einsum("cqi,cqj->cqij", a, a) for l, a in zip(lam, (f, s, n)))


def diffusion_matrix(xyz, conn, cell_dofs, ndofs, D):
    """K[i, j] = −Σ_q ∇Nᵢ·D∇Nⱼ dΩ as a scipy CSR matrix (the sign of the project's diffusion form)"""
    import scipy.sparse as sp
    _, dO, grad, _ = quadrature_geometry(xyz, conn)
    Dq = tensor_at_points(D, conn.shape[0], grad.shape[1])
    Ke = -np.einsum("cqar,cqrs,cqbs,cq->cab", grad, Dq, grad, dO)
    nb = conn.shape[1]
    rows = np.repeat(cell_dofs, nb, axis=1).ravel()
    cols = np.tile(cell_dofs, (1, nb)).ravel()
    return sp.csr_matrix((Ke.ravel(), (rows, cols)), shape=(ndofs, ndofs))


def grounded_solve(K, b, ground):
    """x with K x = b on the free dofs and x[ground] = 0 (rows and columns of the ground dofs eliminated)"""
    import scipy.sparse.linalg as spla
    free = np.setdiff1d(np.arange(K.shape[0]), np.atleast_1d(ground))
    x = np.zeros(K.shape[0])
    x[free] = spla.spsolve(K[free][:, free].tocsc(), b[free])
    return x


def poisson(K, Ki, phi_t, ground):
    """φₑ with K φₑ = −Kᵢ φₘ, grounded"""
    return grounded_solve(K, -(Ki @ phi_t), ground)


def lead_rhs(ndofs, sets):
    """one row per electrode set (dof ids): the first stores −1, each of the other m stores +1/m"""
    r = np.zeros((len(sets), ndofs))
    for i, s in enumerate(sets):
        assert len(s) >= 2
        r[i, s[0]] = -1.0
        for d in s[1:]:
            r[i, d] = 1.0 / (len(s) - 1)
    return r


def lead_fields(K, sets, ground):
    return np.array([grounded_solve(K, r, ground) for r in lead_rhs(K.shape[0], sets)])


def closest_vertex(x, xyz):
    return int(np.argmin(((xyz - np.asarray(x, dtype=np.float64)) ** 2).sum(axis=1)))
