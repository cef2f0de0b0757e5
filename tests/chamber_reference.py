"""NumPy restatement of the 3D-0D chamber facet integrals (test infrastructure): a direct per-facet, per-point loop over
Pressure3D0DVolumeCouplerIntegrator (src/modeling/coupler/fsi.jl:118-185) and the volume integrands (fsi.jl:53-58, src/modeling/rsafdq2022.jl:22-85).
∂V/∂d and ∂V/∂F come from complex-step differentiation of volume_integral, so nothing here shares the hand derivation of the device kernel; the
facet normal and dΓ come from Nanson's formula on the reference normal, not from the kernel's tangent-vector cross product."""
import numpy as np

HEX_SGN = np.array([[-1, -1, -1], [1, -1, -1], [1, 1, -1], [-1, 1, -1], [-1, -1, 1], [1, -1, 1], [1, 1, 1], [-1, 1, 1]], dtype=float)
# Ferrite Lagrange{RefHexahedron, 2}: vertices, edges, faces, volume → index of the 1D basis (0: ξ = −1, 1: ξ = 0, 2: ξ = +1) per direction
HEX27_TIX = np.array([[0, 0, 0], [2, 0, 0], [2, 2, 0], [0, 2, 0], [0, 0, 2], [2, 0, 2], [2, 2, 2], [0, 2, 2], [1, 0, 0], [2, 1, 0], [1, 2, 0], [0, 1, 0],
                      [1, 0, 2], [2, 1, 2], [1, 2, 2], [0, 1, 2], [0, 0, 1], [2, 0, 1], [2, 2, 1], [0, 2, 1], [1, 1, 0], [1, 0, 1], [2, 1, 1], [1, 2, 1],
                      [0, 1, 1], [1, 1, 2], [1, 1, 1]])
# Ferrite.reference_facets(RefHexahedron): (fixed axis, value) of local facets 0…5 — the outward reference normal is value · e_axis
FACET_AXIS = [(2, -1.0), (1, -1.0), (0, 1.0), (1, 1.0), (0, -1.0), (2, 1.0)]
# in-facet directions (s, t) in the order the facet rule enumerates its points: q = i_s + nq · i_t
FACET_ST = [(1, 0), (0, 2), (1, 2), (2, 0), (2, 1), (0, 1)]


def gauss(n):
    return np.polynomial.legendre.leggauss(n)


def shape_q1(xi):
    f = 1.0 + HEX_SGN * xi
    N = 0.125 * f.prod(axis=1)
    dN = np.stack([0.125 * HEX_SGN[:, 0] * f[:, 1] * f[:, 2], 0.125 * f[:, 0] * HEX_SGN[:, 1] * f[:, 2], 0.125 * f[:, 0] * f[:, 1] * HEX_SGN[:, 2]], axis=1)
    return N, dN


def shape_q2(xi):
    v = np.array([[0.5 * x * (x - 1.0), 1.0 - x * x, 0.5 * x * (x + 1.0)] for x in xi])      # [direction][1D basis]
    d = np.array([[x - 0.5, -2.0 * x, x + 0.5] for x in xi])
    t = HEX27_TIX
    N = v[0, t[:, 0]] * v[1, t[:, 1]] * v[2, t[:, 2]]
    dN = np.stack([d[0, t[:, 0]] * v[1, t[:, 1]] * v[2, t[:, 2]], v[0, t[:, 0]] * d[1, t[:, 1]] * v[2, t[:, 2]], v[0, t[:, 0]] * v[1, t[:, 1]] * d[2, t[:, 2]]], axis=1)
    return N, dN


class RSAFDQ2022:
    def __init__(self, h=(0.0, 1.0, 0.0), b=(0.0, 0.0, -0.1)):
        self.h, self.b = np.asarray(h, float), np.asarray(b, float)

    def volume_integral(self, x, d, F, N):                   # rsafdq2022.jl:80-85
        return -(np.linalg.det(F) * (np.outer(self.h, self.h) @ (x + d - self.b)) @ (np.linalg.inv(F).T @ N))


class Hirschvogel2017:
    def volume_integral(self, x, d, F, N):                   # fsi.jl:55-58
        return -(np.linalg.det(F) * (x + d) @ np.linalg.inv(F).T @ N)


def facet_points(X, lf, nq):
    """(ξ, dΓ, n₀) of the nq × nq Gauss points of local facet lf of the trilinear cell with vertex coordinates X (8 × 3)"""
    gx, gw = gauss(nq)
    axis, val = FACET_AXIS[lf]
    s, t = FACET_ST[lf]
    out = []
    for it in range(nq):
        for is_ in range(nq):
            xi = np.zeros(3)
            xi[axis], xi[s], xi[t] = val, gx[is_], gx[it]
            _, dM = shape_q1(xi)
            J = X.T @ dM
            nref = np.zeros(3); nref[axis] = val
            nw = np.linalg.det(J) * np.linalg.inv(J).T @ nref      # Nanson: n dΓ = det J J⁻ᵀ n_ref dΓ_ref
            out.append((xi, np.linalg.norm(nw) * gw[is_] * gw[it], nw / np.linalg.norm(nw), J))
    return out


def assemble(xyz, conn, cell_dofs, order, facets, nq, u, p, method, cstep=1e-30):
    """→ dict(volume, col, row, r, Ke): the sums of fsi.jl:118-185 over `facets` ((cell, local facet) pairs, 0-based); Ke: list of (dofs, Kdd)
    element tangents, one per facet.  nq = 0 selects the interpolation order, like the device form."""
    nq = nq or order
    shape = shape_q1 if order == 1 else shape_q2
    n = u.size
    out = dict(volume=0.0, col=np.zeros(n), row=np.zeros(n), r=np.zeros(n), Ke=[])
    I = np.eye(3)
    for cell, lf in np.asarray(facets).reshape(-1, 2):
        X = xyz[conn[cell]]
        dofs = np.asarray(cell_dofs[cell]).reshape(-1)
        ue = u[dofs].reshape(-1, 3)
        nd = dofs.size
        Kdd = np.zeros((nd, nd))
        for xi, dG, n0, Jg in facet_points(X, lf, nq):
            M, _ = shape_q1(xi)
            N, dNref = shape(xi)
            G = dNref @ np.linalg.inv(Jg)                     # mapped gradients
            x = M @ X
            d = N @ ue
            F = I + ue.T @ G
            Jf = np.linalg.det(F)
            invF = np.linalg.inv(F)
            cofF = invF.T
            nn = cofF @ n0
            nb = N.size
            # fsi.jl:150-165 for all (i, j) at once; the expressions are the reference's: δcofF = −(F⁻¹ ∇δuⱼ F⁻¹)ᵀ, δJ = J tr(∇δuⱼ F⁻¹)
            gradj = np.einsum("ek,bl->bekl", I, G)                                   # ∇δuⱼ = e_e ⊗ ∇N_b, j = (b, e)
            dcof = -np.einsum("km,bemn,nl->belk", invF, gradj, invF)
            dJ = Jf * np.einsum("bekl,lk->be", gradj, invF)
            dJcofn = np.einsum("be,k->bek", dJ, cofF @ n0) + Jf * np.einsum("bekl,l->bek", dcof, n0)   # (δJ cofF + J δcofF) n₀
            Kq = p * np.einsum("a,bec->acbe", N, dJcofn) * dG                        # · δuᵢ, i = (a, c)
            Kdd += Kq.reshape(3 * nb, 3 * nb)
            ci = np.outer(N, Jf * nn).reshape(-1) * dG                               # J n · δuᵢ dΓ
            np.add.at(out["col"], dofs, ci)
            np.add.at(out["r"], dofs, p * ci)
            out["volume"] += method.volume_integral(x, d, F, n0) * dG
            dVdu = np.array([np.imag(method.volume_integral(x, d + 1j * cstep * I[k], F, n0)) / cstep for k in range(3)])
            dVdF = np.array([[np.imag(method.volume_integral(x, d, F + 1j * cstep * np.outer(I[k], I[l]), n0)) / cstep for l in range(3)] for k in range(3)])
            for b in range(N.size):
                for e in range(3):
                    out["row"][dofs[3 * b + e]] += (dVdu @ (N[b] * I[e]) + np.sum(dVdF * np.outer(I[e], G[b]))) * dG
        out["Ke"].append((dofs, Kdd))
    return out


def scatter_csr(Ke, rowptr, colidx):
    nz = np.zeros(len(colidx))
    for dofs, K in Ke:
        for i, di in enumerate(dofs):
            cols = colidx[rowptr[di]:rowptr[di + 1]]
            pos = {int(c): k for k, c in enumerate(cols)}
            for j, dj in enumerate(dofs):
                nz[rowptr[di] + pos[int(dj)]] += K[i, j]
    return nz


def box_mesh(a, b, c, nel=(1, 1, 1)):
    """structured box [0,a]×[0,b]×[0,c] of trilinear hexahedra and its boundary facets with outward normals: (xyz, conn, facets)"""
    nx, ny, nz = nel
    xs, ys, zs = np.linspace(0, a, nx + 1), np.linspace(0, b, ny + 1), np.linspace(0, c, nz + 1)
    xyz = np.array([[x, y, z] for z in zs for y in ys for x in xs])
    nid = lambda i, j, k: i + (nx + 1) * (j + (ny + 1) * k)
    conn, facets = [], []
    for k in range(nz):
        for j in range(ny):
            for i in range(nx):
                cidx = len(conn)
                conn.append([nid(i, j, k), nid(i + 1, j, k), nid(i + 1, j + 1, k), nid(i, j + 1, k), nid(i, j, k + 1), nid(i + 1, j, k + 1), nid(i + 1, j + 1, k + 1),
                             nid(i, j + 1, k + 1)])
                for lf, on in enumerate([k == 0, j == 0, i == nx - 1, j == ny - 1, i == 0, k == nz - 1]):
                    if on:
                        facets.append((cidx, lf))
    return xyz, np.array(conn, dtype=np.int32), np.array(facets, dtype=np.int32)
