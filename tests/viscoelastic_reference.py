"""NumPy restatement of quasi-static viscoelasticity with the reference's LinearMaxwellMaterial (src/modeling/solid/materials.jl:1816-2008) — the
test reference of tests/test_viscoelastic_*.py.  It shares no code with the package.

Per cell and quadrature point: ε = sym(∇u), the local backward-Euler problem (𝕀/Δt + aℂ) : εᵛ₁ = εᵛ₀/Δt + aℂ : ε solved as the reference solves it —
a dense 6 × 6 system in Mandel notation (tomandel / frommandel, materials.jl:1876-1878) — then σ = E₀ ℂ:ε + E₁ ℂ:(ε − εᵛ₁) and the tangent
(E₀+E₁)ℂ − E₁ ℂ : (𝕀/Δt + aℂ)⁻¹ : aℂ from the same Mandel matrices (:1920-1935).  The package evaluates closed forms on the spherical /
deviatoric split instead, so the two routes check each other.  Element integrals as src/modeling/solid/elements.jl:177-225 with dense Kₑ / rₑ, a dense
global K, and a dense-solve time stepper.

State layout of the package: six values per point, components in the order of SymmetricTensor{2,3}.data (11, 21, 31, 22, 32, 33); arrays here are
[cell][q][6]."""
import numpy as np

COMP = ((0, 0), (1, 0), (2, 0), (1, 1), (2, 1), (2, 2))


def sym_from6(q6):
    T = np.zeros((3, 3))
    for s, (i, j) in enumerate(COMP):
        T[i, j] = T[j, i] = q6[s]
    return T


def sym_to6(T):
    return np.array([T[i, j] for i, j in COMP])


# ---- Mandel notation: an orthonormal basis of the symmetric tensors
def _mandel_basis():
    B = np.zeros((6, 3, 3))
    for k in range(3):
        B[k, k, k] = 1.0
    for k, (i, j) in enumerate(((1, 2), (0, 2), (0, 1))):
        B[3 + k, i, j] = B[3 + k, j, i] = np.sqrt(0.5)
    return B


MB = _mandel_basis()


def tomandel2(T):
    return np.einsum("kij,ij->k", MB, T)


def frommandel2(v):
    return np.einsum("k,kij->ij", v, MB)


def tomandel4(C4):
    return np.einsum("kij,ijmn,lmn->kl", MB, C4, MB)


def frommandel4(M):
    return np.einsum("kl,kij,lmn->ijmn", M, MB, MB)


def stiffness(nu):
    """ℂ = ν/((1+ν)(1−2ν)) I⊗I + 1/(1+ν) 𝕀ˢʸᵐ as a 3×3×3×3 array."""
    I = np.eye(3)
    II = np.einsum("ij,kl->ijkl", I, I)
    Is = 0.5 * (np.einsum("ik,jl->ijkl", I, I) + np.einsum("il,jk->ijkl", I, I))
    return nu / ((1.0 + nu) * (1.0 - 2.0 * nu)) * II + 1.0 / (1.0 + nu) * Is


class Maxwell:
    def __init__(self, E0=70e3, E1=20e3, mu=1e3, eta1=1e3, nu=0.3):
        self.E0, self.E1, self.mu, self.eta1, self.nu = float(E0), float(E1), float(mu), float(eta1), float(nu)
        self.C4 = stiffness(self.nu)
        self.Cm = tomandel4(self.C4)

    def params(self):
        return np.array([self.E0, self.E1, self.mu, self.eta1, self.nu])

    def tau(self):
        return self.eta1 * (1.0 + self.nu) / self.E1

    def local_matrices(self, dt):
        a = self.E1 / self.eta1
        return np.eye(6) / dt + a * self.Cm, a * self.Cm

    def point(self, H, q0, dt):
        """∇u (3×3), accepted viscous strain (6) → (εᵛ₁ (6), σ (3×3), ∂σ/∂ε (3×3×3×3) with the condensation term)."""
        eps = 0.5 * (H + H.T)
        A, B = self.local_matrices(dt)
        ev0 = sym_from6(q0)
        ev1 = frommandel2(np.linalg.solve(A, tomandel2(ev0) / dt + B @ tomandel2(eps)))
        sig = self.E0 * np.einsum("ijkl,kl->ij", self.C4, eps) + self.E1 * np.einsum("ijkl,kl->ij", self.C4, eps - ev1)
        T = frommandel4((self.E0 + self.E1) * self.Cm - self.E1 * self.Cm @ np.linalg.solve(A, B))
        return sym_to6(ev1), sig, T


# ---- reference elements
HEX_V = np.array([(-1, -1, -1), (1, -1, -1), (1, 1, -1), (-1, 1, -1), (-1, -1, 1), (1, -1, 1), (1, 1, 1), (-1, 1, 1)], dtype=float)
HEX_EDGES = ((0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (0, 4), (1, 5), (2, 6), (3, 7))
HEX_FACES = ((0, 3, 2, 1), (0, 1, 5, 4), (1, 2, 6, 5), (2, 3, 7, 6), (0, 4, 7, 3), (4, 5, 6, 7))
TET_EDGES = ((0, 1), (1, 2), (2, 0), (0, 3), (1, 3), (2, 3))


def hex_nodes(order):
    """reference positions of the Lagrange nodes in Ferrite's order: vertices, edge midpoints, face centres, cell centre"""
    if order == 1:
        return HEX_V.copy()
    return np.vstack([HEX_V, [HEX_V[list(e)].mean(0) for e in HEX_EDGES], [HEX_V[list(f)].mean(0) for f in HEX_FACES], [[0.0, 0.0, 0.0]]])


def _lagrange1d(order, node_pos, x):
    """value and derivative at x of the 1-D Lagrange polynomial that is 1 at node_pos (nodes −1, 1 or −1, 0, 1)"""
    nodes = (-1.0, 1.0) if order == 1 else (-1.0, 0.0, 1.0)
    others = [n for n in nodes if n != node_pos]
    den = np.prod([node_pos - n for n in others])
    val = np.prod([x - n for n in others]) / den
    der = sum(np.prod([x - m for m in others if m != n]) for n in others) / den
    return val, der


def hex_shape(order, xi):
    P = hex_nodes(order)
    N, dN = np.zeros(len(P)), np.zeros((len(P), 3))
    for a, p in enumerate(P):
        vd = [_lagrange1d(order, p[d], xi[d]) for d in range(3)]
        N[a] = vd[0][0] * vd[1][0] * vd[2][0]
        for d in range(3):
            dN[a, d] = np.prod([vd[e][1] if e == d else vd[e][0] for e in range(3)])
    return N, dN


def hex_rule(n):
    x, w = np.polynomial.legendre.leggauss(n)
    pts = [((x[i], x[j], x[k]), w[i] * w[j] * w[k]) for k in range(n) for j in range(n) for i in range(n)]   # first coordinate fastest
    return np.array([p for p, _ in pts]), np.array([wt for _, wt in pts])


def tet_rule(order):
    """(barycentric points, weights summing to 1/6): order 1 → the 4-point degree-2 rule, order 2 → Keast's 8 points"""
    if order == 1:
        a = (5.0 - np.sqrt(5.0)) / 20.0
        return np.full((4, 4), a) + (1.0 - 4.0 * a) * np.eye(4), np.full(4, 1.0 / 24.0)
    out, w = [], []
    for a, wt in ((0.328054696711427, 0.138527966511862), (0.106952273932930, 0.111472033488138)):
        out.append(np.full((4, 4), a) + (1.0 - 4.0 * a) * np.eye(4))
        w += [wt / 6.0] * 4
    return np.vstack(out), np.array(w)


def tet_shape_gradients(order, lam):
    """dN/dλ (nb, 4)"""
    if order == 1:
        return np.eye(4)
    dN = np.zeros((10, 4))
    for v in range(4):
        dN[v, v] = 4.0 * lam[v] - 1.0
    for e, (i, j) in enumerate(TET_EDGES):
        dN[4 + e, i] = 4.0 * lam[j]
        dN[4 + e, j] = 4.0 * lam[i]
    return dN


def n_points(family, order):
    return (8 if order == 1 else 27) if family == "hex" else (4 if order == 1 else 8)


def point_gradients(family, order, X):
    """mapped gradients ∇Nₐ (nb, 3) and dΩ at every quadrature point of the cell with vertex coordinates X"""
    out = []
    if family == "hex":
        pts, w = hex_rule(2 if order == 1 else 3)
        for xi, wq in zip(pts, w):
            _, dM = hex_shape(1, xi)
            J = X.T @ dM                                   # J[i][k] = Σ_a x_a[i] ∂M_a/∂ξ_k
            _, dN = hex_shape(order, xi)
            out.append((dN @ np.linalg.inv(J), np.linalg.det(J) * wq))
    else:
        lamq, w = tet_rule(order)
        Mi = np.linalg.inv(np.vstack([np.ones(4), X.T]))   # λ solves [1; x] = M λ
        dl = Mi[:, 1:]
        det = np.linalg.det(np.array([X[1] - X[0], X[2] - X[0], X[3] - X[0]]).T)
        for lam, wq in zip(lamq, w):
            out.append((tet_shape_gradients(order, lam) @ dl, det * wq))
    return out


def element(mat, family, order, X, ue, Q0, dt):
    """(Kₑ, rₑ, Q₁ (nq, 6)) of one cell; dof i = 3a + c ↔ ∇δuᵢ = e_c ⊗ ∇Nₐ"""
    U = ue.reshape(-1, 3)
    nd = U.size
    Ke, re, Q1 = np.zeros((nd, nd)), np.zeros(nd), np.zeros_like(Q0)
    for q, (G, dO) in enumerate(point_gradients(family, order, X)):
        H = U.T @ G
        Q1[q], sig, T = mat.point(H, Q0[q], dt)
        re += np.einsum("ak,ck->ac", G, sig).ravel() * dO
        Ke += np.einsum("ak,ckdl,bl->acbd", G, T, G).reshape(nd, nd) * dO
    return Ke, re, Q1


def assemble(mat, family, order, xyz, conn, cell_dofs, u, Qknown, dt, cells=None):
    """dense K (ndofs × ndofs), r, Q₁ [cell][q][6] (cells outside `cells` keep Qknown's values)"""
    n = len(u)
    K, r, Q1 = np.zeros((n, n)), np.zeros(n), Qknown.copy()
    for c in (range(len(conn)) if cells is None else cells):
        d = cell_dofs[c]
        Ke, re, Q1[c] = element(mat, family, order, xyz[conn[c]], u[d], Qknown[c], dt)
        r[d] += re
        K[np.ix_(d, d)] += Ke
    return K, r, Q1


def csr_values(K, rowptr, colidx):
    rows = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    return K[rows, colidx]


def step(mat, family, order, xyz, conn, cell_dofs, u, Qknown, dt, prescribed, solve=np.linalg.solve):
    """One backward-Euler step of the quasi-static problem: `u` satisfies the Dirichlet values on `prescribed`; one Newton iteration (the problem
    is linear in u), then the state at the new displacement.  Returns (u₁, Q₁)."""
    free = np.setdiff1d(np.arange(len(u)), prescribed)
    K, r, _ = assemble(mat, family, order, xyz, conn, cell_dofs, u, Qknown, dt)
    u1 = u.copy()
    u1[free] -= solve(K[np.ix_(free, free)], r[free])
    _, r1, Q1 = assemble(mat, family, order, xyz, conn, cell_dofs, u1, Qknown, dt)
    return u1, Q1, np.abs(r1[free]).max()


def creep_recurrence(mat, eps11, dt, nsteps):
    """the local problem alone at fixed uniaxial strain ε₁₁: the history of εᵛ (nsteps + 1, 6)"""
    H = np.zeros((3, 3))
    H[0, 0] = eps11
    Q = np.zeros((nsteps + 1, 6))
    for k in range(nsteps):
        Q[k + 1] = mat.point(H, Q[k], dt)[0]
    return Q
