"""NumPy reference of the quasi-static mechanics integrals on P1 / P2 tetrahedra (test infrastructure of tests/test_tet_mechanics_*.py).

Written independently of the device code: shape functions, barycentric gradients (from the inverse of the 4 × 4 vertex matrix, not from a
Jacobian), the quadrature tables and the loops of src/modeling/solid/elements.jl:177-225 and src/modeling/core/weak_boundary_conditions.jl are
restated here; the material (Ψ, P, 𝔸) comes from the oracle's point routine `oracle.energy` (orc_energy)."""
import numpy as np

TET_EDGES = ((0, 1), (1, 2), (2, 0), (0, 3), (1, 3), (2, 3))
TET_FACETS = ((0, 2, 1), (0, 1, 3), (1, 2, 3), (0, 3, 2))


def tet_rule(degree):
    """(barycentric points (nq, 4), weights summing to the reference volume 1/6)."""
    if degree == 2:
        a = (5.0 - np.sqrt(5.0)) / 20.0
        lam = np.full((4, 4), a) + (1.0 - 4.0 * a) * np.eye(4)
        return lam, np.full(4, 1.0 / 24.0)
    if degree == 3:  # Keast (1986), 8 points, positive weights
        out, w = [], []
        for a, wt in ((0.328054696711427, 0.138527966511862), (0.106952273932930, 0.111472033488138)):
            out.append(np.full((4, 4), a) + (1.0 - 4.0 * a) * np.eye(4))
            w += [wt / 6.0] * 4
        return np.vstack(out), np.array(w)
    raise ValueError(degree)


def tri_rule(degree):
    """(barycentric points (nq, 3), weights summing to 1: fractions of the facet area)."""
    if degree == 2:
        return np.full((3, 3), 1.0 / 6.0) + 0.5 * np.eye(3), np.full(3, 1.0 / 3.0)
    if degree == 4:  # Dunavant (1985), 6 points
        out, w = [], []
        for a, wt in ((0.445948490915965, 0.223381589678011), (0.091576213509771, 0.109951743655322)):
            out.append(np.full((3, 3), a) + (1.0 - 3.0 * a) * np.eye(3))
            w += [wt] * 3
        return np.vstack(out), np.array(w)
    raise ValueError(degree)


def shape(order, lam):
    """N (nb,), dN/dλ (nb, 4) of the Lagrange basis of the given order at barycentric point lam."""
    lam = np.asarray(lam, dtype=float)
    if order == 1:
        return lam.copy(), np.eye(4)
    N, dN = np.zeros(10), np.zeros((10, 4))
    for v in range(4):
        N[v] = lam[v] * (2.0 * lam[v] - 1.0)
        dN[v, v] = 4.0 * lam[v] - 1.0
    for e, (i, j) in enumerate(TET_EDGES):
        N[4 + e] = 4.0 * lam[i] * lam[j]
        dN[4 + e, i] = 4.0 * lam[j]
        dN[4 + e, j] = 4.0 * lam[i]
    return N, dN


def barycentric_gradients(X):
    """∇λ_v (4, 3) and the signed volume·6 of the tetrahedron with vertex coordinates X (4, 3)."""
    M = np.vstack([np.ones(4), X.T])            # λ solves M λ = (1, x)
    Mi = np.linalg.inv(M)
    det = np.linalg.det(np.array([X[1] - X[0], X[2] - X[0], X[3] - X[0]]).T)
    return Mi[:, 1:], det


class Material:
    """energy / penalty ids and parameters of oracle.energy; frame (3, 3) rows f, s, n or nodal frames (n_cells, 4, 3, 3); active tension
    (scalar) times optional nodal state (n_cells, 4)."""

    def __init__(self, energy, penalty, p, up, fsn=np.eye(3), fsn_field=None, tension=0.0, act_field=None):
        self.energy, self.penalty, self.p, self.up = energy, penalty, list(p), list(up)
        self.fsn, self.fsn_field, self.tension, self.act_field = np.asarray(fsn, dtype=float), fsn_field, float(tension), act_field


def _point_material(oracle, mat, cell, lam, F):
    fsn = mat.fsn
    if mat.fsn_field is not None:
        fr = np.einsum("a,aij->ij", lam, mat.fsn_field[cell])
        fsn = np.array(oracle.orthogonalize(fr[0], fr[1], fr[2]))
    ta = mat.tension
    if mat.act_field is not None:
        ta *= float(lam @ mat.act_field[cell])
    oracle.set_point_activation(ta)
    try:
        _, P, A = oracle.energy(mat.energy, mat.penalty, mat.p, mat.up, F, fsn)
    finally:
        oracle.set_point_activation(0.0)
    return P, A


def element(oracle, order, X, ue, mat, cell, want_K=True):
    """(Kₑ, rₑ) of one cell, elements.jl:177-225: dof i = 3a + c ↔ ∇δuᵢ = e_c ⊗ ∇Nₐ."""
    nb = 4 if order == 1 else 10
    lamq, wq = tet_rule(2 if order == 1 else 3)
    dl, det = barycentric_gradients(X)
    U = ue.reshape(nb, 3)
    Ke, re = np.zeros((3 * nb, 3 * nb)), np.zeros(3 * nb)
    for lam, w in zip(lamq, wq):
        _, dN = shape(order, lam)
        G = dN @ dl                                  # (nb, 3) mapped gradients
        F = np.eye(3) + U.T @ G
        P, A = _point_material(oracle, mat, cell, lam, F)
        dO = w * det
        re += np.einsum("ak,ck->ac", G, P).ravel() * dO
        if want_K:
            A4 = A.reshape(3, 3, 3, 3)               # [c][k][d][l]
            Ke += np.einsum("ak,ckdl,bl->acbd", G, A4, G).reshape(3 * nb, 3 * nb) * dO
    return Ke, re


def assemble(oracle, order, xyz, conn, cell_dofs, u, mat, rowptr=None, colidx=None, cells=None):
    """(nz or None, r): scatter of the element contributions into CSR (sorted columns) and the residual vector."""
    want_K = rowptr is not None
    nz = np.zeros(int(rowptr[-1])) if want_K else None
    r = np.zeros(len(u))
    kmax = 0.0
    for c in (range(len(conn)) if cells is None else cells):
        d = cell_dofs[c]
        Ke, re = element(oracle, order, xyz[conn[c]], u[d], mat, c, want_K)
        r[d] += re
        if want_K:
            kmax = max(kmax, np.abs(Ke).max())
            for i, di in enumerate(d):
                lo, hi = rowptr[di], rowptr[di + 1]
                nz[lo + np.searchsorted(colidx[lo:hi], d)] += Ke[i]
    assemble.kmax = kmax
    return nz, r


def facet_element(order, X, lf, ue, bc, param, pnodal=None, want_K=True):
    """(Kₑ, rₑ) of one (cell, local facet): bc 'robin' Ψ = α u·u, 'spring' Ψ = ½ kₛ (u·N)², 'pressure' follower load p J F⁻ᵀ N."""
    nb = 4 if order == 1 else 10
    fv = TET_FACETS[lf]
    bary, wt = tri_rule(2 if order == 1 else 4)
    dl, _ = barycentric_gradients(X)
    nw = np.cross(X[fv[1]] - X[fv[0]], X[fv[2]] - X[fv[0]])
    area, n0 = 0.5 * np.linalg.norm(nw), nw / np.linalg.norm(nw)
    U = ue.reshape(nb, 3)
    Ke, re = np.zeros((3 * nb, 3 * nb)), np.zeros(3 * nb)
    for b3, w in zip(bary, wt):
        lam = np.zeros(4)
        lam[list(fv)] = b3
        N, dN = shape(order, lam)
        G = dN @ dl
        dG = w * area
        uq = N @ U
        if bc == "robin":
            g, H = 2.0 * param * uq, 2.0 * param * np.eye(3)
        elif bc == "spring":
            g, H = param * (uq @ n0) * n0, param * np.outer(n0, n0)
        else:
            F = np.eye(3) + U.T @ G
            Fi, J = np.linalg.inv(F), np.linalg.det(F)
            p = param * (1.0 if pnodal is None else float(lam @ pnodal))
            v = Fi.T @ n0
            g = p * J * v
        re += np.einsum("a,c->ac", N, g).ravel() * dG
        if want_K:
            if bc in ("robin", "spring"):
                Ke += np.einsum("a,cd,b->acbd", N, H, N).reshape(3 * nb, 3 * nb) * dG
            else:
                gF = G @ Fi                               # (nb, 3): ∇N_b · F⁻¹
                # ∂(J F⁻ᵀN)_c / ∂F_dl ∇N_b[l] = J (v_c (∇N_b F⁻¹)_d − v_d (∇N_b F⁻¹)_c)
                T = p * J * (np.einsum("c,bd->cbd", v, gF) - np.einsum("d,bc->cbd", v, gF))
                Ke += np.einsum("a,cbd->acbd", N, T).reshape(3 * nb, 3 * nb) * dG
    return Ke, re


def assemble_facets(order, xyz, conn, cell_dofs, facets, u, bc, param, rowptr=None, colidx=None, pfield=None):
    want_K = rowptr is not None
    nz = np.zeros(int(rowptr[-1])) if want_K else None
    r = np.zeros(len(u))
    for c, lf in np.asarray(facets).reshape(-1, 2):
        d = cell_dofs[c]
        Ke, re = facet_element(order, xyz[conn[c]], int(lf), u[d], bc, param, None if pfield is None else pfield[c], want_K)
        r[d] += re
        if want_K:
            for i, di in enumerate(d):
                lo, hi = rowptr[di], rowptr[di + 1]
                nz[lo + np.searchsorted(colidx[lo:hi], d)] += Ke[i]
    return nz, r


def csr_matvec(rowptr, colidx, nz, v):
    out = np.zeros(len(rowptr) - 1)
    np.add.at(out, np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr)), nz * v[colidx])
    return out


def perturbed_renumbered_box(tb, nel, left, right, amplitude=0.15, seed=1):
    """A tetrahedral box whose interior AND boundary nodes are moved by ≤ amplitude·h per axis and whose nodes and cells are randomly renumbered.
    Returns the Grid (no named facet sets: the boundary is no longer flat)."""
    g = tb.generate_mesh(tb.Tetrahedron, nel, left, right)
    rng = np.random.default_rng(seed)
    h = (np.asarray(right, dtype=float) - np.asarray(left, dtype=float)) / np.asarray(nel)
    xyz = g.xyz + rng.uniform(-amplitude, amplitude, g.xyz.shape) * h
    node_perm = rng.permutation(g.n_nodes)            # new number of node v
    cell_perm = rng.permutation(g.n_cells)
    inv = np.empty_like(node_perm)
    inv[node_perm] = np.arange(g.n_nodes)
    return tb.Grid(tb.Tetrahedron, xyz[inv], node_perm[g.conn[cell_perm]].astype(np.int32))


def volumes(xyz, conn):
    X = xyz[conn]
    return np.einsum("ij,ij->i", np.cross(X[:, 1] - X[:, 0], X[:, 2] - X[:, 0]), X[:, 3] - X[:, 0]) / 6.0
