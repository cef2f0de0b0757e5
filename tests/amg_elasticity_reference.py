"""NumPy / SciPy restatement of the node-wise smoothed aggregation with a near-null-space (csrc/tb_amg_block.hip; steps 1 – 7 of the method as
include/tbhip.h states it) on top of tests/amg_reference.py, whose aggregation, cycle and CG it uses unchanged: candidates' zero rows, Frobenius
strength of the node blocks, the per-aggregate modified Gram–Schmidt (columns in order, dead columns zeroed, projections kept), the smoothed
prolongator, the Galerkin operator with the unit diagonal of dead coarse dofs.  λmax(D⁻¹A) per level is an input, as in amg_reference.hierarchy.
Also a small host assembler of Q1 linear elasticity for the tests that run without a device."""
import numpy as np
import scipy.sparse as sp

import amg_reference as ref

DEAD_RATIO = 1e-8


# ------------------------------------------------------------------------------------------------ Q1 linear elasticity on the host
def q1_elasticity(tb, dh, E=1.0, nu=0.3):
    """the stiffness matrix of isotropic linear elasticity on the trilinear hexahedra of a first-order 3-component DofHandler (2 × 2 × 2 Gauss
    points), in the handler's dof numbering; free-free: eliminate() applies the conditions"""
    g = dh.grid
    signs = np.asarray(tb.api._HEX8_SIGNS, dtype=np.float64)                 # (8, 3): the reference positions of the vertices
    lam, mu = E * nu / ((1 + nu) * (1 - 2 * nu)), E / (2 * (1 + nu))
    D = np.zeros((6, 6))
    D[:3, :3] = lam
    D[np.arange(3), np.arange(3)] += 2 * mu
    D[np.arange(3, 6), np.arange(3, 6)] = mu
    X = np.asarray(g.xyz, dtype=np.float64)[g.conn]                          # (nc, 8, 3)
    nc = len(X)
    Ke = np.zeros((nc, 24, 24))
    gp = 1.0 / np.sqrt(3.0)
    for q in np.ndindex(2, 2, 2):
        xi = (2 * np.asarray(q) - 1) * gp
        dN = np.stack([0.125 * signs[:, d] * np.prod(np.delete(1 + signs * xi, d, axis=1), axis=1) for d in range(3)], axis=1)   # (8, 3)
        J = np.einsum("cak,ad->ckd", X, dN)                                  # dx_k / dxi_d
        det = np.linalg.det(J)
        G = np.einsum("ad,cdk->cak", dN, np.linalg.inv(J))                   # dN_a / dx_k
        Bm = np.zeros((nc, 6, 24))
        for a in range(8):
            Bm[:, 0, 3 * a], Bm[:, 1, 3 * a + 1], Bm[:, 2, 3 * a + 2] = G[:, a, 0], G[:, a, 1], G[:, a, 2]
            Bm[:, 3, 3 * a], Bm[:, 3, 3 * a + 1] = G[:, a, 1], G[:, a, 0]
            Bm[:, 4, 3 * a + 1], Bm[:, 4, 3 * a + 2] = G[:, a, 2], G[:, a, 1]
            Bm[:, 5, 3 * a], Bm[:, 5, 3 * a + 2] = G[:, a, 2], G[:, a, 0]
        Ke += np.einsum("cia,ij,cjb,c->cab", Bm, D, Bm, np.abs(det))
    dofs = np.asarray(dh.cell_dofs)
    rows = np.repeat(dofs, 24, axis=1).ravel()
    cols = np.tile(dofs, (1, 24)).ravel()
    return ref.canonical(sp.csr_matrix((Ke.ravel(), (rows, cols)), shape=(dh.ndofs, dh.ndofs)))


# ------------------------------------------------------------------------------------------------ steps 1, 2: candidates, node strength
def zero_rows(A, B):
    """step 1: the rows of B of the dofs whose row of A has no non-zero off-diagonal entry are zero"""
    A = ref.canonical(A)
    rows = ref.rows_of(A)
    coupled = np.zeros(A.shape[0], dtype=bool)
    coupled[rows[(rows != A.indices) & (A.data != 0.0)]] = True
    B = B.copy()
    B[~coupled] = 0.0
    return B


def node_strength(A, node, n_nodes, theta):
    """→ (G, flags, nz): the node graph with the Frobenius norms of the blocks (canonical CSR, stored zeros kept), one strength byte per non-zero of
    G (amg_reference.strength on G, no labels) and, per non-zero of A, its non-zero of G"""
    A = ref.canonical(A)
    I, J = node[ref.rows_of(A)], node[A.indices]
    numbered = ref.canonical(sp.csr_matrix((np.ones(A.nnz), (I, J)), shape=(n_nodes, n_nodes)))
    numbered.data = np.arange(1, numbered.nnz + 1, dtype=np.float64)
    nz = np.asarray(numbered[I, J]).ravel().astype(np.int64) - 1
    sums = np.zeros(numbered.nnz)
    np.add.at(sums, nz, A.data ** 2)                                         # in ascending non-zero of A: stored row-major order within a block
    G = sp.csr_matrix((np.sqrt(sums), numbered.indices, numbered.indptr), shape=(n_nodes, n_nodes))
    return G, ref.strength(G, None, theta), nz


# ------------------------------------------------------------------------------------------------ step 4: per-aggregate QR
def qr_block(Ba):
    """modified Gram–Schmidt, columns in order → (Q, R, dead, ratio): ratio[j] = norm after orthogonalisation / norm before (0 for a zero column)"""
    m, k = Ba.shape
    Q, R = Ba.astype(np.float64).copy(), np.zeros((k, k))
    dead, ratio = np.zeros(k, dtype=np.uint8), np.zeros(k)
    for j in range(k):
        before = np.sqrt(Q[:, j] @ Q[:, j])
        for i in range(j):
            if dead[i]:
                continue
            R[i, j] = Q[:, i] @ Q[:, j]
            Q[:, j] -= R[i, j] * Q[:, i]
        after = np.sqrt(Q[:, j] @ Q[:, j])
        ratio[j] = after / before if before > 0.0 else 0.0
        if after <= DEAD_RATIO * before:
            dead[j] = 1
            Q[:, j] = 0.0
        else:
            R[j, j] = after
            Q[:, j] /= after
    return Q, R, dead, ratio


def aggregate_dofs(agg, na):
    """the dofs of every aggregate, ascending → (ptr, dofs)"""
    inside = np.flatnonzero(agg >= 0)
    order = inside[np.argsort(agg[inside], kind="stable")]
    ptr = np.concatenate([[0], np.cumsum(np.bincount(agg[inside], minlength=na))]).astype(np.int64)
    return ptr, order.astype(np.int32)


def tentative(B, agg, na):
    """→ (T csr n × k·na with k stored values per aggregated row, B_{l+1}, dead, ratios, blocks): blocks[a] = B_a"""
    n, k = B.shape
    ptr, dofs = aggregate_dofs(agg, na)
    dense, Bc = np.zeros((n, k)), np.zeros((k * na, k))
    dead, ratios, blocks = np.zeros(k * na, dtype=np.uint8), np.zeros(k * na), []
    for a in range(na):
        d = dofs[ptr[a]:ptr[a + 1]]
        blocks.append(B[d].copy())
        Q, R, dd, rr = qr_block(B[d])
        dense[d], Bc[k * a:k * a + k], dead[k * a:k * a + k], ratios[k * a:k * a + k] = Q, R, dd, rr
    inside = np.flatnonzero(agg >= 0)
    tptr = np.concatenate([[0], np.cumsum(np.where(agg >= 0, k, 0))]).astype(np.int64)
    col = (k * agg[inside, None] + np.arange(k)[None, :]).ravel().astype(np.int32)
    return sp.csr_matrix((dense[inside].ravel(), col, tptr), shape=(n, k * na)), Bc, dead, ratios, blocks


# ------------------------------------------------------------------------------------------------ patterns, as the host planner records them
def plan(A, node, n_nodes, node_flags, G, k):
    A = ref.canonical(A)
    n = A.shape[0]
    node_agg, na = ref.aggregate(G.indptr, G.indices, node_flags)
    agg = node_agg[node].astype(np.int32)
    aptr, adofs = aggregate_dofs(agg, na)
    inside_idx = np.flatnonzero(agg >= 0)
    sT = sp.csr_matrix((np.ones(len(inside_idx) * k), ((np.repeat(inside_idx, k)), (k * agg[inside_idx, None] + np.arange(k)[None, :]).ravel())), shape=(n, k * na))
    inside = sp.diags((agg >= 0).astype(float))
    sA = ref.structure(A)
    P = ref.canonical(inside @ (sA @ sT))
    P.eliminate_zeros()
    P = ref.structure(P)
    numbered = sp.csr_matrix((np.arange(1, P.nnz + 1, dtype=np.float64), P.indices, P.indptr), shape=P.shape)
    R = ref.canonical(numbered.T)
    AP = ref.structure(ref.canonical(sA @ P))
    Ac = ref.structure(ref.canonical(ref.structure(R) @ AP))
    return dict(node_agg=node_agg, agg=agg, na=na, nc=k * na, adof_ptr=aptr, adof=adofs, P=ref.pattern_of(P), R=ref.pattern_of(R),
                r_perm=(R.data - 1).astype(np.int64), AP=ref.pattern_of(AP), Ac=ref.pattern_of(Ac))


# ------------------------------------------------------------------------------------------------ the hierarchy
def hierarchy(A, node, n_nodes, B, lam=None, theta=0.25, max_coarse=1024, max_levels=16):
    """levels[l]: dict(A, node, n_nodes, B, and — but for the last — G, node_S, S, agg, plan, T, dead, ratios, blocks, lam, P); amg_reference.vcycle
    runs on it.  lam as in amg_reference.hierarchy."""
    lam_of = (lambda l, M: lam[l]) if isinstance(lam, (list, tuple)) else (lambda l, M: (lam or (lambda X: 1.05 * ref.lambda_max_exact(X)))(M))
    levels = []
    A = ref.canonical(A)
    k = B.shape[1]
    node = np.asarray(node)
    while True:
        l = len(levels)
        lev = dict(A=A, node=node, n_nodes=n_nodes, B=B)
        levels.append(lev)
        n = A.shape[0]
        if n <= max_coarse or l + 1 >= max_levels:
            break
        Bz = zero_rows(A, B)
        G, node_S, nz = node_strength(A, node, n_nodes, theta)
        pl = plan(A, node, n_nodes, node_S, G, k)
        if pl["na"] == 0 or pl["nc"] >= n:
            break
        T, Bc, dead, ratios, blocks = tentative(Bz, pl["agg"], pl["na"])
        lev.update(B=Bz, G=G, node_S=node_S, S=node_S[nz], agg=pl["agg"], plan=pl, T=T, dead=dead, ratios=ratios, blocks=blocks, lam=lam_of(l, A))
        inside = sp.diags((pl["agg"] >= 0).astype(float))
        omega = 4.0 / (3.0 * lev["lam"])
        P = ref.on_pattern(inside @ (T - omega * (sp.diags(ref.inverse_diagonal(A)) @ (A @ T))), pl["P"], (n, pl["nc"]))
        lev["P"] = P
        Ac = ref.on_pattern(P.T @ (A @ P), pl["Ac"], (pl["nc"], pl["nc"]))
        rows = ref.rows_of(Ac)
        Ac.data[(rows == Ac.indices) & (dead[rows] != 0)] = 1.0                  # step 6
        A, B = Ac, Bc
        node, n_nodes = np.arange(pl["nc"], dtype=np.int32) // k, pl["na"]
    return levels


def operator_complexity(levels):
    return sum(lev["A"].nnz for lev in levels) / levels[0]["A"].nnz
