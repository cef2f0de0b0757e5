"""Independent NumPy restatement of the multi-domain conventions (thunderbolt.jl_amd/multidomain.py, csrc/tb_interface.hip): shared facets counted
by brute force, the interface matrix assembled densely from the CELLS' own geometry maps (not the facet parametrisation the kernel uses), the packed
state map of src/discretization/fem.jl:514-521, and the dense scatter the planner driver is checked against.  Nothing here imports the package."""
import numpy as np

QUAD, HEX = 2, 3                                                      # TB_QUAD4, TB_HEX8
FACETS = {QUAD: ((0, 1), (1, 2), (2, 3), (3, 0)),
          HEX: ((0, 3, 2, 1), (0, 1, 5, 4), (1, 2, 6, 5), (2, 3, 7, 6), (0, 4, 7, 3), (4, 5, 6, 7))}
# reference positions of the local vertices (Ferrite's RefQuadrilateral / RefHexahedron)
CORNERS = {QUAD: np.array([(-1, -1), (1, -1), (1, 1), (-1, 1)], dtype=float),
           HEX: np.array([(-1, -1, -1), (1, -1, -1), (1, 1, -1), (-1, 1, -1), (-1, -1, 1), (1, -1, 1), (1, 1, 1), (-1, 1, 1)], dtype=float)}


def shared_facets(kind, conn, cells_a, cells_b):
    """{(cell_a, local facet of a): (cell_b, local facet of b)} of the facets a cell of a and a cell of b have in common — brute force on node sets"""
    of_b = {}
    for c in cells_b:
        for lf, f in enumerate(FACETS[kind]):
            of_b[frozenset(int(conn[c, v]) for v in f)] = (int(c), lf)
    out = {}
    for c in cells_a:
        for lf, f in enumerate(FACETS[kind]):
            hit = of_b.get(frozenset(int(conn[c, v]) for v in f))
            if hit is not None:
                out[(int(c), lf)] = hit
    return out


def gauss(q):
    return np.polynomial.legendre.leggauss(q)


def _cell_jacobian(kind, X, xi):
    """∂x/∂ξ (sdim × sdim) of the bi-/trilinear cell with vertex coordinates X at the reference point ξ"""
    s = CORNERS[kind]
    d = s.shape[1]
    J = np.zeros((d, d))
    for v in range(len(s)):
        for k in range(d):
            g = s[v, k] / 2 ** d
            for m in range(d):
                if m != k:
                    g *= 1 + s[v, m] * xi[m]
            J[:, k] += X[v, :d] * g
    return J


def _facet_shapes(nf, p):
    if nf == 2:
        return np.array([(1 - p[0]) / 2, (1 + p[0]) / 2])
    s, t = p
    return np.array([(1 - s) * (1 - t), (1 + s) * (1 - t), (1 + s) * (1 + t), (1 - s) * (1 + t)]) / 4


def _measure(kind, X, local_vertices, p):
    """facet measure of the cell at the facet point with facet coordinates p, the facet spanned by `local_vertices` in cyclic order: the image of
    the reference facet's tangents under the cell's own Jacobian"""
    nf = len(local_vertices)
    c = CORNERS[kind][list(local_vertices)]                           # reference positions of the facet's corners
    N = _facet_shapes(nf, p)
    xi = N @ c
    J = _cell_jacobian(kind, X, xi)
    if nf == 2:
        return np.linalg.norm(J @ ((c[1] - c[0]) / 2))
    # tangents of the (affine) map facet square → reference facet
    ts, tt = (c[1] - c[0]) / 2, (c[3] - c[0]) / 2
    return np.linalg.norm(np.cross(J @ ts, J @ tt))


def interface_element_matrices(kind, xyz, conn, records, pairing, G, q=2):
    """(n, 2nf, 2nf) element matrices of the interface term: the dofs of an element are a's facet nodes in facet-node order, then their copies"""
    nf = len(FACETS[kind][0])
    gx, gw = gauss(q)
    pts = [((s,), w) for s, w in zip(gx, gw)] if nf == 2 else [((s, t), ws * wt) for t, wt in zip(gx, gw) for s, ws in zip(gx, gw)]
    G = np.broadcast_to(np.asarray(G, dtype=float), (len(records),))
    out = np.zeros((len(records), 2 * nf, 2 * nf))
    for e, ((ca, la, cb, lb), pair) in enumerate(zip(records, pairing)):
        Xa, Xb = xyz[conn[ca]], xyz[conn[cb]]
        va, vb = FACETS[kind][la], tuple(int(v) for v in pair)
        assert set(vb) == set(FACETS[kind][lb]), "pairing leaves b's facet"
        for p, w in pts:
            N = _facet_shapes(nf, p)
            dG = 0.5 * (_measure(kind, Xa, va, p) + _measure(kind, Xb, vb, p)) * w
            jump = np.concatenate([N, -N])                            # [[N_I]]: + on a, − on b (the sign convention cancels in the product)
            out[e] -= G[e] * np.outer(jump, jump) * dG
    return out


def interface_dofs(kind, cell_dofs, records, pairing):
    return np.array([[cell_dofs[ca, v] for v in FACETS[kind][la]] + [cell_dofs[cb, v] for v in pair] for (ca, la, cb, lb), pair in zip(records, pairing)],
                    dtype=np.int64).reshape(len(records), -1)


def dense_interface_matrix(kind, xyz, conn, cell_dofs, ndofs, records, pairing, G, q=2):
    K = np.zeros((ndofs, ndofs))
    Ke = interface_element_matrices(kind, xyz, conn, records, pairing, G, q)
    for d, ke in zip(interface_dofs(kind, cell_dofs, records, pairing), Ke):
        K[np.ix_(d, d)] += ke
    return K


def csr_of_dense(rowptr, colidx, A):
    rows = np.repeat(np.arange(len(rowptr) - 1), np.diff(rowptr))
    return A[rows, colidx]


def dense_of_csr(rowptr, colidx, nz):
    n = len(rowptr) - 1
    A = np.zeros((n, n))
    A[np.repeat(np.arange(n), np.diff(rowptr)), colidx] = nz
    return A


def pattern_mask(rowptr, colidx):
    n = len(rowptr) - 1
    m = np.zeros((n, n), dtype=bool)
    m[np.repeat(np.arange(n), np.diff(rowptr)), colidx] = True
    return m


def heat_dofrange(subdofs, nstates, phi_index_1based):
    """fem.jl:514-521 for PointBlocked children: heat_dofrange[dof] = state_range(StateBlock(offset, npoints, nstates), k)[φidx], returned 0-based;
    blocks in the given order, a block's points its dofs in the given (ascending) order"""
    n = 1 + max(int(max(d)) for d in subdofs)
    hd = np.zeros(n, dtype=np.int64)                                   # 1-based while it is filled, 0 = unclaimed
    offset = 0
    for dofs, ns, phi in zip(subdofs, nstates, phi_index_1based):
        for k, dof in enumerate(dofs, start=1):
            hd[dof] = offset + (k - 1) * ns + phi
        offset += len(dofs) * ns
    return hd - 1, offset


def planner_scatter(edofs, nf, rowptr, colidx):
    """What the interface planner must list: per touched non-zero (ascending) its contributions (position in the facet-matrix buffer, sign) in the
    order ascending interface element, then local entry I·2nf + J.  None when a coupling is missing."""
    nd = 2 * nf
    touched = {}
    for e, d in enumerate(edofs):
        for I in range(nd):
            cols = colidx[rowptr[d[I]]:rowptr[d[I] + 1]]
            for J in range(nd):
                k = np.searchsorted(cols, d[J])
                if k == len(cols) or cols[k] != d[J]:
                    return None
                touched.setdefault(int(rowptr[d[I]] + k), []).append((e * nf * nf + (I % nf) * nf + (J % nf), -1 if I // nf == J // nf else 1))
    return sorted(touched.items())
