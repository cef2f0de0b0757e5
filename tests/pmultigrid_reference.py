"""numpy-only restatement of the p-level of the multigrid (tb_mg_planners.cpp: build_p_transfer) for the tests: dense P between a second-order and
a first-order hexahedral field on the same cells, from the two cell-dof tables and the tensor indices of the 27 nodes.  A Q1 function at the Q2 node
of tensor index t ∈ {0, 1, 2}³ is the trilinear interpolant of the 8 vertex values at ξ = t − 1: weights 1, ½, ¼, ⅛ on the vertices the index
selects.  Everything else — PᵀAP, the smoother, the cycle — is tests/multigrid_reference.py, imported."""
import numpy as np

from multigrid_reference import chebyshev, csr_to_dense, dense_to_csr, galerkin, vcycle  # noqa: F401  (re-exported for the tests)

HEX8_SIGNS = np.array([(-1, -1, -1), (1, -1, -1), (1, 1, -1), (-1, 1, -1), (-1, -1, 1), (1, -1, 1), (1, 1, 1), (-1, 1, 1)], dtype=np.float64)


def local_P(tb):
    """(27, 8): the Q1 shape functions at the Q2 nodes of the reference cell"""
    xi = np.asarray(tb.api._HEX27_TIX, dtype=np.float64) - 1.0
    return 0.125 * np.prod(1.0 + HEX8_SIGNS[None, :, :] * xi[:, None, :], axis=2)


def dense_p_level(tb, dh_fine, dh_coarse, prescribed_fine=None):
    """P (Q2 dofs × Q1 dofs) and the flags of the prescribed coarse dofs: a coarse dof is prescribed iff the fine vertex dof it coincides with is; rows of
    prescribed fine dofs and columns of prescribed coarse dofs are zero"""
    nc = dh_fine.ip.ncomp
    assert dh_coarse.ip.ncomp == nc and dh_fine.cell_dofs.shape[0] == dh_coarse.cell_dofs.shape[0]
    N = local_P(tb)
    P = np.full((dh_fine.ndofs, dh_coarse.ndofs), np.nan)
    seen = np.zeros(dh_fine.ndofs, dtype=bool)
    twin = np.full(dh_coarse.ndofs, -1, dtype=np.int64)
    for c in range(dh_fine.cell_dofs.shape[0]):
        for k in range(nc):
            fd, cd = dh_fine.cell_dofs[c, k::nc], dh_coarse.cell_dofs[c, k::nc]
            rows = np.zeros((27, dh_coarse.ndofs))
            rows[:, cd] = N
            old = seen[fd]
            assert np.array_equal(P[fd[old]], rows[old]), "the cells of a fine dof disagree on its row of P"
            P[fd] = rows
            seen[fd] = True
            twin[cd] = fd[:8]
    assert seen.all() and (twin >= 0).all()
    cpre = np.zeros(dh_coarse.ndofs, dtype=bool)
    if prescribed_fine is not None:
        pf = np.asarray(prescribed_fine, dtype=bool)
        cpre = pf[twin]
        P[pf, :] = 0.0
        P[:, cpre] = 0.0
    return P, cpre


def chained(tb, gh, dhs, A_fine, prescribed_fine=None):
    """dense level operators, transfers and flags of a chained hierarchy: dhs = first-order handlers of gh.grids (coarsest first) + the second-order
    handler on gh.grids[-1] → (As, Ps, prescribed), laid out as multigrid_reference.hierarchy lays them out"""
    import multigrid_reference as ref
    nl = len(dhs)
    As, Ps, pres = [None] * nl, [None] * nl, [None] * nl
    As[-1] = A_fine
    pres[-1] = np.zeros(dhs[-1].ndofs, dtype=bool) if prescribed_fine is None else np.asarray(prescribed_fine, dtype=bool)
    Ps[-1], pres[-2] = dense_p_level(tb, dhs[-1], dhs[-2], pres[-1] if pres[-1].any() else None)
    As[-2] = galerkin(Ps[-1], As[-1], pres[-2])
    for l in range(nl - 2, 0, -1):
        Ps[l], pres[l - 1] = ref.dense_P(gh.parents[l - 1], dhs[l], dhs[l - 1], pres[l] if pres[l].any() else None)
        As[l - 1] = galerkin(Ps[l], As[l], pres[l - 1])
    return As, Ps, pres
