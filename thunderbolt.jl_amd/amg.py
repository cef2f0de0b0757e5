"""Smoothed-aggregation algebraic multigrid — SmoothedAggregationCoarseSolver(), the default pcoarse_solver of the reference's PMGPrecon
(src/solver/linear/multigrid.jl:27; its how-to imports AlgebraicMultigrid for it) — over tb_amg_* of libtbhip.so: a multigrid preconditioner that needs
only the matrix, for the meshes that have no GridHierarchy (tetrahedra, the readers' meshes, the generated ventricle).

AMGPrecon is the recipe; `materialize(pattern, ch)` gives the AlgebraicHierarchy of one matrix pattern, which pcg_solve, the Newton solver, KrylovMGSolver
and the ECG caches drive through the protocol of the geometric multigrid (materialize / tb_mg_solve).  Inside ChainedMGPrecon(PMGPrecon(), AMGPrecon())
and GMGPrecon(gh, coarse=AMGPrecon()) it replaces the dense inverse of the coarsest level (multigrid.py → tb_mg_set_coarse_amg).

Covered: one field of 1 or 3 components on the whole grid, CG and — for mildly non-symmetric matrices with a positive diagonal, the hierarchy in
general mode: a pivoted, unsymmetrised last-level inverse — restarted GMRES (gmres_solve(…, precond=AMGPrecon(…))), V-cycles with the Chebyshev–Jacobi
smoother.  One hierarchy serves one kind of solve cheaply: CG after GMRES on it, or the other way round, flips the mode and sets up again.  For elasticity,
AMGPrecon(near_nullspace="rigid_body") aggregates node by node and carries the six rigid-body modes through the hierarchy (Vaněk–Mandel–Brezina: a
per-aggregate QR of the candidates gives the tentative prolongator and the candidates of the level below; the method as include/tbhip.h states it);
without the keyword the prolongator has one constant per aggregate and component, which carries the translations only.  Refused with a message: the
bidomain block system (BidomainAMGPrecon in bidomain.py is its recipe), W- and F-cycles, other smoothers, subdomain dof handlers, "rigid_body" on
a scalar or second-order field.  Out of scope: block-Jacobi smoothers, candidates in the current configuration, candidates on scalar fields,
aggregation on the device, classical Ruge–Stüben coarsening, Float32, several ranks."""
import ctypes as C

import numpy as np

from . import _lib as L
from ._lib import check, lib
from .api import _ptr


def component_labels(dh):
    """the component of every dof (int8), in any numbering: local dof l of a cell carries component l mod ncomp; None for a scalar field"""
    nc = dh.ip.ncomp
    if nc == 1:
        return None
    comp = np.zeros(dh.ndofs, dtype=np.int8)
    for c in range(nc):
        comp[dh.cell_dofs[:, c::nc].ravel()] = c
    return comp


def _first_order_vector_field(dh, who):
    if dh.ip.ncomp != 3:
        raise ValueError("%s: a near-null-space lives on the node blocks of a 3-component field (got %d component%s)" % (who, dh.ip.ncomp, "" if dh.ip.ncomp == 1 else "s"))
    if dh.ip.order != 1:
        raise ValueError("%s: a first-order field only (Q1 hexahedra, P1 tetrahedra); a second-order field goes through ChainedMGPrecon(PMGPrecon(), AMGPrecon(near_nullspace=...))" % who)


def dof_nodes(dh):
    """the grid node of every dof of a first-order 3-component field (int32), in any numbering: local dof l of a cell sits on vertex l // 3"""
    _first_order_vector_field(dh, "dof_nodes")
    node = np.zeros(dh.ndofs, dtype=np.int32)
    for v in range(dh.grid.conn.shape[1]):
        for c in range(3):
            node[dh.cell_dofs[:, 3 * v + c]] = dh.grid.conn[:, v]
    return node


def rigid_body_modes(dh):
    """(ndofs, 6): the three translations and the three rotations about the mesh centroid of a first-order 3-component field, the coordinates scaled by
    the largest centred coordinate so that every entry is O(1).  Reference coordinates: the candidates are not updated with the deformation (at finite
    strain the tangent's near-null space moves with it; the reference modes stay a good coarse space as long as the deformation is moderate)."""
    _first_order_vector_field(dh, "rigid_body_modes")
    node, comp = dof_nodes(dh), component_labels(dh)
    xyz = np.asarray(dh.grid.xyz, dtype=np.float64)
    x = xyz - xyz.mean(axis=0)
    x = x / max(np.abs(x).max(), 1e-300)
    x = x[node]                                              # per dof
    B = np.zeros((dh.ndofs, 6))
    for c in range(3):
        B[comp == c, c] = 1.0
    # rotation about axis a: u = e_a × x
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        B[comp == c, 3 + a] = x[comp == c, b]
        B[comp == b, 3 + a] = -x[comp == b, c]
    return B


def resolve_near_nullspace(near_nullspace, dh, who="AMGPrecon"):
    """None, or (n_nodes, node_of_dof, B) for the field of `dh`"""
    if near_nullspace is None:
        return None
    if isinstance(near_nullspace, str):
        if near_nullspace != "rigid_body":
            raise ValueError("%s: near_nullspace is None, \"rigid_body\" or an (ndofs, k) array" % who)
        _first_order_vector_field(dh, who + "(near_nullspace=\"rigid_body\")")
        B = rigid_body_modes(dh)
    else:
        _first_order_vector_field(dh, who + "(near_nullspace=<array>)")
        B = np.ascontiguousarray(near_nullspace, dtype=np.float64)
        if B.ndim != 2 or B.shape[0] != dh.ndofs or not 1 <= B.shape[1] <= 6:
            raise ValueError("%s: near_nullspace is an (ndofs, k) array with 1 <= k <= 6 (got shape %s for %d dofs)" % (who, B.shape, dh.ndofs))
    return len(dh.grid.xyz), dof_nodes(dh), np.ascontiguousarray(B)


class AMGPrecon:
    """AMGPrecon(theta=0.25, degree=2, interval_ratio=4.0, max_coarse=1024, max_levels=16, near_nullspace=None): the recipe — strength threshold θ,
    degree of the smoothing polynomial and ratio λmax/λmin of its interval, the size at which coarsening stops (the last level is inverted densely: at
    most 1 024 dofs), the largest number of levels, and the near-null-space: None (one constant per aggregate and component), "rigid_body" (node-wise
    aggregation with the six rigid-body modes of a first-order 3-component field, in reference coordinates) or an (ndofs, k ≤ 6) array of the user's
    own candidates on the same node blocks."""

    def __init__(self, theta=0.25, degree=2, interval_ratio=4.0, max_coarse=1024, max_levels=16, cycle="V", smoother="chebyshev", near_nullspace=None):
        if cycle != "V":
            raise NotImplementedError("AMGPrecon: V-cycles only (W- and F-cycles are out of scope)")
        if smoother != "chebyshev":
            raise NotImplementedError("AMGPrecon: the Chebyshev-Jacobi smoother only")
        self.theta, self.degree, self.interval_ratio = float(theta), int(degree), float(interval_ratio)
        self.max_coarse, self.max_levels = int(max_coarse), int(max_levels)
        if isinstance(near_nullspace, str) and near_nullspace != "rigid_body":
            raise ValueError("AMGPrecon: near_nullspace is None, \"rigid_body\" or an (ndofs, k) array")
        self.near_nullspace = near_nullspace
        self._materialized = {}

    def check(self, dh):
        check_supported(dh)
        resolve_near_nullspace(self.near_nullspace, dh)

    def materialize(self, pattern, ch=None):
        """the hierarchy of one pattern; `ch` is accepted for the protocol's sake: eliminated rows are decoupled and stay outside every aggregate"""
        key = id(pattern)
        if key not in self._materialized:
            self._materialized[key] = (AlgebraicHierarchy(pattern, self.theta, self.degree, self.interval_ratio, self.max_coarse, self.max_levels,
                                                            near_nullspace=self.near_nullspace), pattern)
        return self._materialized[key][0]


def check_supported(dh):
    if dh.cell_dofs.shape[0] != dh.grid.n_cells:
        raise NotImplementedError("AMGPrecon: subdomain dof handlers are out of scope")
    if dh.ip.ncomp not in (1, 3):
        raise NotImplementedError("AMGPrecon: fields of 1 or 3 components (got %d)" % dh.ip.ncomp)


class AlgebraicHierarchy:
    """A materialised AMGPrecon (tb_amg).  Level 0 is the matrix of `pattern`, level l + 1 the Galerkin operator of level l's aggregates; the first
    `setup` plans (strength on the device, aggregation on the host), every later one redoes the numeric phase on the same aggregates; `replan` drops
    the plan."""

    def __init__(self, pattern, theta=0.25, degree=2, interval_ratio=4.0, max_coarse=1024, max_levels=16, near_nullspace=None):
        dh, device = pattern.dmesh.dh, pattern.dmesh.device
        check_supported(dh)
        nns = resolve_near_nullspace(near_nullspace, dh)
        self.device, self.pattern, self.degree, self.interval_ratio = device, pattern, int(degree), float(interval_ratio)
        comp = component_labels(dh)
        self.h = C.c_void_p()
        check(lib().tb_amg_create(pattern.h, None if comp is None else comp.ctypes.data_as(C.c_void_p), float(theta), int(max_coarse), int(max_levels), C.byref(self.h)))
        self._A = None
        self.k = 0
        if nns is not None:
            self.set_near_nullspace(*nns)

    def set_near_nullspace(self, n_nodes, node_of_dof, B):
        """k candidates on node blocks (tb_amg_set_near_nullspace): before the first setup, or after replan() — a planned hierarchy refuses"""
        node = np.ascontiguousarray(node_of_dof, dtype=np.int32)
        B = np.ascontiguousarray(B, dtype=np.float64)
        if B.ndim != 2 or len(node) != B.shape[0]:
            raise ValueError("set_near_nullspace: B is (ndofs, k) and node_of_dof has ndofs entries")
        check(lib().tb_amg_set_near_nullspace(self.h, int(n_nodes), node.ctypes.data_as(L.c_i32p), B.shape[1], B.ctypes.data_as(L.c_dp)))
        self.k = B.shape[1]
        return self

    general = False          # set_general: the matrix need not be symmetric (pivoted last-level inverse, nothing symmetrised)
    n_setups = 0             # numeric set-ups so far

    def set_general(self, general):
        """general mode on or off (tb_amg_set_general); a change drops the numeric phase, so the next solve or `setup` redoes it"""
        general = bool(general)
        if general != self.general:
            check(lib().tb_amg_set_general(self.h, int(general)))
            self.general = general
            self._A = None
        return self

    def setup(self, A):
        """plan (first call) and numeric phase for the matrix values `A` (after apply_zero): smoothed P, Galerkin chain, D⁻¹, λmax per level, last inverse"""
        check(lib().tb_amg_setup(self.h, _ptr(A), self.degree, self.interval_ratio))
        self._A = A                                  # the cycle reads the array: keep it alive
        self.n_setups += 1
        return self

    def replan(self):
        check(lib().tb_amg_replan(self.h))
        self._A = None
        return self

    def apply(self, r, z):
        check(lib().tb_amg_apply(self.h, _ptr(r), _ptr(z)))
        return z

    @property
    def n_levels(self):
        n = C.c_int()
        check(lib().tb_amg_n_levels(self.h, C.byref(n)))
        return n.value

    def level_size(self, level):
        """(dofs, non-zeros, aggregates) of a level; the last level has no aggregates.  With a near-null-space of k candidates the third number is the
        dofs of the level below, k per aggregate"""
        n, nnz, na = C.c_int64(), C.c_int64(), C.c_int64()
        check(lib().tb_amg_level_size(self.h, level, C.byref(n), C.byref(nnz), C.byref(na)))
        return n.value, nnz.value, na.value

    def level_matrix(self, level):
        """A_l as a scipy.sparse.csr_matrix (stored zeros kept)"""
        import scipy.sparse as sparse
        n, nnz, _ = self.level_size(level)
        ptr, col, val = np.empty(n + 1, dtype=np.int64), np.empty(nnz, dtype=np.int32), np.empty(nnz)
        check(lib().tb_amg_level_csr(self.h, level, ptr.ctypes.data_as(L.c_i64p), col.ctypes.data_as(L.c_i32p), val.ctypes.data_as(L.c_dp)))
        return sparse.csr_matrix((val, col, ptr), shape=(n, n))

    def prolongator(self, level):
        """P from level + 1 to level as a scipy.sparse.csr_matrix"""
        import scipy.sparse as sparse
        n, _, na = self.level_size(level)
        nnz = C.c_int64()
        check(lib().tb_amg_level_prolongator(self.h, level, C.byref(nnz), None, None, None))
        ptr, col, val = np.empty(n + 1, dtype=np.int64), np.empty(nnz.value, dtype=np.int32), np.empty(nnz.value)
        check(lib().tb_amg_level_prolongator(self.h, level, None, ptr.ctypes.data_as(L.c_i64p), col.ctypes.data_as(L.c_i32p), val.ctypes.data_as(L.c_dp)))
        return sparse.csr_matrix((val, col, ptr), shape=(n, na))

    def aggregates(self, level):
        """the aggregate of every dof of the level (−1: outside every aggregate)"""
        out = np.empty(self.level_size(level)[0], dtype=np.int32)
        check(lib().tb_amg_level_aggregates(self.h, level, out.ctypes.data_as(L.c_i32p)))
        return out

    def strength(self, level):
        """one byte per non-zero of A_l: the symmetrised strength graph"""
        out = np.empty(self.level_size(level)[1], dtype=np.uint8)
        check(lib().tb_amg_level_strength(self.h, level, out.ctypes.data_as(C.c_void_p)))
        return out

    def _k(self, level):
        k = C.c_int()
        check(lib().tb_amg_level_near_nullspace(self.h, level, C.byref(k), None))
        return k.value

    def nodes(self, level):
        """the node of every dof of the level (with a near-null-space: level 0 the grid's nodes, below the aggregates of the level above)"""
        out = np.empty(self.level_size(level)[0], dtype=np.int32)
        check(lib().tb_amg_level_nodes(self.h, level, None, out.ctypes.data_as(L.c_i32p)))
        return out

    def near_nullspace(self, level):
        """B_l, (n_l, k): the candidates of the level, rows of eliminated dofs zeroed"""
        out = np.empty((self.level_size(level)[0], self._k(level)))
        check(lib().tb_amg_level_near_nullspace(self.h, level, None, out.ctypes.data_as(L.c_dp)))
        return out

    def tentative(self, level):
        """T_l as a scipy.sparse.csr_matrix (n_l, k · aggregates): row i holds k stored values in the column block of its node's aggregate"""
        import scipy.sparse as sparse
        n, _, nc = self.level_size(level)
        k = self._k(level)
        dense = np.empty((n, k))
        check(lib().tb_amg_level_tentative(self.h, level, dense.ctypes.data_as(L.c_dp)))
        agg = self.aggregates(level)
        inside = np.flatnonzero(agg >= 0)
        ptr = np.concatenate([[0], np.cumsum(np.where(agg >= 0, k, 0))]).astype(np.int64)
        col = (k * agg[inside, None] + np.arange(k)[None, :]).ravel().astype(np.int32)
        return sparse.csr_matrix((dense[inside].ravel(), col, ptr), shape=(n, nc))

    def dead(self, level):
        """one byte per dof of level + 1: 1 where the aggregate's QR found the column dead (unit diagonal, decoupled)"""
        out = np.empty(self.level_size(level)[2], dtype=np.uint8)
        check(lib().tb_amg_level_dead(self.h, level, out.ctypes.data_as(C.c_void_p)))
        return out

    def lambda_max(self, level):
        out = C.c_double()
        check(lib().tb_amg_level_lambda_max(self.h, level, C.byref(out)))
        return out.value

    def solve(self, A, b, x, rtol=1e-5, atol=1e-6, maxiter=1000, setup=True):
        """CG on A x = b preconditioned by one cycle (tb_pcg_solve_amg) → (iterations, residual norm); setup=False reuses the numeric phase"""
        self.set_general(False)
        if setup or self._A is None:
            self.setup(A)
        it, res = C.c_int(), C.c_double()
        check(lib().tb_pcg_solve_amg(self.pattern.h, _ptr(A), _ptr(b), _ptr(x), float(rtol), float(atol), int(maxiter), self.h, C.byref(it), C.byref(res)))
        return it.value, res.value

    def solve_gmres(self, A, b, x, rtol=1e-5, atol=1e-6, maxiter=1000, restart=50, setup=True, general=True):
        """GMRES(restart) on A x = b with one cycle as the fixed right preconditioner (tb_gmres_solve_amg) → (Arnoldi steps, residual norm).  The
        hierarchy goes to general mode first (general=False keeps the symmetrised last-level inverse: for measurements); setup=False reuses the
        numeric phase unless the mode changed"""
        self.set_general(general)
        if setup or self._A is None:
            self.setup(A)
        it, res = C.c_int(), C.c_double()
        check(lib().tb_gmres_solve_amg(self.pattern.h, _ptr(A), _ptr(b), _ptr(x), float(rtol), float(atol), int(maxiter), int(restart), self.h, C.byref(it),
                                       C.byref(res)))
        return it.value, res.value

    reuse_setup = False      # set by the Newton loop under simplified_newton: the tangent, and with it the numeric phase, is the previous one

    def tb_mg_solve(self, pattern, A, b, x, rtol, atol, maxiter):
        """what pcg_solve(…, precond=<this>) runs"""
        if pattern is not self.pattern:
            raise ValueError("pcg_solve: the AMG hierarchy was materialised for another pattern")
        return self.solve(A, b, x, rtol, atol, maxiter, setup=not self.reuse_setup)

    def tb_mg_gmres_solve(self, pattern, A, b, x, rtol, atol, maxiter, restart):
        """what gmres_solve(…, precond=<this>) runs"""
        if pattern is not self.pattern:
            raise ValueError("gmres_solve: the AMG hierarchy was materialised for another pattern")
        return self.solve_gmres(A, b, x, rtol, atol, maxiter, restart, setup=not self.reuse_setup)

    def close(self):
        if self.h:
            lib().tb_amg_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
