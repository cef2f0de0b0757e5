"""Smoothed-aggregation algebraic multigrid — SmoothedAggregationCoarseSolver(), the default pcoarse_solver of the reference's PMGPrecon
(src/solver/linear/multigrid.jl:27; its how-to imports AlgebraicMultigrid for it) — over tb_amg_* of libtbhip.so: a multigrid preconditioner that needs
only the matrix, for the meshes that have no GridHierarchy (tetrahedra, the readers' meshes, the generated ventricle).

AMGPrecon is the recipe; `materialize(pattern, ch)` gives the AlgebraicHierarchy of one matrix pattern, which pcg_solve, the Newton solver, KrylovMGSolver
and the ECG caches drive through the protocol of the geometric multigrid (materialize / tb_mg_solve).  Inside ChainedMGPrecon(PMGPrecon(), AMGPrecon())
and GMGPrecon(gh, coarse=AMGPrecon()) it replaces the dense inverse of the coarsest level (multigrid.py → tb_mg_set_coarse_amg).

Covered: one field of 1 or 3 components on the whole grid, CG, V-cycles with the Chebyshev–Jacobi smoother.  Refused with a message: the bidomain block
system (BidomainAMGPrecon in bidomain.py is its recipe), GMRES, W- and F-cycles, other smoothers, subdomain dof handlers.  Out of scope: rigid-body rotations in the near-null space (elasticity gets the
translations only), block aggregation, aggregation on the device, classical Ruge–Stüben coarsening, Float32, several ranks."""
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


class AMGPrecon:
    """AMGPrecon(theta=0.25, degree=2, interval_ratio=4.0, max_coarse=1024, max_levels=16): the recipe — strength threshold θ, degree of the smoothing
    polynomial and ratio λmax/λmin of its interval, the size at which coarsening stops (the last level is inverted densely: at most 1 024 dofs) and the
    largest number of levels."""

    def __init__(self, theta=0.25, degree=2, interval_ratio=4.0, max_coarse=1024, max_levels=16, cycle="V", smoother="chebyshev"):
        if cycle != "V":
            raise NotImplementedError("AMGPrecon: V-cycles only (W- and F-cycles are out of scope)")
        if smoother != "chebyshev":
            raise NotImplementedError("AMGPrecon: the Chebyshev-Jacobi smoother only")
        self.theta, self.degree, self.interval_ratio = float(theta), int(degree), float(interval_ratio)
        self.max_coarse, self.max_levels = int(max_coarse), int(max_levels)
        self._materialized = {}

    def check(self, dh):
        check_supported(dh)

    def materialize(self, pattern, ch=None):
        """the hierarchy of one pattern; `ch` is accepted for the protocol's sake: eliminated rows are decoupled and stay outside every aggregate"""
        key = id(pattern)
        if key not in self._materialized:
            self._materialized[key] = (AlgebraicHierarchy(pattern, self.theta, self.degree, self.interval_ratio, self.max_coarse, self.max_levels), pattern)
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

    def __init__(self, pattern, theta=0.25, degree=2, interval_ratio=4.0, max_coarse=1024, max_levels=16):
        dh, device = pattern.dmesh.dh, pattern.dmesh.device
        check_supported(dh)
        self.device, self.pattern, self.degree, self.interval_ratio = device, pattern, int(degree), float(interval_ratio)
        comp = component_labels(dh)
        self.h = C.c_void_p()
        check(lib().tb_amg_create(pattern.h, None if comp is None else comp.ctypes.data_as(C.c_void_p), float(theta), int(max_coarse), int(max_levels), C.byref(self.h)))
        self._A = None

    def setup(self, A):
        """plan (first call) and numeric phase for the matrix values `A` (after apply_zero): smoothed P, Galerkin chain, D⁻¹, λmax per level, last inverse"""
        check(lib().tb_amg_setup(self.h, _ptr(A), self.degree, self.interval_ratio))
        self._A = A                                  # the cycle reads the array: keep it alive
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
        """(dofs, non-zeros, aggregates) of a level; the last level has no aggregates"""
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

    def lambda_max(self, level):
        out = C.c_double()
        check(lib().tb_amg_level_lambda_max(self.h, level, C.byref(out)))
        return out.value

    def solve(self, A, b, x, rtol=1e-5, atol=1e-6, maxiter=1000, setup=True):
        """CG on A x = b preconditioned by one cycle (tb_pcg_solve_amg) → (iterations, residual norm); setup=False reuses the numeric phase"""
        if setup or self._A is None:
            self.setup(A)
        it, res = C.c_int(), C.c_double()
        check(lib().tb_pcg_solve_amg(self.pattern.h, _ptr(A), _ptr(b), _ptr(x), float(rtol), float(atol), int(maxiter), self.h, C.byref(it), C.byref(res)))
        return it.value, res.value

    reuse_setup = False      # set by the Newton loop under simplified_newton: the tangent, and with it the numeric phase, is the previous one

    def tb_mg_solve(self, pattern, A, b, x, rtol, atol, maxiter):
        """what pcg_solve(…, precond=<this>) runs"""
        if pattern is not self.pattern:
            raise ValueError("pcg_solve: the AMG hierarchy was materialised for another pattern")
        return self.solve(A, b, x, rtol, atol, maxiter, setup=not self.reuse_setup)

    def close(self):
        if self.h:
            lib().tb_amg_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
