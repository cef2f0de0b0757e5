"""Geometric multigrid preconditioner on the nested hexahedral grids of a GridHierarchy — GMGPrecon and KrylovMGSolver of the reference's multigrid
extension (src/solver/linear/multigrid.jl, ext/ThunderboltFerriteMultigridExt.jl, docs/src/literate-howto/multigrid.jl) over tb_mg_* of libtbhip.so:
Galerkin coarse operators rebuilt from every new matrix, one V(degree, degree) cycle with a Chebyshev–Jacobi smoother, an explicit coarsest inverse.

Covered: h-levels, first-order hexahedra, one field of 1 or 3 components on the whole grid, CG.  Refused with a message: PMGPrecon / ChainedMGPrecon
and second-order fields, tetrahedra, GMRES, W- and F-cycles, other smoothers, hierarchies over several ranks, subdomain dof handlers."""
import ctypes as C

import numpy as np

from . import _lib as L
from ._lib import check, lib
from .api import DofHandler, Hexahedron, LagrangeCollection, _ptr, allocate_matrix
from .meshgen import GridHierarchy


class GMGPrecon:
    """GMGPrecon(gh, degree=2, interval_ratio=4.0): the recipe — a grid hierarchy whose finest grid carries the problem, the degree of the smoothing
    polynomial and the ratio λmax/λmin of its interval.  `materialize(pattern, ch)` builds the device hierarchy for one matrix pattern; pcg_solve and
    the Newton solver do that themselves at their first solve."""

    def __init__(self, gh, degree=2, interval_ratio=4.0, cycle="V", smoother="chebyshev"):
        if not isinstance(gh, GridHierarchy):
            raise TypeError("GMGPrecon: pass a GridHierarchy")
        if cycle != "V":
            raise NotImplementedError("GMGPrecon: V-cycles only (W- and F-cycles are out of scope)")
        if smoother != "chebyshev":
            raise NotImplementedError("GMGPrecon: the Chebyshev-Jacobi smoother only")
        self.gh, self.degree, self.interval_ratio = gh, int(degree), float(interval_ratio)
        self._materialized = {}

    def check(self, dh):
        check_supported(self.gh, dh)

    def materialize(self, pattern, ch=None):
        key = (id(pattern), id(ch))
        if key not in self._materialized:
            self._materialized[key] = (MultigridHierarchy(pattern, self.gh, self.degree, self.interval_ratio, ch), pattern, ch)   # (the key's objects stay alive)
        return self._materialized[key][0]


def PMGPrecon(*args, **kwargs):
    raise NotImplementedError("PMGPrecon: p-levels are out of scope; GMGPrecon covers h-levels of first-order hexahedra")


def ChainedMGPrecon(*args, **kwargs):
    raise NotImplementedError("ChainedMGPrecon: p-levels are out of scope; GMGPrecon covers h-levels of first-order hexahedra")


def check_supported(gh, dh):
    """what the multigrid covers, checked on the host: raises for a DofHandler the hierarchy cannot serve"""
    if dh.grid.cell_kind != Hexahedron:
        raise NotImplementedError("GMGPrecon: hexahedral grids only (there is no tetrahedral uniform_refinement)")
    if dh.ip.order != 1:
        raise NotImplementedError("GMGPrecon: first-order fields only (p-levels / quadratic fields are out of scope)")
    fine = gh.grids[-1]
    if dh.grid is not fine and not (dh.grid.conn.shape == fine.conn.shape and np.array_equal(dh.grid.conn, fine.conn) and np.array_equal(dh.grid.xyz, fine.xyz)):
        raise ValueError("GMGPrecon: the finest grid of the hierarchy is not the grid of the matrix's DofHandler")
    if dh.cell_dofs.shape[0] != fine.n_cells:
        raise NotImplementedError("GMGPrecon: subdomain dof handlers are out of scope")


class MultigridHierarchy:
    """A materialised GMGPrecon: per-level DofHandlers with the fine handler's field, their patterns, the transfer and Galerkin plans (tb_mg).
    `pattern`: the DevicePattern of the system matrix on gh.grids[-1]; `ch`: its ConstraintHandler (None: no Dirichlet dofs)."""

    def __init__(self, pattern, gh, degree=2, interval_ratio=4.0, ch=None):
        dh, device = pattern.dmesh.dh, pattern.dmesh.device
        check_supported(gh, dh)
        self.device, self.gh, self.pattern, self.degree, self.interval_ratio = device, gh, pattern, int(degree), float(interval_ratio)
        nl = len(gh.grids)
        self.dhs = [DofHandler(g, LagrangeCollection(1, dh.ip.ncomp)) for g in gh.grids[:-1]] + [dh]
        self.sps = [allocate_matrix(d) for d in self.dhs[:-1]] + [pattern.sp]
        self.patterns = [d.device_mesh(device).pattern(sp) for d, sp in zip(self.dhs[:-1], self.sps[:-1])] + [pattern]
        self.h = C.c_void_p()
        check(lib().tb_mg_create(device.h, nl, C.byref(self.h)))
        for l, p in enumerate(self.patterns):
            check(lib().tb_mg_set_level(self.h, l, p.h))
        for l in range(1, nl):
            pptr, pidx = gh.parents[l - 1]
            pptr, pidx = np.ascontiguousarray(pptr, dtype=np.int64), np.ascontiguousarray(pidx, dtype=np.int32)
            check(lib().tb_mg_set_transfer(self.h, l, gh.grids[l].n_nodes, pptr.ctypes.data_as(L.c_i64p), pidx.ctypes.data_as(L.c_i32p)))
        self.ch = ch
        if ch is not None:
            check(lib().tb_mg_set_prescribed(self.h, ch.flags(device).ptr))
        self._A = None

    @property
    def n_levels(self):
        return len(self.patterns)

    def setup(self, A):
        """the numeric phase for the matrix values `A` (after apply_zero): Galerkin chain, D⁻¹, λmax per level, coarsest inverse"""
        check(lib().tb_mg_setup(self.h, _ptr(A), self.degree, self.interval_ratio))
        self._A = A                                  # the cycle reads the array: keep it alive
        return self

    def apply(self, r, z):
        check(lib().tb_mg_apply(self.h, _ptr(r), _ptr(z)))
        return z

    def level_matrix(self, level):
        """CSR values of the level's operator on self.sps[level], as a host array"""
        p = C.c_void_p()
        check(lib().tb_mg_level_matrix(self.h, level, C.byref(p)))
        out = np.empty(self.sps[level].nnz)
        check(lib().tb_memcpy_d2h(self.device.h, out.ctypes.data_as(C.c_void_p), p, out.nbytes))
        return out

    def lambda_max(self, level):
        out = C.c_double()
        check(lib().tb_mg_level_lambda_max(self.h, level, C.byref(out)))
        return out.value

    def prolong(self, fine_level, xc, xf):
        check(lib().tb_mg_prolong(self.h, fine_level, _ptr(xc), _ptr(xf)))
        return xf

    def restrict(self, fine_level, rf, rc):
        check(lib().tb_mg_restrict(self.h, fine_level, _ptr(rf), _ptr(rc)))
        return rc

    def solve(self, A, b, x, rtol=1e-5, atol=1e-6, maxiter=1000, setup=True):
        """CG on A x = b preconditioned by one cycle (tb_pcg_solve_mg) → (iterations, residual norm); setup=False reuses the numeric phase"""
        if setup or self._A is None:
            self.setup(A)
        it, res = C.c_int(), C.c_double()
        check(lib().tb_pcg_solve_mg(self.pattern.h, _ptr(A), _ptr(b), _ptr(x), float(rtol), float(atol), int(maxiter), self.h, C.byref(it), C.byref(res)))
        return it.value, res.value

    reuse_setup = False      # set by the Newton loop under simplified_newton: the tangent, and with it the numeric phase, is the previous one

    def tb_mg_solve(self, pattern, A, b, x, rtol, atol, maxiter):
        """what pcg_solve(…, precond=<this>) runs"""
        if pattern is not self.pattern:
            raise ValueError("pcg_solve: the multigrid hierarchy was materialised for another pattern")
        return self.solve(A, b, x, rtol, atol, maxiter, setup=not self.reuse_setup)

    def close(self):
        if self.h:
            lib().tb_mg_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class KrylovMGSolver:
    """KrylovMGSolver(krylov, mg, maxiters): a Krylov method preconditioned by a multigrid (multigrid.jl) — CG; usable as the callable inner_solver of
    NewtonRaphsonSolver ((pattern, J, residual, Δu) → iterations) or through `solve`."""

    def __init__(self, krylov="cg", mg=None, maxiters=None, rtol=1e-8, atol=1e-14):
        if krylov != "cg":
            raise NotImplementedError("KrylovMGSolver(%r): the multigrid preconditions CG only (GMRES is out of scope)" % (krylov,))
        if not isinstance(mg, (GMGPrecon, MultigridHierarchy)):
            raise TypeError("KrylovMGSolver: mg must be a GMGPrecon or a materialised MultigridHierarchy")
        self.mg, self.maxiters, self.rtol, self.atol = mg, maxiters, rtol, atol

    def solve(self, pattern, A, b, x, ch=None):
        mg = self.mg.materialize(pattern, ch) if isinstance(self.mg, GMGPrecon) else self.mg
        return mg.solve(A, b, x, self.rtol, self.atol, self.maxiters if self.maxiters is not None else 1000)

    def __call__(self, pattern, J, b, x):
        return self.solve(pattern, J, b, x)[0]
