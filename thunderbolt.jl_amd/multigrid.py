"""Multigrid preconditioner on hexahedral grids — GMGPrecon, PMGPrecon, ChainedMGPrecon and KrylovMGSolver of the reference's multigrid extension
(src/solver/linear/multigrid.jl, ext/ThunderboltFerriteMultigridExt.jl, docs/src/literate-howto/multigrid.jl) over tb_mg_* of libtbhip.so: Galerkin
coarse operators rebuilt from every new matrix, one V(degree, degree) cycle with a Chebyshev–Jacobi smoother, an explicit coarsest inverse.

Covered: h-levels of first-order hexahedra on the nested grids of a GridHierarchy (GMGPrecon); one p-level from a second-order field to the first-order
field on the same grid (PMGPrecon), alone or on top of the h-levels (ChainedMGPrecon); one field of 1 or 3 components on the whole grid; CG, and restarted GMRES with the
cycle as a fixed right preconditioner (gmres_solve(…, precond=…), KrylovMGSolver(KrylovGMRES(restart), mg), NewtonRaphsonSolver(inner_solver="gmres",
inner_precond=…)) for MILDLY non-symmetric matrices with a positive diagonal: the hierarchy then runs in general mode, whose coarsest inverse is
pivoted and not symmetrised (the point-Jacobi Chebyshev smoother breaks down when the skew part is as large as the symmetric one).  One hierarchy
serves one kind of solve cheaply: CG after GMRES on it, or the other way round, flips the mode and sets up again.  Refused with a message: orders
above 2, tetrahedra, W- and F-cycles, other smoothers, hierarchies over several ranks, subdomain dof handlers."""
import ctypes as C

import numpy as np

from . import _lib as L
from ._lib import check, lib
from .amg import AlgebraicHierarchy, AMGPrecon, resolve_near_nullspace
from .api import DofHandler, Hexahedron, LagrangeCollection, _ptr, allocate_matrix
from .meshgen import GridHierarchy


class GMGPrecon:
    """GMGPrecon(gh, degree=2, interval_ratio=4.0): the recipe — a grid hierarchy whose finest grid carries the problem, the degree of the smoothing
    polynomial and the ratio λmax/λmin of its interval.  `materialize(pattern, ch)` builds the device hierarchy for one matrix pattern; pcg_solve and
    the Newton solver do that themselves at their first solve."""

    def __init__(self, gh, degree=2, interval_ratio=4.0, cycle="V", smoother="chebyshev", coarse=None):
        if not isinstance(gh, GridHierarchy):
            raise TypeError("GMGPrecon: pass a GridHierarchy")
        _check_cycle("GMGPrecon", cycle, smoother)
        self.gh, self.degree, self.interval_ratio = gh, int(degree), float(interval_ratio)
        self.coarse = _check_coarse("GMGPrecon", coarse, self.degree, self.interval_ratio)   # AMGPrecon: one AMG cycle solves the coarsest grid
        self._materialized = {}

    def check(self, dh):
        check_supported(self.gh, dh)

    def materialize(self, pattern, ch=None):
        key = (id(pattern), id(ch))
        if key not in self._materialized:
            self._materialized[key] = (MultigridHierarchy(pattern, self.gh, self.degree, self.interval_ratio, ch, coarse=self.coarse), pattern, ch)   # (the key's objects stay alive)
        return self._materialized[key][0]


def _check_coarse(who, coarse, degree, interval_ratio):
    """the coarse solver of a hierarchy: None (dense inverse) or an AMGPrecon of the hierarchy's degree and interval ratio (the cycle has one for all levels)"""
    if coarse is None:
        return None
    if not isinstance(coarse, AMGPrecon):
        raise TypeError("%s: coarse is None (dense inverse) or an AMGPrecon" % who)
    if coarse.degree != degree or coarse.interval_ratio != interval_ratio:
        raise ValueError("%s: the recipes disagree on degree or interval_ratio (%d, %g and %d, %g); the cycle has one for all levels"
                         % (who, degree, interval_ratio, coarse.degree, coarse.interval_ratio))
    return coarse


def _check_cycle(who, cycle, smoother):
    if cycle != "V":
        raise NotImplementedError("%s: V-cycles only (W- and F-cycles are out of scope)" % who)
    if smoother != "chebyshev":
        raise NotImplementedError("%s: the Chebyshev-Jacobi smoother only" % who)


class PMGPrecon:
    """PMGPrecon(degree=2, interval_ratio=4.0): the recipe of polynomial multigrid — a second-order field over the first-order field on the same grid.
    Keyword-only, no grid hierarchy.  Alone it materialises two levels with the dense inverse on the first-order one (at most 1 024 first-order dofs);
    ChainedMGPrecon puts the h-levels of a GMGPrecon below."""

    def __init__(self, *args, degree=2, interval_ratio=4.0, cycle="V", smoother="chebyshev"):
        if args:
            raise NotImplementedError("PMGPrecon takes keywords only (degree, interval_ratio): p-levels need no grid hierarchy.  For h-levels below the "
                                      "p-level pass ChainedMGPrecon(PMGPrecon(), GMGPrecon(gh))")
        _check_cycle("PMGPrecon", cycle, smoother)
        self.degree, self.interval_ratio = int(degree), float(interval_ratio)
        self._materialized = {}

    gh = None      # no h-levels (ChainedMGPrecon sets the hierarchy of its GMGPrecon)
    coarse = None  # dense inverse on the coarsest level (ChainedMGPrecon(PMGPrecon(), AMGPrecon()): one AMG cycle)

    def check(self, dh):
        check_supported(self.gh, dh, order=2, who=type(self).__name__)

    def materialize(self, pattern, ch=None):
        key = (id(pattern), id(ch))
        if key not in self._materialized:
            self._materialized[key] = (MultigridHierarchy(pattern, self.gh, self.degree, self.interval_ratio, ch, p_level=True, coarse=self.coarse), pattern, ch)
        return self._materialized[key][0]


class ChainedMGPrecon(PMGPrecon):
    """ChainedMGPrecon(pmg, gmg): polynomial multigrid on the fine level with the geometric multigrid of `gmg` as its coarse solver — the h-levels of
    gmg.gh with first-order fields, the caller's second-order field on gmg.gh.grids[-1] on top.  One degree and interval ratio serve all levels."""

    def __init__(self, *args):
        if len(args) != 2 or isinstance(args[0], GridHierarchy):
            raise NotImplementedError("ChainedMGPrecon takes the two recipes it chains, not a grid hierarchy: ChainedMGPrecon(PMGPrecon(), GMGPrecon(gh)) "
                                      "(p-levels on top of the h-levels of gh)")
        pmg, gmg = args
        if type(pmg) is PMGPrecon and isinstance(gmg, AMGPrecon):
            # the reference's default pcoarse_solver (multigrid.jl:27): the first-order level is solved by one AMG cycle, no h-levels
            self.pmg, self.gmg, self.gh = pmg, None, None
            self.degree, self.interval_ratio = pmg.degree, pmg.interval_ratio
            self.coarse = _check_coarse("ChainedMGPrecon", gmg, self.degree, self.interval_ratio)
            self._materialized = {}
            return
        if not (type(pmg) is PMGPrecon and isinstance(gmg, GMGPrecon)):
            raise TypeError("ChainedMGPrecon(pmg, gmg): a PMGPrecon and a GMGPrecon or an AMGPrecon, in this order")
        if pmg.degree != gmg.degree:
            raise ValueError("ChainedMGPrecon: the recipes disagree on degree (%d and %d); the cycle has one for all levels" % (pmg.degree, gmg.degree))
        if pmg.interval_ratio != gmg.interval_ratio:
            raise ValueError("ChainedMGPrecon: the recipes disagree on interval_ratio (%g and %g); the cycle has one for all levels" % (pmg.interval_ratio, gmg.interval_ratio))
        self.pmg, self.gmg, self.gh = pmg, gmg, gmg.gh
        self.degree, self.interval_ratio = pmg.degree, pmg.interval_ratio
        self.coarse = gmg.coarse
        self._materialized = {}


def check_supported(gh, dh, order=1, who="GMGPrecon"):
    """what the multigrid covers, checked on the host: raises for a DofHandler the hierarchy cannot serve (gh None: a p-level alone)"""
    if dh.grid.cell_kind != Hexahedron:
        raise NotImplementedError("%s: hexahedral grids only (there is no tetrahedral uniform_refinement)" % who)
    if order == 1 and dh.ip.order != 1:
        raise NotImplementedError("GMGPrecon: first-order fields only (a second-order field takes ChainedMGPrecon(PMGPrecon(), GMGPrecon(gh)))")
    if order == 2 and dh.ip.order != 2:
        raise NotImplementedError("%s: a field of order 2 only (order %d given; first-order fields take GMGPrecon, orders above 2 are out of scope)" % (who, dh.ip.order))
    if gh is None:
        return
    fine = gh.grids[-1]
    if dh.grid is not fine and not (dh.grid.conn.shape == fine.conn.shape and np.array_equal(dh.grid.conn, fine.conn) and np.array_equal(dh.grid.xyz, fine.xyz)):
        raise ValueError("%s: the finest grid of the hierarchy is not the grid of the matrix's DofHandler" % who)
    if dh.cell_dofs.shape[0] != fine.n_cells:
        raise NotImplementedError("%s: subdomain dof handlers are out of scope" % who)


class MultigridHierarchy:
    """A materialised GMGPrecon, PMGPrecon or ChainedMGPrecon: per-level DofHandlers with the fine handler's components, their patterns, the transfer
    and Galerkin plans (tb_mg).  `pattern`: the DevicePattern of the system matrix on gh.grids[-1]; `ch`: its ConstraintHandler (None: no Dirichlet
    dofs).  p_level: the matrix's field is second order; the level below it is the first-order field on the same grid, the h-levels of `gh` (None: no
    h-levels) follow below that."""

    def __init__(self, pattern, gh, degree=2, interval_ratio=4.0, ch=None, p_level=False, coarse=None):
        dh, device = pattern.dmesh.dh, pattern.dmesh.device
        check_supported(gh, dh, order=2 if p_level else 1, who="ChainedMGPrecon" if p_level and gh is not None else "PMGPrecon" if p_level else "GMGPrecon")
        self.device, self.gh, self.pattern, self.degree, self.interval_ratio = device, gh, pattern, int(degree), float(interval_ratio)
        self.p_level = bool(p_level)
        grids = [dh.grid] if gh is None else list(gh.grids)
        nl = len(grids) + (1 if p_level else 0)
        self.dhs = [DofHandler(g, LagrangeCollection(1, dh.ip.ncomp)) for g in (grids if p_level else grids[:-1])] + [dh]
        self.sps = [allocate_matrix(d) for d in self.dhs[:-1]] + [pattern.sp]
        self.patterns = [d.device_mesh(device).pattern(sp) for d, sp in zip(self.dhs[:-1], self.sps[:-1])] + [pattern]
        self.h = C.c_void_p()
        check(lib().tb_mg_create(device.h, nl, C.byref(self.h)))
        for l, p in enumerate(self.patterns):
            check(lib().tb_mg_set_level(self.h, l, p.h))
        if p_level:
            check(lib().tb_mg_set_p_transfer(self.h, nl - 1))
        for l in range(1, len(grids)):
            pptr, pidx = gh.parents[l - 1]
            pptr, pidx = np.ascontiguousarray(pptr, dtype=np.int64), np.ascontiguousarray(pidx, dtype=np.int32)
            check(lib().tb_mg_set_transfer(self.h, l, grids[l].n_nodes, pptr.ctypes.data_as(L.c_i64p), pidx.ctypes.data_as(L.c_i32p)))
        self.ch = ch
        if ch is not None:
            check(lib().tb_mg_set_prescribed(self.h, ch.flags(device).ptr))
        self.coarse = coarse
        if coarse is not None:
            check(lib().tb_mg_set_coarse_amg(self.h, coarse.theta, coarse.max_coarse, coarse.max_levels))
            nns = resolve_near_nullspace(coarse.near_nullspace, self.dhs[0])     # the AMG sits on the first-order level 0, whose coordinates are its grid's
            if nns is not None:
                n_nodes, node, B = nns
                check(lib().tb_mg_set_coarse_amg_near_nullspace(self.h, n_nodes, node.ctypes.data_as(L.c_i32p), B.shape[1], B.ctypes.data_as(L.c_dp)))
        self._A = None

    @property
    def n_levels(self):
        return len(self.patterns)

    general = False          # set_general: the matrix need not be symmetric (pivoted coarsest inverse, nothing symmetrised)
    n_setups = 0             # numeric set-ups so far

    def set_general(self, general):
        """general mode on or off (tb_mg_set_general; it reaches the AMG of coarse=AMGPrecon(…) too); a change drops the numeric phase, so the next
        solve or `setup` redoes it"""
        general = bool(general)
        if general != self.general:
            check(lib().tb_mg_set_general(self.h, int(general)))
            self.general = general
            self._A = None
        return self

    def setup(self, A):
        """the numeric phase for the matrix values `A` (after apply_zero): Galerkin chain, D⁻¹, λmax per level, coarsest inverse"""
        check(lib().tb_mg_setup(self.h, _ptr(A), self.degree, self.interval_ratio))
        self._A = A                                  # the cycle reads the array: keep it alive
        self.n_setups += 1
        return self

    def apply(self, r, z):
        check(lib().tb_mg_apply(self.h, _ptr(r), _ptr(z)))
        return z

    def coarse_hierarchy(self):
        """the AMG hierarchy below level 0 (coarse=AMGPrecon(…), after one setup) as an AlgebraicHierarchy to inspect; this object keeps owning it.  The
        view is taken afresh at every call: its `general` is this hierarchy's mode and its `n_setups` this hierarchy's count at that moment (every set-up
        of this hierarchy sets the AMG up too), and the mode is changed through this hierarchy's set_general only — the view's refuses"""
        h = C.c_void_p()
        check(lib().tb_mg_coarse_amg(self.h, C.byref(h)))
        if not h:
            return None
        view = AlgebraicHierarchy.__new__(AlgebraicHierarchy)
        view.device, view.pattern, view.degree, view.interval_ratio, view.h, view._A, view.owner = self.device, self.patterns[0], self.degree, self.interval_ratio, h, None, self
        view.close = lambda: None
        view.general, view.n_setups = self.general, self.n_setups

        def refuse(general):
            raise RuntimeError("the AMG below level 0 takes its mode from the hierarchy that owns it: call set_general on the MultigridHierarchy")
        view.set_general = refuse
        view.k = 0 if self.coarse is None or self.coarse.near_nullspace is None else 6 if isinstance(self.coarse.near_nullspace, str) else np.shape(self.coarse.near_nullspace)[1]
        return view

    def level_matrix(self, level):
        """CSR values of the level's operator on self.sps[level], as a host array"""
        p = C.c_void_p()
        check(lib().tb_mg_level_matrix(self.h, level, C.byref(p)))
        out = np.empty(self.sps[level].nnz)
        check(lib().tb_memcpy_d2h(self.device.h, out.ctypes.data_as(C.c_void_p), p, out.nbytes))
        return out

    def plan(self, level):
        """(blocked, n_terms) of the Galerkin plan between `level` and the level below (after one setup): blocked — one 4-byte term per pair of
        3 × 3 blocks instead of one per pair of non-zeros"""
        blocked, n = C.c_int(), C.c_int64()
        check(lib().tb_mg_level_plan(self.h, level, C.byref(blocked), C.byref(n)))
        return bool(blocked.value), n.value

    def galerkin(self, level):
        """the product below `level` alone, as the latest setup computed it (enqueues only): what a measurement of the Galerkin kernels times"""
        check(lib().tb_mg_galerkin(self.h, level))

    def plan_bytes(self, level):
        """device bytes of that plan: the terms, the pointer per coarse non-zero (block) and, blocked, the block-row tables of the two patterns"""
        blocked, n = self.plan(level)
        per = 9 if blocked else 1
        extra = 4 * (self.sps[level].nnz + self.sps[level - 1].nnz) // 9 if blocked else 0
        return 4 * n + 8 * (self.sps[level - 1].nnz // per + 1) + extra

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
        self.set_general(False)
        if setup or self._A is None:
            self.setup(A)
        it, res = C.c_int(), C.c_double()
        check(lib().tb_pcg_solve_mg(self.pattern.h, _ptr(A), _ptr(b), _ptr(x), float(rtol), float(atol), int(maxiter), self.h, C.byref(it), C.byref(res)))
        return it.value, res.value

    def solve_gmres(self, A, b, x, rtol=1e-5, atol=1e-6, maxiter=1000, restart=50, setup=True, general=True):
        """GMRES(restart) on A x = b with one cycle as the fixed right preconditioner (tb_gmres_solve_mg) → (Arnoldi steps, residual norm).  The
        hierarchy goes to general mode first (general=False keeps the symmetrised coarsest inverse: for measurements); setup=False reuses the
        numeric phase unless the mode changed"""
        self.set_general(general)
        if setup or self._A is None:
            self.setup(A)
        it, res = C.c_int(), C.c_double()
        check(lib().tb_gmres_solve_mg(self.pattern.h, _ptr(A), _ptr(b), _ptr(x), float(rtol), float(atol), int(maxiter), int(restart), self.h, C.byref(it),
                                      C.byref(res)))
        return it.value, res.value

    reuse_setup = False      # set by the Newton loop under simplified_newton: the tangent, and with it the numeric phase, is the previous one

    def tb_mg_solve(self, pattern, A, b, x, rtol, atol, maxiter):
        """what pcg_solve(…, precond=<this>) runs"""
        if pattern is not self.pattern:
            raise ValueError("pcg_solve: the multigrid hierarchy was materialised for another pattern")
        return self.solve(A, b, x, rtol, atol, maxiter, setup=not self.reuse_setup)

    def tb_mg_gmres_solve(self, pattern, A, b, x, rtol, atol, maxiter, restart):
        """what gmres_solve(…, precond=<this>) runs"""
        if pattern is not self.pattern:
            raise ValueError("gmres_solve: the multigrid hierarchy was materialised for another pattern")
        return self.solve_gmres(A, b, x, rtol, atol, maxiter, restart, setup=not self.reuse_setup)

    def close(self):
        if self.h:
            lib().tb_mg_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class KrylovGMRES:
    """KrylovGMRES(restart=50): restarted GMRES as the Krylov method of a KrylovMGSolver — the reference's KrylovJL_GMRES(gmres_restart = …), the
    default of its KrylovMGSolver (multigrid.jl:114-115, there with a restart of 400)."""

    def __init__(self, restart=50):
        if int(restart) < 1:
            raise ValueError("KrylovGMRES: restart must be at least 1 (got %r)" % (restart,))
        self.restart = int(restart)

    def __repr__(self):
        return "KrylovGMRES(restart=%d)" % self.restart


class KrylovMGSolver:
    """KrylovMGSolver(krylov, mg, maxiters): a Krylov method preconditioned by a multigrid (multigrid.jl) — "cg", or KrylovGMRES(restart) for matrices
    that are not symmetric (the hierarchy then runs in general mode); usable as the callable inner_solver of NewtonRaphsonSolver ((pattern, J,
    residual, Δu) → iterations) or through `solve`."""

    def __init__(self, krylov="cg", mg=None, maxiters=None, rtol=1e-8, atol=1e-14):
        if not isinstance(krylov, KrylovGMRES) and krylov != "cg":
            raise NotImplementedError("KrylovMGSolver(%r): the Krylov method is \"cg\" or a tb.KrylovGMRES(restart=...) object (GMRES takes its restart "
                                      "length from there; the bare string is not accepted)" % (krylov,))
        if not isinstance(mg, (GMGPrecon, PMGPrecon, MultigridHierarchy, AMGPrecon, AlgebraicHierarchy)):
            raise TypeError("KrylovMGSolver: mg must be a GMGPrecon, a PMGPrecon, a ChainedMGPrecon, an AMGPrecon or a materialised hierarchy")
        self.krylov, self.mg, self.maxiters, self.rtol, self.atol = krylov, mg, maxiters, rtol, atol

    def solve(self, pattern, A, b, x, ch=None):
        mg = self.mg.materialize(pattern, ch) if hasattr(self.mg, "materialize") else self.mg
        maxiter = self.maxiters if self.maxiters is not None else 1000
        if isinstance(self.krylov, KrylovGMRES):
            return mg.solve_gmres(A, b, x, self.rtol, self.atol, maxiter, self.krylov.restart)
        return mg.solve(A, b, x, self.rtol, self.atol, maxiter)

    def __call__(self, pattern, J, b, x):
        return self.solve(pattern, J, b, x)[0]
