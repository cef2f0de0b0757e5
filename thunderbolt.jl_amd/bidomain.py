"""Parabolic–elliptic bidomain electrophysiology: φₑ as an unknown beside φₘ.

The reference declares the model (ParabolicEllipticBidomainModel, src/modeling/electrophysiology.jl:305-326, "Not implemented yet"; the tutorial
ep03_bidomain.jl is a stub), so the discretisation here is this package's: backward Euler on the transformed system of electrophysiology.jl:308-311,

    [ M − Δt Kᵢ      −Δt Kᵢ        ] [φₘ⁺]   [ M φₘ + source_m ]
    [ −Δt Kᵢ         −Δt (Kᵢ + Kₑ) ] [φₑ⁺] = [ source_e        ]

with M the plain mass, Kᵢ and Kₑ the diffusion matrices of κᵢ/(χCₘ) and κₑ/(χCₘ) in the sign of heat_system_matrix (K negative semidefinite).  The
matrix is symmetric positive semidefinite with null vector (0, 1); φₑ is fixed by a ground (vertex ids, as in ecg.py): the φₑ rows and columns of
those dofs are eliminated, the mean diagonal of the φₑφₑ block goes on the eliminated rows, the right-hand side is zeroed there.

The coupled solve runs in csrc/tb_bidomain.hip (tb_bidomain_*): one fused product for all four blocks over a node-interleaved unknown, and conjugate
gradients preconditioned with the inverse 2 × 2 diagonal blocks — or, with `precond=GMGPrecon(gh)`, with one geometric multigrid V-cycle on the node
pairs (csrc/tb_bidomain_mg.hip, tb_bidomain_mg_*: BidomainMultigrid), whose iteration count does not grow with the mesh; on meshes without a
GridHierarchy (tetrahedra, the readers' meshes, the generated ventricle) `precond=BidomainAMGPrecon()` gives the same from the matrix alone: one
smoothed-aggregation V-cycle on the node pairs (csrc/tb_bidomain_amg.hip, tb_bidomain_amg_*: BidomainAlgebraicMultigrid).  BidomainBackwardEulerStage has
the interface of BackwardEulerStage, so it goes into LieTrotterGodunov and ReactionTangentController unchanged."""
import ctypes as C

import numpy as np

from . import _lib as L
from ._lib import check, lib
from .api import (BilinearDiffusionIntegrator, BilinearMassIntegrator, ConductivityToDiffusivityCoefficient, ConstantCoefficient, DeviceVector, DofHandler,
                  LagrangeCollection, LinearIntegrator, _ptr, allocate_matrix, needs_update, setup_operator, solve_converged, update_operator)
from .ecg import _vertex_ids, vertex_dofs
from .amg import AMGPrecon
from .amg import check_supported as amg_check_supported
from .multigrid import ChainedMGPrecon, GMGPrecon, PMGPrecon, check_supported
from .solid import meandiag


class ParabolicEllipticBidomainModel:
    """ParabolicEllipticBidomainModel(χ, Cₘ, κᵢ, κₑ, stim, ion) (src/modeling/electrophysiology.jl:305-326): the reference's fields in the
    reference's order, and the symbols of φₘ, φₑ and the internal state."""

    def __init__(self, chi, Cm, kappa_i, kappa_e, stim, ion, phi_m_symbol="φₘ", phi_e_symbol="φₑ", state_symbol="s"):
        for name, v in (("chi", chi), ("Cm", Cm), ("kappa_i", kappa_i), ("kappa_e", kappa_e)):
            if v is None:
                raise ValueError("ParabolicEllipticBidomainModel: %s is missing" % name)
        self.chi, self.Cm, self.kappa_i, self.kappa_e, self.stim, self.ion = chi, Cm, kappa_i, kappa_e, stim, ion
        self.transmembrane_solution_symbol, self.extracellular_solution_symbol, self.internal_state_symbol = phi_m_symbol, phi_e_symbol, state_symbol

    def diffusivities(self):
        """(Dᵢ, Dₑ) = (κᵢ, κₑ)/(χCₘ), lowered as the monodomain's κ is"""
        return (ConductivityToDiffusivityCoefficient(self.kappa_i, self.Cm, self.chi), ConductivityToDiffusivityCoefficient(self.kappa_e, self.Cm, self.chi))


def check_balanced(values, what="source_e"):
    """An extracellular source whose entries do not sum to zero contradicts the sealed boundary (the ground would absorb the imbalance as a current
    sink): ValueError naming the sum when |Σ| > 1e-10 · Σ|·|."""
    v = np.asarray(values, dtype=np.float64)
    s, a = float(np.sum(v)), float(np.sum(np.abs(v)))
    if not abs(s) <= 1e-10 * a:
        raise ValueError("%s: the extracellular current sums to %.17g (Σ|entries| = %.17g): it has to balance, the boundary is sealed and the ground is "
                         "no current sink" % (what, s, a))


class BidomainSystem:
    """The device block system of one pattern (tb_bidomain_*): set_matrices, apply, solve, pack, unpack on node-interleaved vectors of 2n values."""

    def __init__(self, pattern):
        self.pattern, self.n = pattern, pattern.sp.rowptr.size - 1
        self.h = C.c_void_p()
        check(lib().tb_bidomain_create(pattern.h, C.byref(self.h)))

    def set_matrices(self, M, Ki, Ke, dt, ground_flags, ground_diag, pattern=None):
        check(lib().tb_bidomain_set_matrices(self.h, (pattern or self.pattern).h, _ptr(M), _ptr(Ki), _ptr(Ke), float(dt), _ptr(ground_flags), float(ground_diag)))

    def apply(self, x, y):
        check(lib().tb_bidomain_apply(self.h, _ptr(x), _ptr(y)))

    def solve(self, b, x, rtol=1e-5, atol=1e-6, maxiter=1000, precond=None):
        """(iterations, residual norm).  precond None: block-Jacobi PCG (tb_bidomain_solve); a BidomainMultigrid of this system, set up for the current
        matrices: CG preconditioned by one V-cycle (tb_bidomain_mg_solve); a BidomainAlgebraicMultigrid likewise (tb_bidomain_amg_solve)"""
        it, res = C.c_int(), C.c_double()
        if precond is None:
            check(lib().tb_bidomain_solve(self.h, _ptr(b), _ptr(x), float(rtol), float(atol), int(maxiter), C.byref(it), C.byref(res)))
        elif isinstance(precond, (BidomainMultigrid, BidomainAlgebraicMultigrid)):
            if precond.system is not self:
                raise ValueError("BidomainSystem.solve: the multigrid hierarchy was materialised for another block system")
            solve = lib().tb_bidomain_mg_solve if isinstance(precond, BidomainMultigrid) else lib().tb_bidomain_amg_solve
            check(solve(precond.h, _ptr(b), _ptr(x), float(rtol), float(atol), int(maxiter), C.byref(it), C.byref(res)))
        else:
            raise TypeError("BidomainSystem.solve: precond is None (block-Jacobi), a BidomainMultigrid or a BidomainAlgebraicMultigrid")
        return it.value, res.value

    def pack(self, m, e, out, zero_ground=False):
        check(lib().tb_bidomain_pack(self.h, _ptr(m), _ptr(e) if e is not None else None, int(bool(zero_ground)), _ptr(out)))

    def unpack(self, x, m, e):
        check(lib().tb_bidomain_unpack(self.h, _ptr(x), _ptr(m) if m is not None else None, _ptr(e) if e is not None else None))

    def __del__(self):
        try:
            if self.h:
                lib().tb_bidomain_destroy(self.h)
                self.h = C.c_void_p()
        except Exception:
            pass


class BidomainMultigrid:
    """BidomainMultigrid(system, gh, degree=2, interval_ratio=4.0): the materialised multigrid hierarchy of one BidomainSystem (tb_bidomain_mg_*),
    modelled on MultigridHierarchy — per-level scalar first-order DofHandlers and patterns on the grids of `gh` (finest: the system's own), the tb_mg
    that holds the transfers and the Galerkin term lists (owned here; its numeric phase is never run), and the block hierarchy on top.  `setup()`
    follows every `system.set_matrices`; `apply(r, z)` is one V(degree, degree) cycle on node-interleaved vectors."""

    def __init__(self, system, gh, degree=2, interval_ratio=4.0):
        if not isinstance(system, BidomainSystem):
            raise TypeError("BidomainMultigrid: pass the BidomainSystem the hierarchy preconditions")
        pattern = system.pattern
        dh, device = pattern.dmesh.dh, pattern.dmesh.device
        check_supported(gh, dh)
        self.system, self.gh, self.device, self.degree, self.interval_ratio = system, gh, device, int(degree), float(interval_ratio)
        grids = list(gh.grids)
        self.dhs = [DofHandler(g, LagrangeCollection(1, 1)) for g in grids[:-1]] + [dh]
        self.sps = [allocate_matrix(d) for d in self.dhs[:-1]] + [pattern.sp]
        self.patterns = [d.device_mesh(device).pattern(sp) for d, sp in zip(self.dhs[:-1], self.sps[:-1])] + [pattern]
        self.mg, self.h = C.c_void_p(), C.c_void_p()
        check(lib().tb_mg_create(device.h, len(grids), C.byref(self.mg)))
        for l, p in enumerate(self.patterns):
            check(lib().tb_mg_set_level(self.mg, l, p.h))
        for l in range(1, len(grids)):
            pptr, pidx = gh.parents[l - 1]
            pptr, pidx = np.ascontiguousarray(pptr, dtype=np.int64), np.ascontiguousarray(pidx, dtype=np.int32)
            check(lib().tb_mg_set_transfer(self.mg, l, grids[l].n_nodes, pptr.ctypes.data_as(L.c_i64p), pidx.ctypes.data_as(L.c_i32p)))
        check(lib().tb_bidomain_mg_create(system.h, self.mg, C.byref(self.h)))

    @property
    def n_levels(self):
        return len(self.patterns)

    def setup(self):
        """the numeric phase for the matrices of the latest system.set_matrices: Galerkin chain, block inverses, λmax per level, coarsest inverse"""
        check(lib().tb_bidomain_mg_setup(self.h, self.degree, self.interval_ratio))
        return self

    def apply(self, r, z):
        check(lib().tb_bidomain_mg_apply(self.h, _ptr(r), _ptr(z)))
        return z

    def level_blocks(self, level):
        """(a₁₁, a₁₂, a₂₁, a₂₂) of the level's operator: CSR values on self.sps[level], host arrays"""
        p, nnz = C.c_void_p(), C.c_int64()
        check(lib().tb_bidomain_mg_level_planes(self.h, level, C.byref(p), C.byref(nnz)))
        out = np.empty((4, nnz.value))
        check(lib().tb_memcpy_d2h(self.device.h, out.ctypes.data_as(C.c_void_p), p, out.nbytes))
        return tuple(out)

    def lambda_max(self, level):
        out = C.c_double()
        check(lib().tb_bidomain_mg_level_lambda_max(self.h, level, C.byref(out)))
        return out.value

    def cycle_below(self, level):
        """measurement hook: the cycle from `level` (below the finest) down on that level's own buffers, whatever they hold (enqueues only) — its
        duration is the coarse tail of a cycle, its result means nothing"""
        check(lib().tb_bidomain_mg_cycle_below(self.h, level))

    def close(self):
        if self.h:
            lib().tb_bidomain_mg_destroy(self.h)
            self.h = None
        if self.mg:
            lib().tb_mg_destroy(self.mg)
            self.mg = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BidomainAMGPrecon:
    """BidomainAMGPrecon(theta=0.25, degree=2, interval_ratio=4.0, max_coarse=128, max_levels=16): the recipe of the algebraic block cycle — AMGPrecon's
    arguments with nodes in the place of dofs.  The last level is inverted densely: at most 512 nodes (1 024 unknowns); the default of 128 keeps the
    one-workgroup dense inverse from dominating the numeric set-up."""

    def __init__(self, theta=0.25, degree=2, interval_ratio=4.0, max_coarse=128, max_levels=16, cycle="V", smoother="chebyshev", near_nullspace=None):
        if near_nullspace is not None:
            raise NotImplementedError("BidomainAMGPrecon: a near_nullspace is out of scope for the block system (its fields are scalar: the constant is their near-null space)")
        if cycle != "V":
            raise NotImplementedError("BidomainAMGPrecon: V-cycles only (W- and F-cycles are out of scope)")
        if smoother != "chebyshev":
            raise NotImplementedError("BidomainAMGPrecon: the Chebyshev smoother on the 2 x 2 node blocks only")
        self.theta, self.degree, self.interval_ratio = float(theta), int(degree), float(interval_ratio)
        self.max_coarse, self.max_levels = int(max_coarse), int(max_levels)

    def check(self, dh):
        amg_check_supported(dh)
        if dh.ip.order != 1 or dh.ip.ncomp != 1:
            raise NotImplementedError("BidomainAMGPrecon: first-order scalar fields only (order %d, %d component(s))" % (dh.ip.order, dh.ip.ncomp))

    def materialize(self, system):
        return BidomainAlgebraicMultigrid(system, self.theta, self.degree, self.interval_ratio, self.max_coarse, self.max_levels)


class BidomainAlgebraicMultigrid:
    """BidomainAlgebraicMultigrid(system, theta=0.25, degree=2, interval_ratio=4.0, max_coarse=128, max_levels=16): the materialised smoothed-aggregation
    hierarchy of one BidomainSystem (tb_bidomain_amg_*).  Level 0 is the block system, level l + 1 the Galerkin operator of level l's aggregates (found on
    the φₑφₑ plane, one scalar prolongator for both unknowns).  `setup()` follows every `system.set_matrices`: the first one plans, every later one
    redoes the numeric phase on the same aggregates; `replan()` drops the plan.  `setups` and `aggregations` are the library's own counts
    (tb_bidomain_amg_counts): successful set-ups, and host aggregation runs — one per level planned, none in a numeric-only set-up.  `apply(r, z)` is one
    V(degree, degree) cycle on node-interleaved vectors."""

    def __init__(self, system, theta=0.25, degree=2, interval_ratio=4.0, max_coarse=128, max_levels=16):
        if not isinstance(system, BidomainSystem):
            raise TypeError("BidomainAlgebraicMultigrid: pass the BidomainSystem the hierarchy preconditions")
        self.system, self.device, self.degree, self.interval_ratio = system, system.pattern.dmesh.device, int(degree), float(interval_ratio)
        self.h = C.c_void_p()
        check(lib().tb_bidomain_amg_create(system.h, float(theta), int(max_coarse), int(max_levels), C.byref(self.h)))

    def setup(self):
        """plan (first call) and numeric phase for the matrices of the latest system.set_matrices"""
        check(lib().tb_bidomain_amg_setup(self.h, self.degree, self.interval_ratio))
        return self

    def replan(self):
        check(lib().tb_bidomain_amg_replan(self.h))
        return self

    def _counts(self):
        s, a = C.c_int64(), C.c_int64()
        check(lib().tb_bidomain_amg_counts(self.h, C.byref(s), C.byref(a)))
        return s.value, a.value

    @property
    def setups(self):
        return self._counts()[0]

    @property
    def aggregations(self):
        return self._counts()[1]

    def apply(self, r, z):
        check(lib().tb_bidomain_amg_apply(self.h, _ptr(r), _ptr(z)))
        return z

    @property
    def n_levels(self):
        n = C.c_int()
        check(lib().tb_bidomain_amg_n_levels(self.h, C.byref(n)))
        return n.value

    def level_size(self, level):
        """(nodes, non-zeros of the scalar pattern, aggregates) of a level; the last level has no aggregates"""
        n, nnz, na = C.c_int64(), C.c_int64(), C.c_int64()
        check(lib().tb_bidomain_amg_level_size(self.h, level, C.byref(n), C.byref(nnz), C.byref(na)))
        return n.value, nnz.value, na.value

    def level_pattern(self, level):
        """(rowptr, colidx) of the level's scalar pattern"""
        n, nnz, _ = self.level_size(level)
        ptr, col = np.empty(n + 1, dtype=np.int64), np.empty(nnz, dtype=np.int32)
        check(lib().tb_bidomain_amg_level_csr(self.h, level, ptr.ctypes.data_as(L.c_i64p), col.ctypes.data_as(L.c_i32p)))
        return ptr, col

    def level_blocks(self, level):
        """(a₁₁, a₁₂, a₂₁, a₂₂) of the level's operator: CSR values on level_pattern(level), host arrays"""
        out = np.empty((4, self.level_size(level)[1]))
        check(lib().tb_bidomain_amg_level_planes(self.h, level, *(out[q].ctypes.data_as(L.c_dp) for q in range(4))))
        return tuple(out)

    def prolongator(self, level):
        """the scalar P from level + 1 to level as a scipy.sparse.csr_matrix (the block transfer is P ⊗ I₂)"""
        import scipy.sparse as sparse
        n, _, na = self.level_size(level)
        nnz = C.c_int64()
        check(lib().tb_bidomain_amg_level_prolongator(self.h, level, C.byref(nnz), None, None, None))
        ptr, col, val = np.empty(n + 1, dtype=np.int64), np.empty(nnz.value, dtype=np.int32), np.empty(nnz.value)
        check(lib().tb_bidomain_amg_level_prolongator(self.h, level, None, ptr.ctypes.data_as(L.c_i64p), col.ctypes.data_as(L.c_i32p), val.ctypes.data_as(L.c_dp)))
        return sparse.csr_matrix((val, col, ptr), shape=(n, na))

    def aggregates(self, level):
        """the aggregate of every node of the level (−1: outside every aggregate, as every grounded node is)"""
        out = np.empty(self.level_size(level)[0], dtype=np.int32)
        check(lib().tb_bidomain_amg_level_aggregates(self.h, level, out.ctypes.data_as(L.c_i32p)))
        return out

    def lambda_max(self, level):
        """the estimate of λmax(B⁻¹𝒜) the level's smoother runs on"""
        out = C.c_double()
        check(lib().tb_bidomain_amg_level_lambda_max(self.h, level, C.byref(out)))
        return out.value

    def products(self, level, fused=True):
        """measurement hook: the Galerkin products between `level` and the level below once more (enqueues only) — fused: the two three-plane launches
        of the set-up; otherwise three launch pairs of the scalar product kernel, one plane each.  The planes keep their bits either way."""
        check(lib().tb_bidomain_amg_products(self.h, int(level), int(bool(fused))))

    def close(self):
        if self.h:
            lib().tb_bidomain_amg_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BidomainBackwardEulerStage:
    """BackwardEulerStage for the bidomain block system: perform_step(φₘ, t, Δt) advances φₘ in place and the stage's own `phi_e` (n values, zero at
    the start, the initial guess of the next step).  `ground`: vertex ids (or positions), mandatory.  `source`: the transmembrane stimulus, a
    LinearIntegrator scaled as BackwardEulerStage scales its source.  `source_e`: the extracellular current Iₛₜᵢₘ,ₑ − Iₛₜᵢₘ,ᵢ, a LinearIntegrator or
    nodal currents by dof (array of n values); it has to sum to zero (checked whenever it is (re)assembled).  The combined operator is rebuilt only
    when Δt changes (`generation` counts the rebuilds).  `solver.mirror` has no meaning here.  `precond` (keyword only): None — block-Jacobi PCG — or
    GMGPrecon(gh) with gh's finest grid the stage's, or BidomainAMGPrecon(...) on any mesh: the hierarchy is materialised here (`multigrid`, a
    BidomainMultigrid or a BidomainAlgebraicMultigrid) and set up again with every rebuild of the operator (the algebraic one keeps its aggregates)."""

    def __init__(self, solver, strategy, dh, diffusion_i, diffusion_e, ground, source=None, source_e=None, pattern=None, t0=0.0, *, precond=None):
        if dh.ip.order != 1 or dh.ip.ncomp != 1:
            raise NotImplementedError("BidomainBackwardEulerStage: first-order scalar fields only (order %d, %d component(s))" % (dh.ip.order, dh.ip.ncomp))
        if precond is not None:
            if isinstance(precond, (PMGPrecon, ChainedMGPrecon)):
                raise NotImplementedError("BidomainBackwardEulerStage: %s is out of scope - the block system is first order, pass GMGPrecon(gh)" % type(precond).__name__)
            if isinstance(precond, AMGPrecon):
                raise NotImplementedError("BidomainBackwardEulerStage: the scalar AMGPrecon is out of scope for the block system - pass BidomainAMGPrecon(...)")
            if getattr(getattr(precond, "coarse", None), "near_nullspace", None) is not None:
                raise NotImplementedError("BidomainBackwardEulerStage: a near_nullspace is out of scope for the block system (its fields are scalar)")
            if not isinstance(precond, (GMGPrecon, BidomainAMGPrecon)):
                raise NotImplementedError("BidomainBackwardEulerStage: precond is None (block-Jacobi) or GMGPrecon(gh); %r is out of scope" % (precond,))
            precond.check(dh)
        if ground is None or len(ground) == 0:
            raise ValueError("BidomainBackwardEulerStage: `ground` is empty - without a grounded vertex φₑ is determined up to a constant only and the "
                             "block matrix is singular")
        self.solver, self.device, self.dh = solver, strategy.device, dh
        self.sp = pattern or allocate_matrix(dh)
        n = dh.ndofs
        self.M = update_operator(setup_operator(strategy, BilinearMassIntegrator(ConstantCoefficient(1.0)), dh, self.sp), t0)
        self.Ki = update_operator(setup_operator(strategy, BilinearDiffusionIntegrator(diffusion_i), dh, self.sp), t0)
        self.Ke = update_operator(setup_operator(strategy, BilinearDiffusionIntegrator(diffusion_e), dh, self.sp), t0)
        self.ground_dofs = np.unique(vertex_dofs(dh)[_vertex_ids(ground, dh.grid)])
        flags = np.zeros(n, dtype=np.uint8)
        flags[self.ground_dofs] = 1
        self.ground_flags = self.device.to_device(flags)
        self.source = None if source is None else update_operator(setup_operator(strategy, source, dh), t0)
        self.source_e = None
        if source_e is not None:
            if isinstance(source_e, LinearIntegrator):
                self.source_e = update_operator(setup_operator(strategy, source_e, dh), t0)
                self.source_e_b = self.source_e.b
                check_balanced(self.source_e_b.to_host())
            else:
                v = np.ascontiguousarray(np.asarray(source_e, dtype=np.float64).ravel())
                if v.size != n:
                    raise ValueError("source_e: %d nodal currents for %d dofs" % (v.size, n))
                check_balanced(v)
                self.source_e_b = self.device.to_device(v)
        else:
            self.source_e_b = None
        self.system = BidomainSystem(self.M.pattern)
        if isinstance(precond, BidomainAMGPrecon):
            self.multigrid = precond.materialize(self.system)
        else:
            self.multigrid = None if precond is None else BidomainMultigrid(self.system, precond.gh, precond.degree, precond.interval_ratio)
        # the mean diagonal of Kᵢ + Kₑ does not depend on Δt: read once (tb_meandiag is Ferrite's: the mean of |dᵢᵢ|, and K's diagonal is negative)
        self._kdiag = meandiag(self.Ki.pattern, self.Ki.A) + meandiag(self.Ke.pattern, self.Ke.A)
        self.phi_e = self.device.zeros(n)
        self.b = DeviceVector(self.device, n)
        self.rhs = DeviceVector(self.device, 2 * n)
        self.x = DeviceVector(self.device, 2 * n)
        self.dt_last = None
        self.last_iters = 0
        self.generation = 0

    def ground_diag(self, dt):
        return float(dt) * self._kdiag

    def perform_step(self, phi, t, dt):
        """One backward-Euler step of the block system: True on success."""
        if self.dt_last is None or abs(dt - self.dt_last) > 1e-14 * abs(dt):
            self.system.set_matrices(self.M.A, self.Ki.A, self.Ke.A, dt, self.ground_flags, self.ground_diag(dt))
            if self.multigrid is not None:
                self.multigrid.setup()
            self.dt_last = dt
            self.generation += 1
        check(lib().tb_spmv_csr(self.M.pattern.h, self.M.A.ptr, _ptr(phi), 1.0, 0.0, self.b.ptr))          # M φₘ
        if self.source is not None:
            if needs_update(self.source, t + dt):
                update_operator(self.source, t + dt)
            check(lib().tb_axpy(self.device.h, self.b.n, 1.0, self.source.b.ptr, self.b.ptr))
        if self.source_e is not None and needs_update(self.source_e, t + dt):
            update_operator(self.source_e, t + dt)
            check_balanced(self.source_e_b.to_host())
        self.system.pack(self.b, self.source_e_b, self.rhs, zero_ground=True)
        self.system.pack(phi, self.phi_e, self.x)
        its, res = self.system.solve(self.rhs, self.x, self.solver.rtol, self.solver.atol, self.solver.maxiter, precond=self.multigrid)
        self.system.unpack(self.x, phi, self.phi_e)
        self.last_iters, self.last_resnorm = its, res
        return solve_converged(self.M.pattern, res)
