"""Parabolic–elliptic bidomain electrophysiology: φₑ as an unknown beside φₘ.

The reference declares the model (ParabolicEllipticBidomainModel, src/modeling/electrophysiology.jl:305-326, "Not implemented yet"; the tutorial
ep03_bidomain.jl is a stub), so the discretisation here is this package's: backward Euler on the transformed system of electrophysiology.jl:308-311,

    [ M − Δt Kᵢ      −Δt Kᵢ        ] [φₘ⁺]   [ M φₘ + source_m ]
    [ −Δt Kᵢ         −Δt (Kᵢ + Kₑ) ] [φₑ⁺] = [ source_e        ]

with M the plain mass, Kᵢ and Kₑ the diffusion matrices of κᵢ/(χCₘ) and κₑ/(χCₘ) in the sign of heat_system_matrix (K negative semidefinite).  The
matrix is symmetric positive semidefinite with null vector (0, 1); φₑ is fixed by a ground (vertex ids, as in ecg.py): the φₑ rows and columns of
those dofs are eliminated, the mean diagonal of the φₑφₑ block goes on the eliminated rows, the right-hand side is zeroed there.

The coupled solve runs in csrc/tb_bidomain.hip (tb_bidomain_*): one fused product for all four blocks over a node-interleaved unknown, and conjugate
gradients preconditioned with the inverse 2 × 2 diagonal blocks.  BidomainBackwardEulerStage has the interface of BackwardEulerStage, so it goes into
LieTrotterGodunov and ReactionTangentController unchanged."""
import ctypes as C

import numpy as np

from ._lib import check, lib
from .api import (BilinearDiffusionIntegrator, BilinearMassIntegrator, ConductivityToDiffusivityCoefficient, ConstantCoefficient, DeviceVector,
                  LinearIntegrator, _ptr, allocate_matrix, needs_update, setup_operator, solve_converged, update_operator)
from .ecg import _vertex_ids, vertex_dofs
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

    def solve(self, b, x, rtol=1e-5, atol=1e-6, maxiter=1000):
        it, res = C.c_int(), C.c_double()
        check(lib().tb_bidomain_solve(self.h, _ptr(b), _ptr(x), float(rtol), float(atol), int(maxiter), C.byref(it), C.byref(res)))
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


class BidomainBackwardEulerStage:
    """BackwardEulerStage for the bidomain block system: perform_step(φₘ, t, Δt) advances φₘ in place and the stage's own `phi_e` (n values, zero at
    the start, the initial guess of the next step).  `ground`: vertex ids (or positions), mandatory.  `source`: the transmembrane stimulus, a
    LinearIntegrator scaled as BackwardEulerStage scales its source.  `source_e`: the extracellular current Iₛₜᵢₘ,ₑ − Iₛₜᵢₘ,ᵢ, a LinearIntegrator or
    nodal currents by dof (array of n values); it has to sum to zero (checked whenever it is (re)assembled).  The combined operator is rebuilt only
    when Δt changes (`generation` counts the rebuilds).  `solver.mirror` has no meaning here."""

    def __init__(self, solver, strategy, dh, diffusion_i, diffusion_e, ground, source=None, source_e=None, pattern=None, t0=0.0):
        if dh.ip.order != 1 or dh.ip.ncomp != 1:
            raise NotImplementedError("BidomainBackwardEulerStage: first-order scalar fields only (order %d, %d component(s))" % (dh.ip.order, dh.ip.ncomp))
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
        its, res = self.system.solve(self.rhs, self.x, self.solver.rtol, self.solver.atol, self.solver.maxiter)
        self.system.unpack(self.x, phi, self.phi_e)
        self.last_iters, self.last_resnorm = its, res
        return solve_converged(self.M.pattern, res)
