"""Pseudo-ECG from the transmembrane potential on the device: the Plonsey volume integral, the Poisson reconstruction and Geselowitz lead fields.

  reference (file:line)                                                                 here
  ---------------------------------------------------------------------------------------------------------------
  Plonsey1964ECGGaussCache(op, φₘ)        src/modeling/electrophysiology/ecg.jl:55-69        same name
  PoissonECGReconstructionCache(…)        ecg.jl:166-338                                     same name
  Geselowitz1989ECGLeadCache(…)           ecg.jl:382-590                                     same name
  update_ecg!(cache, φₘ)                  ecg.jl:140-147, 340-353, 607-614                   update_ecg
  evaluate_ecg(cache[, x, κₜ])            ecg.jl:80-106, 356-359, 617-619                    evaluate_ecg
  get_closest_vertex(x, grid)             called at ecg.jl:417-418                           get_closest_vertex (returns the node id)
  _add_electrode!                         ecg.jl:592-605                                     lead_right_hand_sides

The arithmetic that belongs to the ECG runs in csrc/tb_ecg.hip (tb_ecg_*, tb_scrub_scale); the torso methods stand on what the package already has:
assembled diffusion operators, NodalIntergridInterpolation, apply_zero and the preconditioned CG.  This project's DofHandler is ONE field on ONE
subdomain, so "κᵢ in the heart, 0 outside" (the reference's AnalyticalCoefficient of test_ecg.jl, or its subdomain handlers) is a FieldCoefficient on
the torso mesh: `cellset_coefficient` builds it from a cell set.

Three things are handled differently from the reference, on purpose:
  * evaluate_ecg(::Plonsey…, x::AbstractVector{<:Vec}, κₜ) (ecg.jl:100-106) overwrites its result with the last electrode's scalar — an evident
    slip.  Here the intent: one value per electrode.
  * The diffusion form carries the reference's minus sign (diffusion.jl:28-50), so K is negative semi-definite and the device CG (which flags
    pᵀAp ≤ 0) is handed −K and −b, as coordinates.py does with D = −I.
  * The reference's lead solve never applies its ground constraint — it hands the singular system to a direct solver (ecg.jl:569-587).  Here the
    ground is applied.  The source Kᵢφₘ sums to zero (constants are in the kernel of Kᵢ), so the constant this fixes is invisible in the leads.
`subdomains_from` and time-dependent conductivities have no counterpart (forms are evaluated at their creation time)."""
import ctypes as C

import numpy as np

from . import _lib as L
from ._lib import check, lib
from .api import (BilinearDiffusionIntegrator, BilinearOperator, DeviceVector, FieldCoefficient, PerColorAssemblyStrategy, _ptr, allocate_matrix,
                  pcg_solve, setup_operator, update_operator)
from .solid import ConstraintHandler, apply_zero, meandiag
from .transfer import NodalIntergridInterpolation, PointEvalHandler, evaluate_at_points, transfer


# --------------------------------------------------------------------------------------- host helpers
def get_closest_vertex(x, grid):
    """get_closest_vertex(x, grid): the id (0-based) of the grid node closest to x; the lowest id among equally close ones."""
    d = grid.xyz - np.asarray(x, dtype=np.float64).reshape(1, 3)
    return int(np.argmin((d * d).sum(axis=1)))


def vertex_dofs(dh):
    """dof of every grid node for a first-order scalar field (the reference's vertexdof_indices + celldofs, ecg.jl:599-602)"""
    if dh.ip.order != 1 or dh.ip.ncomp != 1:
        raise NotImplementedError("vertex_dofs: first-order scalar fields")
    n2d = np.full(dh.grid.n_nodes, -1, dtype=np.int64)
    n2d[dh.grid.conn.ravel()] = dh.cell_dofs.ravel()
    return n2d


def cellset_coefficient(grid, cells, inside=1.0, outside=0.0):
    """FieldCoefficient on `grid` that is `inside` in the cells of the set (a name of one of the grid's cell sets, or 0-based ids) and `outside`
    elsewhere — e.g. κᵢ on a torso mesh whose heart is a cell set.  The nodal data are per cell, so the jump is exact at the set's boundary."""
    cells = grid.getcellset(cells) if isinstance(cells, str) else np.asarray(cells, dtype=np.int64)
    data = np.full(grid.conn.shape, float(outside))
    data[cells] = float(inside)
    return FieldCoefficient(data)


def lead_right_hand_sides(ndofs, electrode_dof_sets):
    """The right-hand sides of the lead-field solves (ecg.jl:571-583 with _add_electrode!, which STORES −weight): per set, the first electrode's
    dof holds −1 and each of the other m holds +1/m.  (n_leads, ndofs)."""
    rhs = np.zeros((len(electrode_dof_sets), ndofs))
    for i, s in enumerate(electrode_dof_sets):
        if len(s) < 2:
            raise ValueError("Electrode set %d has too few electrodes (%d<2)" % (i, len(s)))
        rhs[i, s[0]] = -1.0
        for d in s[1:]:
            rhs[i, d] = 1.0 / (len(s) - 1)
    return rhs


def _vertex_ids(items, grid):
    """positions → closest vertices; integers are vertex ids already"""
    return [int(v) if np.ndim(v) == 0 else get_closest_vertex(v, grid) for v in items]


def _device_points(device, x):
    if isinstance(x, DeviceVector):
        assert x.n % 3 == 0, "device electrodes are n × 3 doubles"
        return x, x.n // 3
    p = np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(-1, 3))
    return device.to_device(p.ravel()), len(p)


def scrub_scale(x, alpha):
    """x = α·(isnan(x) ? 0 : x) on the device (tb_scrub_scale; ecg.jl:345-347, 612); enqueue only"""
    check(lib().tb_scrub_scale(x.dev.h, x.n, float(alpha), x.ptr))
    return x


# --------------------------------------------------------------------------------------- Plonsey
class Plonsey1964ECGGaussCache:
    """Plonsey1964ECGGaussCache(op, φₘ): `op` an assembled-operator object of a BilinearDiffusionIntegrator on the heart mesh (its D and
    quadrature are the cache's), `φₘ` a DeviceVector of the heart's dofs.  Holds κ∇φₘ at the quadrature points (`fluxes()`: host copy,
    (n_cells, n_qp, 3)); x̃ and dΩ are tabulated once on the device."""

    def __init__(self, op, phi):
        if not isinstance(op, BilinearOperator) or op.integrator.form != L.TB_FORM_DIFFUSION:
            raise TypeError("Plonsey1964ECGGaussCache: op must be the operator of a BilinearDiffusionIntegrator")
        self.op, self.device = op, op.strategy.device
        self.h = C.c_void_p()
        check(lib().tb_ecg_create(op.form.h, C.byref(self.h)))
        self.n_points = int(lib().tb_ecg_npoints(self.h))
        self._x = None
        self.update(phi)

    def update(self, phi):
        assert phi.n == self.op.dh.ndofs, "φₘ has %d entries, the handler %d dofs" % (phi.n, self.op.dh.ndofs)
        check(lib().tb_ecg_update(self.h, _ptr(phi)))

    def evaluate(self, x, kappa_t, out=None):
        """x: one point, (n, 3) host values or a DeviceVector of 3·n doubles (then nothing is uploaded: with `out` given the call only enqueues)"""
        if not isinstance(x, DeviceVector):
            key = np.asarray(x, dtype=np.float64).tobytes()
            if self._x is None or self._x[0] != key:                 # the electrodes of the previous call stay on the device
                self._x = (key,) + _device_points(self.device, x)
            xd, n = self._x[1], self._x[2]
        else:
            xd, n = _device_points(self.device, x)
        if out is None:
            out = DeviceVector(self.device, n)
        assert out.n == n
        check(lib().tb_ecg_evaluate(self.h, n, _ptr(xd), float(kappa_t), _ptr(out)))
        return out

    def fluxes(self):
        nq = self.n_points // self.op.dh.grid.n_cells
        out = np.empty(3 * self.n_points)
        check(lib().tb_memcpy_d2h(self.device.h, out.ctypes.data_as(C.c_void_p), C.c_void_p(lib().tb_ecg_fluxes_device(self.h)), out.nbytes))
        return out.reshape(-1, nq, 3)

    def __del__(self):
        try:
            if self.h:
                lib().tb_ecg_destroy(self.h)
        except Exception:
            pass


# --------------------------------------------------------------------------------------- the torso part both torso methods share
class _TorsoSource:
    """heart → torso transfer and the source operator Kᵢ on the torso: φₘ_t and Kᵢφₘ_t (ecg.jl:342-344, 609-611)"""

    def __init__(self, device, heart_dh, torso_dh, kappa_i, torso_heart_domain, strategy, qorder, pattern):
        self.device, self.heart_dh, self.torso_dh = device, heart_dh, torso_dh
        self.strategy = strategy or PerColorAssemblyStrategy(device)
        self.sp = pattern or allocate_matrix(torso_dh)
        self.source_op = update_operator(setup_operator(self.strategy, BilinearDiffusionIntegrator(kappa_i, qorder), torso_dh, self.sp), 0.0)
        self.transfer_op = NodalIntergridInterpolation(device, heart_dh, torso_dh, subdomains_to=torso_heart_domain)
        self.phi_t = device.zeros(torso_dh.ndofs)          # φₘ on the torso; dofs outside the heart domain stay 0
        self.source = device.zeros(torso_dh.ndofs)         # κ∇φₘ_t of the reference

    def product(self, phi, alpha):
        transfer(self.phi_t, self.transfer_op, phi)
        self.source_op.mul(self.source, self.phi_t, alpha, 0.0)


def _negated_grounded_matrix(device, op, ch):
    """−K with the ground rows and columns eliminated (mean diagonal on the eliminated rows): symmetric positive definite"""
    A = device.zeros(op.A.n)
    check(lib().tb_axpy(device.h, op.A.n, -1.0, op.A.ptr, A.ptr))
    apply_zero(A, None, ch, pattern=op.pattern, diag=meandiag(op.pattern, A))
    return A


# --------------------------------------------------------------------------------------- Poisson
class PoissonECGReconstructionCache:
    """PoissonECGReconstructionCache(device, heart_dh, torso_dh, κᵢ, κ, electrodes, ground, torso_heart_domain): ∇·κ∇φₑ = −∇·κᵢ∇φₘ on the torso
    (ecg.jl:149-165).  κᵢ and κ are coefficients on the TORSO mesh (κᵢ zero outside the heart: cellset_coefficient); `ground`: vertex ids or
    positions (closest vertex) held at φₑ = 0; `torso_heart_domain`: the torso cells the heart occupies (cell-set name or ids; None: every cell).
    Raises if an electrode is not found in the torso mesh (ecg.jl:284-289).

    update_ecg: transfer → source_op.mul → tb_scrub_scale(−1) → apply_zero → solve, all on the device.  The product is taken with α = −1, so that
    `source` holds the reference's right-hand side b = −Kᵢφₘ_t (before its NaN scrub); tb_scrub_scale(−1) scrubs it and forms −b, the right-hand side
    of the −K system the CG is given (see the module docstring).  The solve is pcg_solve (rtol 1e-12 relative to ‖b‖: it starts from zero)."""

    def __init__(self, device, heart_dh, torso_dh, kappa_i, kappa, electrodes, ground, torso_heart_domain=None, strategy=None, qorder=0,
                 rtol=1e-12, maxiter=20000, precond="jacobi", pattern=None):
        self.device, self.torso_dh = device, torso_dh
        self.src = _TorsoSource(device, heart_dh, torso_dh, kappa_i, torso_heart_domain, strategy, qorder, pattern)
        self.source_op, self.transfer_op = self.src.source_op, self.src.transfer_op
        self.torso_op = update_operator(setup_operator(self.src.strategy, BilinearDiffusionIntegrator(kappa, qorder), torso_dh, self.src.sp), 0.0)
        self.ch = ConstraintHandler(torso_dh, vertex_dofs(torso_dh)[_vertex_ids(ground, torso_dh.grid)])
        self.ph = PointEvalHandler(device, torso_dh, np.asarray(electrodes, dtype=np.float64).reshape(-1, 3))
        if self.ph.n_missing:
            raise RuntimeError("Poisson reconstruction setup failed! Some electrodes are not found in the torso mesh (%s)." % (self.ph.cells,))
        self.A = _negated_grounded_matrix(device, self.torso_op, self.ch)
        self.phi_e = device.zeros(torso_dh.ndofs)
        self.rtol, self.maxiter, self.precond = rtol, maxiter, precond
        self.last_iters, self.last_resnorm = 0, 0.0

    def right_hand_side(self, phi):
        """the enqueue-only part of update_ecg (fits inside MI355XDevice.capture): `src.source` = −b with the ground entries zeroed"""
        self.src.product(phi, -1.0)
        scrub_scale(self.src.source, -1.0)
        apply_zero(None, self.src.source, self.ch, pattern=self.torso_op.pattern)

    def solve(self):
        # started from zero, not from the previous φₑ as the reference's u0 = ϕₑ: the stopping test is relative to ‖b − A x₀‖, and a start at the
        # converged solution of the previous step would ask for twelve more digits than the arithmetic has
        self.phi_e.fill_zero()
        self.last_iters, self.last_resnorm = pcg_solve(self.torso_op.pattern, self.A, self.src.source, self.phi_e, rtol=self.rtol, atol=0.0,
                                                       maxiter=self.maxiter, precond=self.precond)

    def update(self, phi):
        self.right_hand_side(phi)
        self.solve()

    def evaluate(self, out=None):
        return evaluate_at_points(self.ph, self.torso_dh, self.phi_e, out)


# --------------------------------------------------------------------------------------- lead fields
class Geselowitz1989ECGLeadCache:
    """Geselowitz1989ECGLeadCache(device, heart_dh, torso_dh, κᵢ, κ, electrode_sets, ground, torso_heart_domain): one lead per electrode set
    (≥ 2 electrodes each: positions, snapped to the closest torso vertex, or vertex ids).  The lead field of a set solves K Z = rhs with the
    right-hand sides of ecg.jl:571-583 (lead_right_hand_sides) and the ground applied — one solve per lead, into the dense row-major device
    matrix `Z` (n_leads × ndofs).  update_ecg = transfer → mul → scrub; evaluate_ecg = −Z·(Kᵢφₘ_t) by tb_ecg_leads, without leaving the device."""

    def __init__(self, device, heart_dh, torso_dh, kappa_i, kappa, electrode_sets, ground, torso_heart_domain=None, strategy=None, qorder=0,
                 rtol=1e-12, maxiter=20000, precond="jacobi", pattern=None):
        self.device, self.torso_dh = device, torso_dh
        self.src = _TorsoSource(device, heart_dh, torso_dh, kappa_i, torso_heart_domain, strategy, qorder, pattern)
        self.source_op, self.transfer_op = self.src.source_op, self.src.transfer_op
        lead_op = update_operator(setup_operator(self.src.strategy, BilinearDiffusionIntegrator(kappa, qorder), torso_dh, self.src.sp), 0.0)
        n2d = vertex_dofs(torso_dh)
        self.electrode_vertices = [_vertex_ids(s, torso_dh.grid) for s in electrode_sets]
        self.ch = ConstraintHandler(torso_dh, n2d[_vertex_ids(ground, torso_dh.grid)])
        rhs = lead_right_hand_sides(torso_dh.ndofs, [n2d[s] for s in self.electrode_vertices])
        A = _negated_grounded_matrix(device, lead_op, self.ch)
        n = torso_dh.ndofs
        self.n_leads = len(rhs)
        self.Z = device.zeros(self.n_leads * n)
        self.lead_iters = []
        b = DeviceVector(device, n)
        for i, r in enumerate(rhs):                                  # K z = r  ⇔  (−K) z = −r
            b.copy_from_host(-r)
            apply_zero(None, b, self.ch, pattern=lead_op.pattern)
            it, _ = pcg_solve(lead_op.pattern, A, b, self.Z.view(i * n, n), rtol=rtol, atol=0.0, maxiter=maxiter, precond=precond)
            self.lead_iters.append(it)

    def update(self, phi):
        self.src.product(phi, 1.0)
        scrub_scale(self.src.source, 1.0)

    def evaluate(self, out=None):
        n = self.torso_dh.ndofs
        if out is None:
            out = DeviceVector(self.device, self.n_leads)
        assert out.n == self.n_leads
        check(lib().tb_ecg_leads(self.device.h, self.n_leads, n, self.Z.ptr, n, self.src.source.ptr, -1.0, _ptr(out)))
        return out


# --------------------------------------------------------------------------------------- the reference's two verbs
def update_ecg(cache, phi):
    """update_ecg!(cache, φₘ): φₘ a DeviceVector of the heart's dofs"""
    cache.update(phi)


def evaluate_ecg(cache, x=None, kappa_t=None, out=None):
    """evaluate_ecg(plonsey, x, κₜ) → DeviceVector of one value per electrode (x: one point or (n, 3));
    evaluate_ecg(poisson) → φₑ at its electrodes;  evaluate_ecg(geselowitz) → one value per lead."""
    if isinstance(cache, Plonsey1964ECGGaussCache):
        if x is None or kappa_t is None:
            raise TypeError("evaluate_ecg(plonsey_cache, x, kappa_t)")
        return cache.evaluate(x, kappa_t, out)
    return cache.evaluate(out)
