"""Activation times from the anisotropic eikonal equation √(∇Tᵀ G ∇T) = 1 on the device, and the transmembrane potential recovered from them by
shifting an action-potential template: the reaction-eikonal route to a pseudo-ECG.

The reference names this as its next electrophysiology tutorial and has not written it (docs/src/literate-tutorials/ep05_eikonal.jl is an empty
stub, docs/src/tutorials/index.md:96 "Reaction-Eikonal ECG (TODO)"), so there is no reference interface to mirror; the names below follow the
package's own pattern (model, cache, verbs):

  EikonalModel(G)                                  G: the squared conduction velocity, any coefficient BilinearDiffusionIntegrator takes
  EikonalActivationCache(strategy_or_device, model, dh)   owns the diffusion form and the tb_eikonal (csrc/tb_eikonal.hip)
  solve_activation(cache, sources, times, …)       → DeviceVector T of the handler's dofs (+∞ where no source reaches)
  ActionPotentialTemplate(t0, dt, samples)         a uniformly tabulated U; .from_cell_model runs an ionic model on one point
  activation_potential(cache_or_T, t, template)    φₘ = U(t − T), a DeviceVector update_ecg takes as it is

Out of scope (each refused with a message where it can be reached): quadrilaterals and 2-D problems, second-order fields, cell sets and
subdomains, several ranks, eikonal-diffusion and eikonal-reaction variants, re-entry and repolarisation times, Float32."""
import ctypes as C

import numpy as np

from . import _lib as L
from ._lib import check, lib
from .ecg import vertex_dofs
from .api import (BilinearDiffusionIntegrator, DeviceVector, MI355XDevice, PointwiseODEFunction, ForwardEulerCellSolver, _Form, _lower_coef, _ptr,
                  perform_step, setup_solver_cache)


class EikonalModel:
    """EikonalModel(G): G the squared conduction velocity tensor — ConstantCoefficient (scalar or 3 × 3), FieldCoefficient,
    SpectralTensorCoefficient over constant or nodal microstructure, or one of them in a ConductivityToDiffusivityCoefficient."""

    def __init__(self, G):
        self.G = G


class EikonalActivationCache:
    """EikonalActivationCache(strategy_or_device, model, dh): the diffusion form that carries G on `dh`'s mesh and the device solver built on it
    (corner incidence, node adjacency, M = G⁻¹ per cell).  After solve_activation: `T` (DeviceVector), `sweeps`, `converged`."""

    def __init__(self, strategy_or_device, model, dh):
        if not isinstance(model, EikonalModel):
            raise TypeError("EikonalActivationCache: model must be an EikonalModel")
        self.device = strategy_or_device if isinstance(strategy_or_device, MI355XDevice) else strategy_or_device.device
        self.model, self.dh = model, dh
        self.dmesh = dh.device_mesh(self.device)
        c, self._keep = _lower_coef(model.G)
        self.form = _Form(self.dmesh, BilinearDiffusionIntegrator.form, 0, c)
        self.h = C.c_void_p()
        check(lib().tb_eikonal_create(self.form.h, C.byref(self.h)))
        self.T = None
        self.sweeps, self.converged = 0, False
        self.evaluations = self.updates = self.local_solves = 0     # of the latest solve (tb_eikonal_last_counts)
        self._source_dofs = None

    def residual(self, T=None, out=None):
        """T_i − min(local solves on T) at every dof that was not a source of the latest solve (tb_eikonal_residual); enqueue only"""
        T = self.T if T is None else T
        out = out or DeviceVector(self.device, self.dh.ndofs)
        assert T.n == self.dh.ndofs and out.n == self.dh.ndofs
        check(lib().tb_eikonal_residual(self.h, _ptr(T), _ptr(out)))
        return out

    def __del__(self):
        try:
            if self.h:
                lib().tb_eikonal_destroy(self.h)
        except Exception:
            pass


def source_dofs(dh, sources):
    """`sources`: vertex ids (0-based grid nodes) or the name of one of the grid's node sets → the dofs of those vertices"""
    if isinstance(sources, str):
        sources = dh.grid.getnodeset(sources)
    v = np.atleast_1d(np.asarray(sources, dtype=np.int64))
    if v.size and (v.min() < 0 or v.max() >= dh.grid.n_nodes):
        raise ValueError("solve_activation: source vertex outside [0, %d)" % dh.grid.n_nodes)
    d = vertex_dofs(dh)[v]
    if (d < 0).any():
        raise ValueError("solve_activation: a source vertex belongs to no cell")
    return d.astype(np.int32)


def solve_activation(cache, sources, times=None, rtol=1e-12, max_sweeps=None, out=None, allow_unconverged=False):
    """Arrival times of the wave that starts at `sources` (vertex ids or a node-set name) at `times` (one per source, default 0): a DeviceVector over
    the handler's dofs, +∞ where no source reaches.  `max_sweeps` defaults to the node count.  Sets cache.T, cache.sweeps and cache.converged; a
    solve that did not converge raises unless allow_unconverged=True."""
    d = np.ascontiguousarray(source_dofs(cache.dh, sources))
    t = np.zeros(len(d)) if times is None else np.ascontiguousarray(np.broadcast_to(np.asarray(times, dtype=np.float64), d.shape))
    if max_sweeps is None:
        max_sweeps = cache.dh.ndofs
    T = out or DeviceVector(cache.device, cache.dh.ndofs)
    assert T.n == cache.dh.ndofs
    sweeps, conv = C.c_int(), C.c_int()
    check(lib().tb_eikonal_solve(cache.h, len(d), d.ctypes.data_as(L.c_i32p), t.ctypes.data_as(L.c_dp), float(rtol), int(max_sweeps), _ptr(T),
                                 C.byref(sweeps), C.byref(conv)))
    cache.T, cache.sweeps, cache.converged, cache._source_dofs = T, sweeps.value, bool(conv.value), d
    counts = np.zeros(3, dtype=np.int64)
    check(lib().tb_eikonal_last_counts(cache.h, counts.ctypes.data_as(L.c_i64p)))
    cache.evaluations, cache.updates, cache.local_solves = (int(v) for v in counts)
    if not cache.converged and not allow_unconverged:
        raise RuntimeError("solve_activation: not converged after %d sweeps (max_sweeps = %d); pass allow_unconverged=True to keep the iterate"
                           % (sweeps.value, max_sweeps))
    return T


class ActionPotentialTemplate:
    """ActionPotentialTemplate(t0, dt, samples): U(t0 + k·dt) = samples[k]; linear between the samples, samples[0] before t0 (the resting value),
    samples[-1] beyond the table."""

    def __init__(self, t0, dt, samples):
        self.t0, self.dt = float(t0), float(dt)
        self.samples = np.ascontiguousarray(samples, dtype=np.float64)
        if self.samples.ndim != 1 or len(self.samples) < 2 or not self.dt > 0.0:
            raise ValueError("ActionPotentialTemplate: at least two samples and dt > 0")
        self._dev = {}

    def on(self, device):
        if id(device) not in self._dev:
            self._dev[id(device)] = device.to_device(self.samples)
        return self._dev[id(device)]

    def __call__(self, tau):
        """host evaluation (numpy.interp with clamped ends)"""
        return np.interp(tau, self.t0 + self.dt * np.arange(len(self.samples)), self.samples)

    @classmethod
    def from_cell_model(cls, model, dt, duration, stimulus, device=None, substeps=1):
        """One point of `model` (an ionic model of this package) stepped by the device reaction step: φₘ is raised by `stimulus` at time 0 (an
        instantaneous charge), then recorded every `dt` over `duration`.  Sample 0 is the resting value."""
        device = device or MI355XDevice(0)
        f = PointwiseODEFunction(1, model)
        u0 = np.asarray(model.default_initial_state(), dtype=np.float64).copy()
        rest = u0[model.phi_index]
        u0[model.phi_index] += float(stimulus)
        cache = setup_solver_cache(f, ForwardEulerCellSolver(device), u=device.to_device(u0))
        n = int(round(duration / dt))
        samples = np.empty(n + 1)
        samples[0] = rest
        h = dt / substeps
        for k in range(n):
            for j in range(substeps):
                perform_step(f, cache, k * dt + j * h, h)
            samples[k + 1] = cache.un.to_host()[model.phi_index]
        return cls(0.0, dt, samples)


def activation_potential(cache_or_T, t, template, out=None):
    """φₘ(x) = U(t − T(x)) (tb_eikonal_potential): `cache_or_T` an EikonalActivationCache after solve_activation, or a DeviceVector of arrival
    times.  Enqueue only — inside MI355XDevice.capture the time is the one DeviceGraph.launch(t) sets."""
    T = cache_or_T.T if isinstance(cache_or_T, EikonalActivationCache) else cache_or_T
    if T is None:
        raise ValueError("activation_potential: the cache holds no activation times yet (solve_activation)")
    dev = T.dev
    out = out or DeviceVector(dev, T.n)
    assert out.n == T.n
    U = template.on(dev)
    check(lib().tb_eikonal_potential(dev.h, T.n, _ptr(T), float(t), len(template.samples), template.t0, template.dt, _ptr(U), _ptr(out)))
    return out
