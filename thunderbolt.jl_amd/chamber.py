"""3D–0D chamber coupling of Regazzoni, Salvador, Africa, Fedele, Dedè, Quarteroni (2022): the chamber pressure is an unknown tied to the
cavity volume by a Lagrange-multiplier row, and a closed-loop lumped circulation supplies that volume.

  reference (file:line)                                                            here
  ---------------------------------------------------------------------------------------------------------------
  RSAFDQ2022SurrogateVolume / Hirschvogel2017SurrogateVolume / ConstantChamberVolume   same names
      src/modeling/rsafdq2022.jl:75-85, src/modeling/coupler/fsi.jl:36-58
  ChamberVolumeCoupling / LumpedFluidSolidCoupler        fsi.jl:4-31                same names
  compute_chamber_volume                                 rsafdq2022.jl:22-63        compute_chamber_volume
  AssembledRSAFDQ2022Operator.update_linearization!      rsafdq-operator.jl:36-85   BlockedChamberSystem.linearize
  eliminate_constraints_from_linearization!              rsafdq2022.jl:262-279      (same method)
  SchurComplementLinearSolver                            src/solver/linear/schur.jl:92-197
  RSAFDQ2022LumpedCicuitModel / lumped_driver! / Φ_RSAFDQ2022 / DummyLumpedCircuitModel   src/modeling/fluid/lumped.jl
  RSAFDQ2022Model / RSAFDQ2022Split / semidiscretize     rsafdq2022.jl:125-249      same names / semidiscretize_rsafdq
  VolumeTransfer0D3D / PressureTransfer3D0D + LieTrotterGodunov   transfer_operators.jl:177-223   RSAFDQ2022Integrator.step

The facet integrals run on the device (tb_chamber_assemble, csrc/tb_chamber.hip), the inner solves of the Schur complement are the device
Krylov solvers, A₂₁z are device dot products; the circuit (12 states) and the s₂ × s₂ Schur system stay on the host.
"""
import ctypes as C
import math
from types import SimpleNamespace

import numpy as np

from . import _lib as L
from ._lib import check, lib
from .api import DeviceVector, _ptr
from .solid import (ActiveStressModel, BlockedLinearSolver, DisplacementSystem, HomotopyPathSolver, NewtonRaphsonSolver, NonlinearOperator, apply_zero, dot,
                    inner_linear_solve, nlsolve, solve_converged, update_linearization)

TB_VOLUME_RSAFDQ2022, TB_VOLUME_HIRSCHVOGEL2017 = 0, 1


# --------------------------------------------------------------------------------------- volume methods and coupler
class RSAFDQ2022SurrogateVolume:
    """−∫ det F ((h ⊗ h)(x + d − b)) · F⁻ᵀ N dΓ (rsafdq2022.jl:66-85): the volume measured through the displacement along the axis h."""
    method = TB_VOLUME_RSAFDQ2022

    def __init__(self, h=(0.0, 1.0, 0.0), b=(0.0, 0.0, -0.1)):
        self.h, self.b = np.asarray(h, dtype=np.float64), np.asarray(b, dtype=np.float64)

    def params(self):
        return np.ascontiguousarray(np.concatenate([self.h, self.b]))

    def volume_integral(self, x, d, F, N):
        return -np.linalg.det(F) * (np.outer(self.h, self.h) @ (x + d - self.b)) @ (np.linalg.inv(F).T @ N)


class Hirschvogel2017SurrogateVolume:
    """−∫ (x + d) · det F F⁻ᵀ N dΓ (fsi.jl:44-58)."""
    method = TB_VOLUME_HIRSCHVOGEL2017

    def params(self):
        return None

    def volume_integral(self, x, d, F, N):
        return -np.linalg.det(F) * (x + d) @ (np.linalg.inv(F).T @ N)


class ConstantChamberVolume:
    """Debug helper (fsi.jl:33-42): keeps the chamber volume constant.  Host only — there is nothing to integrate."""
    method = None

    def __init__(self, volume):
        self.volume = float(volume)

    def volume_integral(self, x, d, F, N):
        return self.volume


class ChamberVolumeCoupling:
    """Which surface to couple with which variables of the circuit (fsi.jl:4-17)."""

    def __init__(self, chamber_surface_setname, control_point_setname, chamber_volume_method, lumped_volume_symbol, lumped_pressure_symbol,
                 pressure_symbol_3D):
        self.chamber_surface_setname, self.control_point_setname = chamber_surface_setname, control_point_setname
        self.chamber_volume_method = chamber_volume_method
        self.lumped_volume_symbol, self.lumped_pressure_symbol, self.pressure_symbol_3D = lumped_volume_symbol, lumped_pressure_symbol, pressure_symbol_3D


class LumpedFluidSolidCoupler:
    """Enforce chamber volume 3D = chamber volume 0D by a Lagrange multiplier, the chamber pressure (fsi.jl:19-31)."""

    def __init__(self, chamber_couplings, displacement_symbol):
        self.chamber_couplings, self.displacement_symbol = list(chamber_couplings), displacement_symbol


def _facets_of(dh, setname):
    fs = setname if not isinstance(setname, str) else dh.grid.facetset(setname)
    return np.ascontiguousarray(fs, dtype=np.int32).reshape(-1, 2)


class ChamberForm:
    """Device form of one chamber surface (tb_chamber_form_create)."""

    def __init__(self, dmesh, facets, volume_method, facet_qpoints=0):
        if getattr(volume_method, "method", None) is None:
            raise ValueError("%s has no device form (host only)" % type(volume_method).__name__)
        self.dmesh, self.h = dmesh, C.c_void_p()
        facets = np.ascontiguousarray(facets, dtype=np.int32).reshape(-1, 2)
        mp = volume_method.params()
        check(lib().tb_chamber_form_create(dmesh.h, volume_method.method, None if mp is None else mp.ctypes.data_as(L.c_dp), int(facet_qpoints),
                                           facets.ctypes.data_as(L.c_i32p), len(facets), 0, C.byref(self.h)))

    def assemble(self, u, p, pattern=None, nzval=None, r=None, col=None, row=None, volume=None):
        """tb_chamber_assemble: ADDS to every output given (device vectors)."""
        check(lib().tb_chamber_assemble(self.h, None if pattern is None else pattern.h, _ptr(u), float(p), _ptr(nzval), _ptr(r), _ptr(col), _ptr(row),
                                        _ptr(volume)))

    def __del__(self):
        try:
            lib().tb_form_destroy(self.h)
        except Exception:
            pass


def compute_chamber_volume(dh, u, setname, volume_method, device=None):
    """compute_chamber_volume(dh, u, setname, method) (rsafdq2022.jl:22-63).  Like the reference it integrates with a facet rule of order
    2·order of the interpolation, not the rule of the coupling integrator: 2 Gauss points per direction for Q1.  The device form holds at most 3
    points per direction, so Q2 fields integrate with 3 (exact to degree 5) where the reference takes 4.  `u`: a DeviceVector, or host values
    (then `device` is needed)."""
    if isinstance(volume_method, ConstantChamberVolume):
        return volume_method.volume
    dev = u.dev if isinstance(u, DeviceVector) else device
    ud = u if isinstance(u, DeviceVector) else dev.to_device(np.ascontiguousarray(u, dtype=np.float64))
    form = ChamberForm(dh.device_mesh(dev), _facets_of(dh, setname), volume_method, facet_qpoints=min(2 * dh.ip.order, 3))
    vol = dev.zeros(1)
    form.assemble(ud, 0.0, volume=vol)
    return float(vol.to_host()[0])


# --------------------------------------------------------------------------------------- Schur complement solver
class _HostOps:
    @staticmethod
    def solve(inner, A11, b):
        out = inner(A11, b)
        x, ok = out if isinstance(out, tuple) else (out, True)
        return np.asarray(x, dtype=np.float64), bool(ok), 0, None

    @staticmethod
    def negated(b):
        return -np.asarray(b, dtype=np.float64)

    @staticmethod
    def dot(a, b):
        return float(np.dot(a, b))

    @staticmethod
    def combine(z1, z2, u2, out):
        """out = −(z₁ + Σ z₂ᵢ u₂ᵢ)"""
        out[:] = -(z1 + sum(z * c for z, c in zip(z2, u2)))
        return out


class _DeviceOps:
    def __init__(self, settings):
        self.settings = settings

    def solve(self, inner, A11, b):
        pattern, J = A11
        x = DeviceVector(b.dev, b.n)
        x.fill_zero()
        its, lres = inner_linear_solve(self.settings, pattern, J, b, x, self.settings.inner_rtol)
        return x, lres is None or solve_converged(pattern, lres), its, lres

    @staticmethod
    def negated(b):
        out = DeviceVector(b.dev, b.n)
        out.fill_zero()
        check(lib().tb_axpy(b.dev.h, b.n, -1.0, b.ptr, out.ptr))
        return out

    @staticmethod
    def dot(a, b):
        return dot(a, b)                                      # tb_dot: one scalar to the host

    @staticmethod
    def combine(z1, z2, u2, out):
        out.fill_zero()
        check(lib().tb_axpy(out.dev.h, out.n, -1.0, z1.ptr, out.ptr))
        for z, c in zip(z2, u2):
            check(lib().tb_axpy(out.dev.h, out.n, -float(c), z.ptr, out.ptr))
        return out


class SchurComplementLinearSolver(BlockedLinearSolver):
    """SchurComplementLinearSolver(inner_alg) (schur.jl:1-197) for the 2 × 2 blocked system
        / A₁₁ A₁₂ \\ u₁ = b₁
        \\ A₂₁ A₂₂ / u₂ = b₂
    with a small second block.  Step by step as the reference (:129-186, Benzi, Golub, Liesen 2005 p. 30), signs included:
        A₁₁ z₁ = −b₁,  A₁₁ z₂ᵢ = A₁₂ᵢ,  (A₂₁ z₂ − A₂₂) u₂ = −(A₂₁ z₁ + b₂),  u₁ = −(z₂ u₂ + z₁).
    A failed inner solve fails the outer solve (:133-145, :156-168).  solve(…, strict=False) carries on with a device Krylov solve that stopped
    above its tolerance (the increment is then inexact: `inexact` is set and `residual` holds the largest inner residual norm), which is what
    NewtonRaphsonSolver(strict_inner_solve=False) asks for; an inner solve that reports failure itself fails the outer solve either way.

    inner: "gmres" or "cg" (the device Krylov solvers), a callable (pattern, J, b, x) → iterations as NewtonRaphsonSolver accepts (device), or —
    for systems held on the host — a callable (A₁₁, b) → x or (x, succeeded).  On the device A₁₁ = (pattern, J), b₁ and the columns of A₁₂ /
    rows of A₂₁ are device vectors; A₂₁ z is computed by tb_dot, so only s₂ + s₂² scalars reach the host, where the dense s₂ × s₂ system is solved."""

    def __init__(self, inner="gmres", rtol=1e-8, atol=1e-14, maxiter=5000, gmres_restart=50):
        if inner not in ("cg", "gmres") and not callable(inner):
            raise ValueError("inner: 'cg', 'gmres' or a callable")
        self.inner, self.rtol, self.atol, self.maxiter, self.gmres_restart = inner, rtol, atol, maxiter, gmres_restart
        self.inner_iters, self.failure, self.inexact, self.residual = [], None, False, None

    def _inner(self, ops, A11, b, what, strict):
        """one inner solve → z, or None when it fails the outer solve"""
        z, ok, its, lres = ops.solve(self.inner, A11, b)
        self.inner_iters.append(its)
        if lres is not None:
            self.residual = lres if self.residual is None else max(self.residual, lres)
        if not ok:
            self.failure = what + " solve failed" if lres is None else "%s solve stopped at %d iterations with residual %.3e above its tolerance" % (what, its, lres)
            if strict or lres is None:
                return None
            self.inexact = True
        return z

    def solve(self, A11, A12, A21, A22, b1, b2, u1=None, rtol=None, atol=None, maxiter=None, strict=True):
        """→ (u₁, u₂, succeeded).  A12: the s₂ columns, A21: the s₂ rows, A22: s₂ × s₂ (host), b2: s₂ (host)."""
        host = isinstance(A11, np.ndarray)
        if host:
            ops = _HostOps
            if not callable(self.inner):
                raise ValueError("a host system needs a callable inner solve (A11, b) -> x")
        else:
            ops = _DeviceOps(SimpleNamespace(inner_solver=self.inner, inner_precond=None, inner_rtol=self.rtol if rtol is None else rtol,
                                             inner_atol=self.atol if atol is None else atol, inner_maxiter=self.maxiter if maxiter is None else maxiter,
                                             gmres_restart=self.gmres_restart))
        s2 = len(A12)
        A22 = np.zeros((s2, s2)) if A22 is None else np.asarray(A22, dtype=np.float64).reshape(s2, s2)
        b2 = np.asarray(b2, dtype=np.float64).reshape(s2)
        self.inner_iters, self.failure, self.inexact, self.residual = [], None, False, None
        # A₁₁ z₁ = −b₁
        z1 = self._inner(ops, A11, ops.negated(b1), "A11 z1 = b1", strict)
        if z1 is None:
            return None, None, False
        # the transfer matrix A₁₁ z₂ = A₁₂
        z2 = []
        for i in range(s2):
            z = self._inner(ops, A11, A12[i], "A11 z2 = A12 (%d)" % i, strict)
            if z is None:
                return None, None, False
            z2.append(z)
        # (A₂₁ z₂ − A₂₂) u₂ = −(A₂₁ z₁ + b₂)
        rhs = -(np.array([ops.dot(A21[k], z1) for k in range(s2)]) + b2)
        S = np.array([[ops.dot(A21[k], z2[i]) for i in range(s2)] for k in range(s2)]).reshape(s2, s2) - A22
        try:
            u2 = np.linalg.solve(S, rhs)
        except np.linalg.LinAlgError:
            self.failure = "singular Schur complement"
            return None, None, False
        # u₁ = −(z₂ u₂ + z₁)
        if u1 is None:
            u1 = np.empty_like(z1) if host else DeviceVector(z1.dev, z1.n)
        ops.combine(z1, z2, u2, u1)
        return u1, u2, True


# --------------------------------------------------------------------------------------- blocked operator and Newton
class ChamberTying:
    """RSAFDQ2022SingleChamberTying (rsafdq2022.jl:3-13): one chamber of the blocked problem."""

    def __init__(self, form, volume_method, setname, V0D, volume_index=None, pressure_index=None, pressure_symbol="p"):
        self.form, self.volume_method, self.setname = form, volume_method, setname
        self.V0D = float(V0D)
        self.volume_index, self.pressure_index, self.pressure_symbol = volume_index, pressure_index, pressure_symbol


class BlockedChamberSystem(DisplacementSystem):
    """The unknowns [u_d; p] of the 3D block (RSAFDQ20223DFunction): the displacement lives in nlsolve's device vector, the chamber
    pressures `p` (one per chamber) on the host.  linearize = AssembledRSAFDQ2022Operator.update_linearization! (rsafdq-operator.jl:36-85)
    followed by eliminate_constraints_from_linearization! (rsafdq2022.jl:262-279); the increment comes from the Schur complement solver."""

    def __init__(self, op, ch, chambers, linear_solver=None):
        super().__init__(op, ch)
        if getattr(op, "internal", None) is not None:
            # _check_rsafdq_internal_variables (rsafdq2022.jl:144-171)
            raise ValueError("The RSAFDQ2022 3D-0D coupling does not support materials with internal variables yet. "
                             "Use a material without internal variables, e.g. a plain PK1Model")
        self.chambers = list(chambers)
        self.linear_solver = linear_solver
        dev, n, k = op.strategy.device, op.dh.ndofs, len(self.chambers)
        self.p = np.zeros(k)
        self.cols = [DeviceVector(dev, n) for _ in range(k)]   # J_dp
        self.rows = [DeviceVector(dev, n) for _ in range(k)]   # J_pd
        self.vols = DeviceVector(dev, k)
        self.V3D = np.zeros(k)
        self.r_p = np.zeros(k)
        self.dp = np.zeros(k)
        self.du1 = DeviceVector(dev, n)

    def linearize(self, u, res, t, tangent):
        if not tangent:
            raise NotImplementedError("residual! of the blocked 3D-0D operator (rsafdq-operator.jl:86-93): use the full Newton")
        op, ch = self.op, self.ch
        update_linearization(op, u, t, residual=res)          # pass 1: the volume (and weak boundary) terms
        self.vols.fill_zero()
        for k, chamber in enumerate(self.chambers):           # pass 2: forward and backward coupling
            self.cols[k].fill_zero()
            self.rows[k].fill_zero()
            chamber.form.assemble(u, self.p[k], pattern=op.pattern, nzval=op.J, r=res, col=self.cols[k], row=self.rows[k], volume=self.vols.view(k, 1))
        apply_zero(op.J, res, ch, pattern=op.pattern)
        for k in range(len(self.chambers)):
            apply_zero(None, self.cols[k], ch, pattern=op.pattern)   # J_dp[prescribed, :] = 0
            apply_zero(None, self.rows[k], ch, pattern=op.pattern)   # J_pd[:, prescribed] = 0
        self.V3D = self.vols.to_host()
        self.r_p = self.V3D - np.array([c.V0D for c in self.chambers])

    def residual_norm(self, res):
        return float(np.sqrt(dot(res, res) + float(self.r_p @ self.r_p)))

    def solve_increment(self, solver, res, du, inner_rtol):
        ls = self.linear_solver if self.linear_solver is not None else solver.inner_solver
        if not isinstance(ls, SchurComplementLinearSolver):
            ls = SchurComplementLinearSolver(ls, gmres_restart=solver.gmres_restart)
        _, dp, ok = ls.solve((self.op.pattern, self.op.J), self.cols, self.rows, None, res, self.r_p, u1=du, rtol=inner_rtol, atol=solver.inner_atol,
                             maxiter=solver.inner_maxiter, strict=solver.strict_inner_solve)
        its = int(sum(ls.inner_iters))
        self.failure_detail = ls.failure
        if not ok:
            return its, None, False                           # no increment: nlsolve fails the step whatever strict_inner_solve says
        self.dp = dp
        return its, ls.residual, not ls.inexact

    def apply_increment(self, u, du):
        inorm_d = super().apply_increment(u, du)
        self.p = self.p - self.dp
        return float(np.sqrt(inorm_d ** 2 + float(self.dp @ self.dp)))

    def save_state(self, u):
        return u.to_host(), self.p.copy()

    def restore_state(self, u, state):
        u.copy_from_host(state[0])
        self.p = state[1].copy()


# --------------------------------------------------------------------------------------- lumped circulation (host, 12 states)
def Φ_RSAFDQ2022(t, tC, tR, TC, TR, THB):
    """Activation transient of the paper (lumped.jl:80-100): [tC, tC + TC] contraction, [tR, tR + TR] relaxation, period THB."""
    tnow = (t - tC) % THB
    if 0 <= tnow < TC:
        return 0.5 * (1.0 - math.cos(math.pi / TC * tnow))
    tnow = (t - tR) % THB
    if 0 <= tnow < TR:
        return 0.5 * (1.0 + math.cos(math.pi / TR * tnow))
    return 0.0


Phi_RSAFDQ2022 = Φ_RSAFDQ2022


def elastance_RSAFDQ2022(t, Epass, Emax, tC, tR, TC, TR, THB):
    return Epass + Emax * Φ_RSAFDQ2022(t, tC, tR, TC, TR, THB)


class DummyLumpedCircuitModel:
    """DummyLumpedCircuitModel(volume_fun) (lumped.jl:56-78): locks the volume at volume_fun(t)."""

    def __init__(self, volume_fun):
        self.volume_fun = volume_fun

    def state_symbols(self):
        return ("V",)

    def num_states(self):
        return 1

    def num_unknown_pressures(self):
        return 1

    def get_variable_symbol_index(self, symbol):
        return 0                                              # deliberately permissive: the single state is the chamber volume

    def get_parameter_symbol_index(self, symbol):
        return 0

    def default_initial_state(self):
        return np.array([float(self.volume_fun(0.0))])

    def lumped_driver(self, du, u, t, external_input):
        du[0] = self.volume_fun(t) - u[0]
        return du

    def advance(self, u, t, dt, external_input, substeps=None):
        return np.array([float(self.volume_fun(t + dt))])     # the state IS the prescribed volume


class RSAFDQ2022LumpedCicuitModel:
    """Lumped (0D) closed-loop circulation for LV simulations (lumped.jl:106-367; the reference's spelling of the name).  Parameters and
    defaults are the reference's; Python folds the subscript letters of an identifier (NFKC), so `Rsysₐᵣ` and `Rsysar` name the same
    keyword.  Units kPa, mL, ms.  States, in the order lumped_driver writes them: state_symbols()."""

    DEFAULTS = dict(
        lv_pressure_given=True, rv_pressure_given=True, la_pressure_given=True, ra_pressure_given=True,
        Rsysar=106.6578947368421, Csysar=9.000740192450037, Lsysar=666.6118421052632,
        Rsysven=34.66381578947368, Csysven=1200.098692326671, Lsysven=66.66118421052632,
        Rpular=21.66488486842105, Cpular=75.00616827041698, Lpular=66.66118421052632,
        Rpulven=21.66488486842105, Cpulven=120.0098692326671, Lpulven=66.66118421052632,
        Rmin=1.0, Rmax=9.999e6,
        Epassla=0.011999013157894737, Eactmaxla=0.009332565789473684, V0la=4.0, tCla=600.0, TCla=104.0, TRla=680.0,
        Epassra=0.009332565789473684, Eactmaxra=0.007999342105263157, V0ra=4.0, TRra=560.0, tCra=64.0, TCra=640.0,
        Epassrv=0.0066661184210526315, Eactmaxrv=0.07332730263157895, V0rv=10.0, tCrv=0.0, TCrv=272.0, TRrv=120.0,
        Epasslv=0.01066578947368421, Eactmaxlv=0.3666365131578947, V0lv=5.0, tClv=0.0, TClv=340.0, TRlv=170.0,
        pex=0.0, THB=800.0)
    STATE_SYMBOLS = ("Vₗₐ", "Vₗᵥ", "Vᵣₐ", "Vᵣᵥ", "psysₐᵣ", "psysᵥₑₙ", "ppulₐᵣ", "ppulᵥₑₙ", "Qsysₐᵣ", "Qsysᵥₑₙ", "Qpulₐᵣ", "Qpulᵥₑₙ")

    def __init__(self, **kw):
        unknown = set(kw) - set(self.DEFAULTS)
        if unknown:
            raise TypeError("RSAFDQ2022LumpedCicuitModel: unknown parameters %s" % sorted(unknown))
        for k, v in self.DEFAULTS.items():
            setattr(self, k, kw.get(k, v))

    def state_symbols(self):
        return self.STATE_SYMBOLS

    def num_states(self):
        return 12

    def num_unknown_pressures(self):
        return int(not self.lv_pressure_given) + int(not self.rv_pressure_given) + int(not self.la_pressure_given) + int(not self.ra_pressure_given)

    def get_variable_symbol_index(self, symbol):
        """position (0-based) of `symbol` in the state vector (lumped.jl:15-27)"""
        import unicodedata
        key = unicodedata.normalize("NFKC", symbol)
        for i, s in enumerate(self.STATE_SYMBOLS):
            if s == symbol or unicodedata.normalize("NFKC", s) == key:
                return i
        raise KeyError("Variable named %r not found in a RSAFDQ2022LumpedCicuitModel. Available: %s" % (symbol, ", ".join(self.STATE_SYMBOLS)))

    # The pressure-index rules are the reference's, statement by statement (lumped.jl:221-261), shifted to 0-based: the counter advances for
    # every EARLIER chamber whose pressure is given.
    def lumped_circuit_relative_lv_pressure_index(self):
        return 0

    def lumped_circuit_relative_rv_pressure_index(self):
        return int(self.lv_pressure_given)

    def lumped_circuit_relative_la_pressure_index(self):
        return int(self.lv_pressure_given) + int(self.rv_pressure_given)

    def lumped_circuit_relative_ra_pressure_index(self):
        return int(self.lv_pressure_given) + int(self.rv_pressure_given) + int(self.la_pressure_given)

    def get_parameter_symbol_index(self, symbol):
        import unicodedata
        key = unicodedata.normalize("NFKC", symbol)
        table = {"pla": ("la_pressure_given", self.lumped_circuit_relative_la_pressure_index), "plv": ("lv_pressure_given", self.lumped_circuit_relative_lv_pressure_index),
                 "pra": ("ra_pressure_given", self.lumped_circuit_relative_ra_pressure_index), "prv": ("rv_pressure_given", self.lumped_circuit_relative_rv_pressure_index)}
        if key not in table:
            raise KeyError("Variable named %r not found for RSAFDQ2022LumpedCicuitModel: the external pressures are pₗₐ, pₗᵥ, pᵣₐ, pᵣᵥ" % symbol)
        given, index = table[key]
        if getattr(self, given):
            raise KeyError("Trying to query the external pressure index of %r, but that pressure is not an external input" % symbol)
        return index()

    def default_initial_state(self):
        """default_initial_state! (lumped.jl:216-219): obtain a periodic state by pre-pacing in isolation"""
        return np.array([65.0, 120.0, 65.0, 145.0, 10.66, 4.0, 4.67, 3.2, 0.0, 0.0, 0.0, 0.0])

    def lumped_driver(self, du, u, t, external_input):
        """Right-hand side of equation system (6) of the paper (lumped_driver!, lumped.jl:263-367)."""
        m = self
        Vla, Vlv, Vra, Vrv, psysar, psysven, ppular, ppulven, Qsysar, Qsysven, Qpular, Qpulven = (float(v) for v in u)
        # note tR = tC + TC
        plv = elastance_RSAFDQ2022(t, m.Epasslv, m.Eactmaxlv, m.tClv, m.tClv + m.TClv, m.TClv, m.TRlv, m.THB) * (Vlv - m.V0lv) if m.lv_pressure_given \
            else external_input[m.lumped_circuit_relative_lv_pressure_index()]
        prv = elastance_RSAFDQ2022(t, m.Epassrv, m.Eactmaxrv, m.tCrv, m.tCrv + m.TCrv, m.TCrv, m.TRrv, m.THB) * (Vrv - m.V0rv) if m.rv_pressure_given \
            else external_input[m.lumped_circuit_relative_rv_pressure_index()]
        pla = elastance_RSAFDQ2022(t, m.Epassla, m.Eactmaxla, m.tCla, m.tCla + m.TCla, m.TCla, m.TRla, m.THB) * (Vla - m.V0la) if m.la_pressure_given \
            else external_input[m.lumped_circuit_relative_la_pressure_index()]
        pra = elastance_RSAFDQ2022(t, m.Epassra, m.Eactmaxra, m.tCra, m.tCra + m.TCra, m.TCra, m.TRra, m.THB) * (Vra - m.V0ra) if m.ra_pressure_given \
            else external_input[m.lumped_circuit_relative_ra_pressure_index()]

        def Q(p1, p2):                                        # valve: Rmin when open, Rmax when closed
            return (p1 - p2) / (m.Rmin if p1 > p2 else m.Rmax)

        Qmv, Qav, Qtv, Qpv = Q(pla, plv), Q(plv, psysar), Q(pra, prv), Q(prv, ppular)
        du[0] = Qpulven - Qmv                                 # LA
        du[1] = Qmv - Qav                                     # LV
        du[2] = Qsysven - Qtv                                 # RA
        du[3] = Qtv - Qpv                                     # RV
        du[4] = (Qav - Qsysar) / m.Csysar
        du[5] = (Qsysar - Qsysven) / m.Csysven
        du[6] = (Qpv - Qpular) / m.Cpular
        du[7] = (Qpular - Qpulven) / m.Cpulven
        du[8] = -m.Rsysar / m.Lsysar * (Qsysar + (psysven - psysar) / m.Rsysar)
        du[9] = -m.Rsysven / m.Lsysven * (Qsysven + (pra - psysven) / m.Rsysven)
        du[10] = -m.Rpular / m.Lpular * (Qpular + (ppulven - ppular) / m.Rpular)
        du[11] = -m.Rpulven / m.Lpulven * (Qpulven + (pla - ppulven) / m.Rpulven)
        return du

    def advance(self, u, t, dt, external_input, substeps=None):
        return integrate_circuit(self, u, t, dt, external_input, substeps=substeps)


def integrate_circuit(model, u, t, dt, external_input=(), substeps=None, max_substep=0.5):
    """Advance the circuit over [t, t + dt] with the classical fourth-order Runge–Kutta method on `substeps` equal sub-steps (default: the fewest
    with a sub-step ≤ max_substep ms; the fastest rates of the default circuit are below 1/ms).  This departs from the reference, which
    integrates the circuit with the adaptive Tsit5 of a third-party package; results agree to the accuracy of either integrator, not to rounding."""
    n = int(substeps) if substeps else max(1, int(math.ceil(abs(dt) / max_substep - 1e-12)))
    h = dt / n
    y = [float(v) for v in u]
    m = len(y)
    k1, k2, k3, k4 = [0.0] * m, [0.0] * m, [0.0] * m, [0.0] * m
    for s in range(n):
        ts = t + s * h
        model.lumped_driver(k1, y, ts, external_input)
        model.lumped_driver(k2, [y[i] + 0.5 * h * k1[i] for i in range(m)], ts + 0.5 * h, external_input)
        model.lumped_driver(k3, [y[i] + 0.5 * h * k2[i] for i in range(m)], ts + 0.5 * h, external_input)
        model.lumped_driver(k4, [y[i] + h * k3[i] for i in range(m)], ts + h, external_input)
        y = [y[i] + h / 6.0 * (k1[i] + 2.0 * k2[i] + 2.0 * k3[i] + k4[i]) for i in range(m)]
    return np.array(y)


def prepace_circuit(model, beats=10, substeps_per_beat=None):
    """The reference's set-up (test_fsi.jl:66-75): the circuit alone, all pressures given, from its default state over `beats` heart beats."""
    u = model.default_initial_state()
    for b in range(beats):
        u = integrate_circuit(model, u, b * model.THB, model.THB, (), substeps=substeps_per_beat)
    return u


# --------------------------------------------------------------------------------------- the split model
class RSAFDQ2022Model:
    """The split model of the paper (rsafdq2022.jl:122-133): structural model, circuit model, coupler."""

    def __init__(self, structural_model, circuit_model, coupler):
        self.structural_model, self.circuit_model, self.coupler = structural_model, circuit_model, coupler


class RSAFDQ2022Split:
    """Annotation for the split of the paper (rsafdq2022.jl:135-140)."""

    def __init__(self, model):
        self.model = model


class RSAFDQ2022Function:
    """What semidiscretize(::RSAFDQ2022Split, …) returns (rsafdq2022.jl:208-249): the blocked 3D function with its chamber tyings and the
    circuit function, plus the state both sub-problems work on."""

    def __init__(self, split, op, ch, chambers, circuit_model, linear_solver=None):
        self.split, self.op, self.ch, self.circuit_model = split, op, ch, circuit_model
        self.system = BlockedChamberSystem(op, ch, chambers, linear_solver)
        self.chambers = self.system.chambers
        self.u = op.strategy.device.zeros(op.dh.ndofs)
        self.circuit_state = circuit_model.default_initial_state()
        self.external_input = np.zeros(circuit_model.num_unknown_pressures())

    @property
    def pressures(self):
        return self.system.p

    @property
    def V3D(self):
        return self.system.V3D


def semidiscretize_rsafdq(split, strategy, dh, pattern, ch, facet_qpoints=0, linear_solver=None):
    """semidiscretize(::RSAFDQ2022Split, discretization, mesh) (rsafdq2022.jl:208-249) with the discretisation objects of this package:
    `dh`, the sparsity `pattern` and the constraint handler `ch` of the displacement field."""
    model = split.model
    coupler, circuit = model.coupler, model.circuit_model
    if len(coupler.chamber_couplings) < 1:
        raise ValueError("Provide at least one coupling for the semi-discretization of an RSAFDQ2022 model")
    sm = model.structural_model
    domains = list(sm.values()) if isinstance(sm, dict) else [sm]
    if any(coupler.displacement_symbol != q.sym for q in domains):
        raise ValueError("Coupler is not compatible with structural model")
    for q in domains:
        cm = q.constitutive_model
        if isinstance(cm, ActiveStressModel) and cm.internal_model() is not None:
            raise ValueError("The RSAFDQ2022 3D-0D coupling does not support materials with internal variables yet. "
                             "Use a material without internal variables, e.g. a plain PK1Model")
    op = NonlinearOperator(strategy, sm, dh, pattern)
    if circuit.num_unknown_pressures() != len(coupler.chamber_couplings):
        raise ValueError("Number of chambers in structural model (%d) and circuit model (%d) differs." % (len(coupler.chamber_couplings), circuit.num_unknown_pressures()))
    chambers = []
    zero = strategy.device.zeros(dh.ndofs)
    for c in coupler.chamber_couplings:
        form = ChamberForm(op.dmesh, _facets_of(dh, c.chamber_surface_setname), c.chamber_volume_method, facet_qpoints)
        V0 = compute_chamber_volume(dh, zero, c.chamber_surface_setname, c.chamber_volume_method)   # create_chamber_tyings :201-202
        chambers.append(ChamberTying(form, c.chamber_volume_method, c.chamber_surface_setname, V0, circuit.get_variable_symbol_index(c.lumped_volume_symbol),
                                     circuit.get_parameter_symbol_index(c.lumped_pressure_symbol), c.pressure_symbol_3D))
    return RSAFDQ2022Function(split, op, ch, chambers, circuit, linear_solver)


class RSAFDQ2022Integrator:
    """LieTrotterGodunov((chamber_solver, circuit_solver)) on an RSAFDQ2022Function, in the reference's order (test_fsi.jl:41-49,
    transfer_operators.jl:181-216): V⁰ᴰ of every chamber ← circuit state; the 3D block by blocked Newton under the HomotopyPathSolver;
    circuit external input ← chamber pressure; the circuit over Δt (integrate_circuit: fixed-step RK4, not the reference's Tsit5)."""

    def __init__(self, f, chamber_solver=None, circuit_substeps=None):
        self.f = f
        self.chamber_solver = chamber_solver or HomotopyPathSolver(NewtonRaphsonSolver(max_iter=10, tol=1e-2, inner_solver="gmres", inner_rtol=1e-10))
        self.circuit_substeps = circuit_substeps
        self.t = 0.0

    def step(self, dt, adaptive=False):
        f = self.f
        for c in f.chambers:                                  # VolumeTransfer0D3D
            c.V0D = float(f.circuit_state[c.volume_index])
        ok = self.chamber_solver.solve(f.u, f.op, f.ch, (self.t, self.t + dt), dt, adaptive=adaptive, system=f.system)
        if not ok:
            return False
        for k, c in enumerate(f.chambers):                    # PressureTransfer3D0D
            f.external_input[c.pressure_index] = f.system.p[k]
        f.circuit_state = f.circuit_model.advance(f.circuit_state, self.t, dt, f.external_input, substeps=self.circuit_substeps)
        self.t += dt
        return True
