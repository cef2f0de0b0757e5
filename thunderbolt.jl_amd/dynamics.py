"""Elastodynamics M ü + f_int(u) = f_ext by fixed-step Newmark-β integration in displacement form.

  reference (file:line)                                                            here
  ---------------------------------------------------------------------------------------------------------------
  ElastodynamicsModel                    src/modeling/solid_mechanics.jl:30-69      ElastodynamicsModel
  NewmarkSolver                          src/solver/time/newmark.jl:4-47            NewmarkSolver
  NewmarkStageOperator                   newmark.jl:52-139                          NewmarkStageOperator (a DisplacementSystem of nlsolve)
  _consistent_initial_acceleration       newmark.jl:486-533                         NewmarkIntegrator._initial_acceleration
  perform_step!                          newmark.jl:566-604                         NewmarkIntegrator.step
  velocity / acceleration / integrator(t) newmark.jl:238-382                        NewmarkIntegrator.velocity / .acceleration / __call__

The vector mass (tb_assemble_matrix on the 3-component field), the predictor, the inertia stage r += M(u − ũ)/(βΔt²), J += M/(βΔt²), the corrector
and the Hermite interpolant run on the device (csrc/tb_newmark.hip); the wrapped internal-force operator, Newton and the Krylov solves are the
quasi-static stack of solid.py.

State layout.  The reference keeps ONE state vector [d; v] (plus condensed internal variables) and maps the structural numbering into it.  Here the
displacement d, the velocity v and the acceleration a are THREE device vectors in the structural numbering (`.u`, `.v`, `.a` of the integrator);
there is no combined vector and no mapping.

Not in this module (NotImplementedError): condensed internal variables under Newmark (an ActiveStressModel over a sarcomere model with state —
hence also the rate-coupled local problem, which needs the velocity anchor of newmark.jl:535-549), LinearMaxwellMaterial under Newmark (its
quasi-static form is solid.py's), and adaptive stepping
(the Zienkiewicz–Xie error estimate, PIDController and the rollback of the acceleration, newmark.jl:606-698)."""
import numpy as np

from ._lib import check, lib
from .api import (BilinearMassIntegrator, BilinearOperator, ConstantCoefficient, DeviceVector, FieldCoefficient, Hexahedron, _ptr, pcg_solve,
                  solve_converged)
from .solid import (ActiveStressModel, ConstraintHandler, DisplacementSystem, LinearMaxwellMaterial, NewtonRaphsonSolver, NonlinearOperator, PrestressedMechanicalModel,
                    QuasiStaticModel, apply_zero, dot, nlsolve, residual, update_linearization)


class Dirichlet:
    """Dirichlet(field_name, dofs, values): the dofs a condition on the field `field_name` prescribes — in the numbering of that field's DofHandler —
    and their values: None (zero), an array, or a callable t → array (update_constraints!)."""

    def __init__(self, field_name, dofs, values=None):
        self.field_name, self.dofs, self.values = field_name, np.asarray(dofs, dtype=np.int64), values


class ElastodynamicsModel:
    """ElastodynamicsModel(displacement_sym, velocity_sym, material, facet_models, rho) — the 4-argument form has no facet models
    (solid_mechanics.jl:30-59).  The velocity is a field but no Newton unknown: a Dirichlet condition on it is refused."""

    def __init__(self, displacement_symbol, velocity_symbol, material_model, *args):
        if len(args) == 1:
            facet_models, rho = (), args[0]
        elif len(args) == 2:
            facet_models, rho = args
        else:
            raise TypeError("ElastodynamicsModel(displacement_sym, velocity_sym, material, [facet_models,] rho)")
        self.displacement_symbol, self.velocity_symbol = displacement_symbol, velocity_symbol
        self.material_model, self.facet_models = material_model, tuple(facet_models)
        self.rho = rho if isinstance(rho, (ConstantCoefficient, FieldCoefficient)) else ConstantCoefficient(float(rho))

    def quasi_static(self):
        """The internal-force weak form: the QuasiStaticModel the element caches are built from (facet models ride along)."""
        return QuasiStaticModel(self.displacement_symbol, self.material_model, self.facet_models)


def _refuse_unsupported_material(cm):
    inner = cm.inner_model if isinstance(cm, PrestressedMechanicalModel) else cm
    if isinstance(inner, LinearMaxwellMaterial):
        raise NotImplementedError("LinearMaxwellMaterial under Newmark: condensed internal variables are not implemented for elastodynamics")
    if isinstance(inner, ActiveStressModel) and inner.internal_model() is not None:
        raise NotImplementedError("condensed internal variables under Newmark (ActiveStressModel over a sarcomere model with state, and with it the "
                                  "rate-coupled local problem that needs the velocity anchor) are not implemented: use a model without internal state")


class NewmarkSolver:
    """NewmarkSolver(beta=1/4, gamma=1/2, inner_solver=NewtonRaphsonSolver(...)) (newmark.jl:40-47).  The defaults are the average-acceleration
    rule: unconditionally stable, second order, energy conserving; γ > ½ adds numerical dissipation and drops the scheme to first order.  The
    stage tangent K + M/(βΔt²) is symmetric positive definite for the materials here, so the default Newton solves it with Jacobi-CG."""

    def __init__(self, beta=0.25, gamma=0.5, inner_solver=None):
        if not (beta > 0.0 and np.isfinite(beta) and np.isfinite(gamma)):
            raise ValueError("NewmarkSolver: beta must be positive (the displacement form divides by beta dt^2)")
        self.beta, self.gamma = float(beta), float(gamma)
        self.inner_solver = inner_solver if inner_solver is not None else NewtonRaphsonSolver(max_iter=100, tol=1e-4, inner_solver="cg", inner_rtol=1e-10,
                                                                                                inner_maxiter=20000)


class NewmarkStageOperator(DisplacementSystem):
    """NewmarkStageOperator (newmark.jl:52-139) behind nlsolve's `system=` interface: the internal-force operator `op` plus the inertia the scheme
    adds — residual r = f_int(u) + M(u − ũ)/(βΔt²), tangent J = K(u) + M/(βΔt²).  `linearize` calls the wrapped linearisation (or residual), then
    tb_newmark_stage — one pass over M for both terms — then eliminates the constraints.  The only place that knows the scheme's coefficients."""

    def __init__(self, op, M, ch):
        super().__init__(op, ch)
        self.M = M
        self.utilde = op.strategy.device.zeros(op.dh.ndofs)     # ũ of the current step, written once per step
        self.c = 1.0                                            # 1/(βΔt²), overwritten by the first step

    def set_step(self, beta, dt):
        self.c = 1.0 / (beta * dt * dt)

    def add_inertia(self, u, res, tangent):
        check(lib().tb_newmark_stage(self.op.pattern.h, self.M.A.ptr, float(self.c), _ptr(u), self.utilde.ptr, self.op.J.ptr if tangent else None, _ptr(res)))

    def linearize(self, u, res, t, tangent):
        op, ch = self.op, self.ch
        if tangent:
            update_linearization(op, u, t, residual=res)
            self.add_inertia(u, res, True)
            op.J_includes_inertia = True
            apply_zero(op.J, res, ch, pattern=op.pattern)
        else:
            residual(op, res, u, t)                            # the eliminated stage tangent of iteration 0 stays in op.J
            self.add_inertia(u, res, False)
            apply_zero(None, res, ch, pattern=op.pattern)

    def mul(self, out, x):
        """out = (K + M/(βΔt²)) x: the inertia is part of the operator, so it is part of its action (newmark.jl:83-87).  After `linearize` op.J
        already holds the sum; update_linearization clears the operator's `J_includes_inertia` whenever it rewrites J, and the mass product is then
        added here."""
        check(lib().tb_spmv_csr(self.op.pattern.h, self.op.J.ptr, _ptr(x), 1.0, 0.0, _ptr(out)))
        if not getattr(self.op, "J_includes_inertia", False):
            check(lib().tb_spmv_csr(self.op.pattern.h, self.M.A.ptr, _ptr(x), float(self.c), 1.0, _ptr(out)))
        return out


def _cell_density(dh, models):
    """first-order nodal density per cell (n_cells × 8 on hexahedra, × 4 on tetrahedra) of a domain split: each subdomain's constant ρ on its cells"""
    nb1 = 8 if dh.grid.cell_kind == Hexahedron else 4
    data = np.zeros((dh.grid.n_cells, nb1))
    seen = np.zeros(dh.grid.n_cells, dtype=bool)
    for name, m in models.items():
        if not isinstance(m.rho, ConstantCoefficient):
            raise NotImplementedError("a domain split takes one constant density per subdomain")
        cells = np.asarray(dh.grid.getcellset(name))
        data[cells] = float(m.rho.val)
        seen[cells] = True
    if not seen.all():
        raise ValueError("the subdomains of the elastodynamics model do not cover the mesh: %d cells have no density" % int((~seen).sum()))
    return FieldCoefficient(data)


def _copy(dst, src):
    check(lib().tb_memcpy_d2d(dst.dev.h, dst.ptr, src.ptr, src.nbytes))


class NewmarkIntegrator:
    """init(ElastodynamicsProblem(f, u0, v0, tspan), NewmarkSolver(), dt = dt; adaptive = false) in one object.

    model: an ElastodynamicsModel, or a dict cellset-name → ElastodynamicsModel (one material and density per subdomain).  dh / pattern: the
    DofHandler and sparsity pattern of the displacement field; ch: its ConstraintHandler, or a list of Dirichlet conditions (a condition on the
    velocity symbol is refused: the scheme writes the velocity from the converged displacement and would overwrite it).  u0, v0: host arrays in
    the structural numbering (None: zero).

    `.u`, `.v`, `.a` are three device vectors in the structural numbering — NOT the reference's single state vector [d; v]; `.t`, `.tprev` the ends
    of the last step.  step() → bool: a failed Newton returns False and leaves u, v, a and t at the accepted state.  velocity() / acceleration():
    the state at `.t`; with a time, the first / second derivative of the cubic Hermite interpolant through (u, v) at both ends of the last step;
    integrator(t): the interpolated displacement (new device vectors)."""

    def __init__(self, model, dh, pattern, ch, strategy, u0=None, v0=None, tspan=(0.0, 1.0), dt=None, solver=None, adaptive=False, controller=None, qorder=0):
        if adaptive or controller is not None:
            raise NotImplementedError("adaptive Newmark stepping (Zienkiewicz-Xie error estimate, PIDController, rollback of the acceleration) is not "
                                      "implemented: fixed steps only")
        if dt is None or not dt > 0.0:
            raise ValueError("NewmarkIntegrator: a positive step size dt is required")
        models = model if isinstance(model, dict) else {None: model}
        dsyms, vsyms = {m.displacement_symbol for m in models.values()}, {m.velocity_symbol for m in models.values()}
        if len(dsyms) != 1 or len(vsyms) != 1:
            raise ValueError("the subdomains must agree on one displacement and one velocity symbol")
        self.displacement_symbol, self.velocity_symbol = dsyms.pop(), vsyms.pop()
        for m in models.values():
            _refuse_unsupported_material(m.material_model)
        self.ch = self._constraints(dh, ch)
        self.model, self.dh, self.strategy = model, dh, strategy
        self.solver = solver if solver is not None else NewmarkSolver()
        dev = self.dev = strategy.device
        qs = {name: m.quasi_static() for name, m in models.items()}
        self.op = NonlinearOperator(strategy, qs if isinstance(model, dict) else qs[None], dh, pattern, qorder=qorder)
        rho = _cell_density(dh, models) if isinstance(model, dict) else model.rho
        self.M = BilinearOperator(strategy, BilinearMassIntegrator(rho), dh, pattern)
        self.M.update(float(tspan[0]))                         # the mass is constant: assembled once
        self.stage = NewmarkStageOperator(self.op, self.M, self.ch)
        n = self.n = dh.ndofs
        self.t = self.tprev = float(tspan[0])
        self.tend, self.dt = float(tspan[1]), float(dt)
        self._set_values(self.ch, self.t)
        hu0 = np.zeros(n) if u0 is None else np.ascontiguousarray(u0, dtype=np.float64)
        self._applied = hu0[self.ch.prescribed_dofs].copy()     # the prescribed values the accepted displacement carries
        self.u = dev.to_device(hu0)
        self.v = dev.to_device(np.zeros(n) if v0 is None else np.ascontiguousarray(v0, dtype=np.float64))
        self.uprev, self.vprev = dev.zeros(n), dev.zeros(n)
        _copy(self.uprev, self.u)
        _copy(self.vprev, self.v)
        self.vtilde, self._z = dev.zeros(n), dev.zeros(n)
        self.nsteps = 0
        self.a = self._initial_acceleration()

    def _constraints(self, dh, ch):
        if isinstance(ch, ConstraintHandler) or ch is None:
            self._dirichlet = []
            return ch if ch is not None else ConstraintHandler(dh, np.zeros(0, dtype=np.int64))
        conds = list(ch)
        for c in conds:
            if c.field_name == self.velocity_symbol:
                raise ValueError("a Dirichlet condition on the velocity field %r is refused: Newmark reconstructs the velocity from the converged displacement "
                                 "and would overwrite it; prescribe the displacement %r instead" % (c.field_name, self.displacement_symbol))
            if c.field_name != self.displacement_symbol:
                raise ValueError("Dirichlet condition on unknown field %r (fields: %r, %r)" % (c.field_name, self.displacement_symbol, self.velocity_symbol))
        self._dirichlet = conds
        dofs = np.concatenate([c.dofs for c in conds]) if conds else np.zeros(0, dtype=np.int64)
        return ConstraintHandler(dh, dofs)

    def _set_values(self, ch, t):
        """update_constraints!(f, cache, t): the prescribed values at time t (conditions with values that do not depend on t are written once)"""
        for c in self._dirichlet:
            vals = c.values(t) if callable(c.values) else c.values
            if vals is None:
                continue
            pos = np.searchsorted(ch.prescribed_dofs, c.dofs)
            ch.values[pos] = np.broadcast_to(np.asarray(vals, dtype=np.float64), c.dofs.shape)

    def _apply_values(self, vec):
        """apply!(u, ch) on the stage unknowns — a host round trip, made only when the prescribed values differ from the ones the state carries"""
        ch = self.ch
        if len(ch.prescribed_dofs) == 0 or np.array_equal(ch.values, self._applied):
            return
        h = vec.to_host()
        h[ch.prescribed_dofs] = ch.values
        vec.copy_from_host(h)

    def _initial_acceleration(self):
        """M a₀ = f_ext(t₀) − f_int(u₀) with the constraints eliminated on a COPY of M (the stage keeps using M), a₀ = 0 on the prescribed dofs
        (newmark.jl:496-533)."""
        dev, pat = self.dev, self.op.pattern
        rhs = DeviceVector(dev, self.n)
        residual(self.op, rhs, self.u, self.t)
        neg = dev.zeros(self.n)                                 # −(f_int − f_ext)
        check(lib().tb_axpy(dev.h, self.n, -1.0, rhs.ptr, neg.ptr))
        Mc = DeviceVector(dev, self.M.A.n)
        _copy(Mc, self.M.A)
        check(lib().tb_apply_zero_csr(pat.h, Mc.ptr, neg.ptr, self.ch.flags(dev).ptr, 1.0))
        a0 = dev.zeros(self.n)
        self.a0_iterations = 0
        if dot(neg, neg) == 0.0:                                # an equilibrium (or a stress-free start): nothing to solve
            return a0
        its, res = pcg_solve(pat, Mc, neg, a0, rtol=1e-13, atol=0.0, maxiter=10000, precond="jacobi")
        if not solve_converged(pat, res):
            raise RuntimeError("initial acceleration: the mass solve stopped at %d iterations with residual %.3e" % (its, res))
        apply_zero(None, a0, self.ch, pattern=pat)
        self.a0_iterations = its
        return a0

    # ------------------------------------------------------------------------------------------- stepping
    def step(self, dt=None):
        """perform_step! (newmark.jl:566-604): constraints at t + Δt, predictors, Newton on the displacement, corrector."""
        dt = self.dt if dt is None else float(dt)
        beta, gamma = self.solver.beta, self.solver.gamma
        dev, n = self.dev, self.n
        t1 = self.t + dt
        self._set_values(self.ch, t1)
        z = self._z
        _copy(z, self.u)                                        # init_stage!: the Newton starts from uₙ
        self._apply_values(z)
        check(lib().tb_newmark_predict(dev.h, n, dt, beta, gamma, self.u.ptr, self.v.ptr, self.a.ptr, self.stage.utilde.ptr, self.vtilde.ptr))
        self.stage.set_step(beta, dt)
        if not nlsolve(z, self.op, self.ch, self.solver.inner_solver, t=t1, system=self.stage):
            return False                                        # u, v, a, t untouched: the corrector has not run
        _copy(self.uprev, self.u)
        _copy(self.vprev, self.v)
        _copy(self.u, z)
        self._applied = self.ch.values.copy()
        check(lib().tb_newmark_correct(dev.h, n, dt, beta, gamma, self.u.ptr, self.stage.utilde.ptr, self.vtilde.ptr, self.a.ptr, self.v.ptr))
        self.tprev, self.t = self.t, t1
        self.nsteps += 1
        return True

    def solve(self):
        """step to the end of tspan with the fixed step (the last one lands on it) → bool"""
        while self.t < self.tend - 1e-12 * max(1.0, abs(self.tend)):
            h = min(self.dt, self.tend - self.t)
            if self.tend - (self.t + h) < 1e-9 * self.dt:
                h = self.tend - self.t
            if not self.step(h):
                return False
        return True

    # ------------------------------------------------------------------------------------------- read-out
    def _hermite(self, t, D):
        out = DeviceVector(self.dev, self.n)
        dt = self.t - self.tprev
        if dt == 0.0:                                           # before the first step there is no interval: the current state answers any t
            _copy(out, (self.u, self.v, self.a)[D])
            return out
        theta = (float(t) - self.tprev) / dt
        check(lib().tb_hermite_interpolate(self.dev.h, self.n, theta, dt, D, self.uprev.ptr, self.vprev.ptr, self.u.ptr, self.v.ptr, out.ptr))
        return out

    def __call__(self, t):
        """the displacement interpolated to t (interpolate_solution!, newmark.jl:288-289)"""
        return self._hermite(t, 0)

    def velocity(self, t=None):
        return self.v if t is None else self._hermite(t, 1)

    def acceleration(self, t=None):
        """no argument: the scheme's own acceleration at `.t`; with a time: the second derivative of the interpolant, linear over the step and only
        an approximation of the scheme's (newmark.jl:263-268)"""
        return self.a if t is None else self._hermite(t, 2)
