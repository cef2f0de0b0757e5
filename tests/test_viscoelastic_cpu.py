"""LinearMaxwellMaterial without a GPU: tb_host_maxwell_eval — the point routine the viscoelastic kernels run, evaluated on the host (closed forms on
the spherical / deviatoric split) — against tests/viscoelastic_reference.py, which solves the local problem as the reference does (6 × 6 Mandel
system, src/modeling/solid/materials.jl:1854-1936).  Relative differences are taken against the largest entry of the compared quantity."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import viscoelastic_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-13   # measured (printed below): tangent 4e-16, state ≤ 2e-14, stress ≤ 5e-14 — the largest at ν = 0.49, where the 6 × 6 system's condition number is ≈ 75


def rel(a, b):
    return float(np.abs(np.asarray(a) - np.asarray(b)).max() / np.abs(b).max())


def host_eval(tb, params, F, Q0, dt):
    dp = C.POINTER(C.c_double)
    params, F, Q0 = (np.ascontiguousarray(x, dtype=np.float64) for x in (params, F, Q0))
    Q1, P, A = np.zeros(6), np.zeros((3, 3)), np.zeros((9, 9))
    rc = tb.lib().tb_host_maxwell_eval(params.ctypes.data_as(dp), len(params), F.ctypes.data_as(dp), Q0.ctypes.data_as(dp), float(dt),
                                       Q1.ctypes.data_as(dp), P.ctypes.data_as(dp), A.ctypes.data_as(dp))
    return rc, Q1, P, A


@pytest.mark.parametrize("nu", [-0.2, 0.0, 0.3, 0.49])
@pytest.mark.parametrize("dt_over_tau", [1e-6, 1.0, 1e6])
def test_point_routine_matches_the_mandel_solve(tb, nu, dt_over_tau):
    ref = R.Maxwell(nu=nu)
    mat = tb.LinearMaxwellMaterial(nu=nu)
    dt = dt_over_tau * ref.tau()
    rng = np.random.default_rng(int(1000 * (nu + 1)) + int(np.log10(dt_over_tau)) + 7)
    for _ in range(5):
        H = rng.uniform(-1e-2, 1e-2, (3, 3))
        Q0 = rng.uniform(-1e-2, 1e-2, 6)
        Q1, P, A = tb.material_routine(mat, np.eye(3) + H, Qknown=Q0, dt=dt)
        rQ, rP, rT = ref.point(H, Q0, dt)
        eQ, eP, eA = rel(Q1, rQ), rel(P, rP), rel(A.reshape(3, 3, 3, 3), rT)
        print("nu %5.2f dt/tau %g: state %.2e stress %.2e tangent %.2e" % (nu, dt_over_tau, eQ, eP, eA))
        assert np.isfinite(Q1).all() and np.isfinite(P).all() and np.isfinite(A).all()
        assert eQ <= TOL and eP <= TOL and eA <= TOL
        # the two limits.  Per part p the relaxed fraction is g = x/(1 + x) with x = a kₚ Δt = (Δt/τ)(1+ν) kₚ, i.e. Δt/τ for the deviatoric part and
        # (Δt/τ)(1+ν)/(1−2ν) for the spherical one; a component moves by g_d·dev + g_v·sph with |dev| ≤ 2m, |sph| ≤ m, m = max|ε| + max|εᵛ₀|
        eps = 0.5 * (H + H.T)
        m = np.abs(Q0).max() + np.abs(eps).max()
        xs = dt_over_tau * np.array([1.0, (1.0 + nu) / (1.0 - 2.0 * nu)])
        if dt_over_tau == 1e-6:      # nothing relaxes: εᵛ₁ → εᵛ₀
            assert np.abs(Q1 - Q0).max() <= 3.0 * (xs / (1.0 + xs)).max() * m
        if dt_over_tau == 1e6:       # everything relaxes: εᵛ₁ → ε and the tangent → E₀ℂ (what is left of the branch: E₁ kₚ/(1 + x) per part)
            left = (1.0 / (1.0 + xs)).max()
            assert np.abs(R.sym_from6(Q1) - eps).max() <= 3.0 * left * m
            assert rel(A.reshape(3, 3, 3, 3), ref.E0 * R.stiffness(nu)) <= 1.01 * left * ref.E1 / ref.E0


def test_tangent_has_the_minor_symmetries_and_matches_central_differences(tb):
    mat = tb.LinearMaxwellMaterial()
    rng = np.random.default_rng(3)
    H, Q0, dt = rng.uniform(-1e-2, 1e-2, (3, 3)), rng.uniform(-1e-2, 1e-2, 6), 0.05
    F = np.eye(3) + H
    _, P, A = tb.material_routine(mat, F, Qknown=Q0, dt=dt)
    A4 = A.reshape(3, 3, 3, 3)
    assert (A4 == A4.transpose(1, 0, 2, 3)).all() and (A4 == A4.transpose(0, 1, 3, 2)).all() and (A4 == A4.transpose(2, 3, 0, 1)).all()
    assert (P == P.T).all()
    h = 1e-4   # σ is linear in F: central differences are exact up to rounding, |σ| ε / h ≈ 1e-9 relative to the tangent
    fd = np.zeros((3, 3, 3, 3))
    for k in range(3):
        for l in range(3):
            dF = np.zeros((3, 3))
            dF[k, l] = h
            fd[:, :, k, l] = (tb.material_routine(mat, F + dF, Qknown=Q0, dt=dt)[1] - tb.material_routine(mat, F - dF, Qknown=Q0, dt=dt)[1]) / (2 * h)
    assert rel(A4, fd) <= 1e-8


def test_purely_elastic_material_keeps_its_state(tb):
    mat = tb.LinearMaxwellMaterial(E1=0.0)
    ref = R.Maxwell(E1=0.0)
    rng = np.random.default_rng(4)
    H, Q0 = rng.uniform(-1e-2, 1e-2, (3, 3)), rng.uniform(-1e-2, 1e-2, 6)
    Q1, P, A = tb.material_routine(mat, np.eye(3) + H, Qknown=Q0, dt=0.1)
    assert (Q1 == Q0).all()
    eps = 0.5 * (H + H.T)
    assert rel(P, ref.E0 * np.einsum("ijkl,kl->ij", ref.C4, eps)) <= TOL
    assert rel(A.reshape(3, 3, 3, 3), ref.E0 * ref.C4) <= TOL


@pytest.mark.parametrize("params", [
    [np.nan, 20e3, 1e3, 1e3, 0.3], [70e3, np.inf, 1e3, 1e3, 0.3], [70e3, 20e3, np.nan, 1e3, 0.3], [70e3, 20e3, 1e3, np.inf, 0.3],
    [70e3, 20e3, 1e3, 1e3, np.nan], [70e3, 20e3, 1e3, 0.0, 0.3], [70e3, 20e3, 1e3, -1.0, 0.3], [-1.0, 20e3, 1e3, 1e3, 0.3],
    [70e3, -1.0, 1e3, 1e3, 0.3], [70e3, 20e3, 1e3, 1e3, -1.0], [70e3, 20e3, 1e3, 1e3, 0.5], [70e3, 20e3, 1e3, 1e3, 0.7], [70e3, 20e3, 1e3, 1e3]])
def test_refused_parameter_sets(tb, params):
    rc, *_ = host_eval(tb, params, np.eye(3), np.zeros(6), 0.1)
    assert rc == tb._lib.TB_ERR_BAD_ARG
    assert tb.lib().tb_last_error_string()


def test_host_entry_refuses_a_non_positive_time_step_and_takes_null_outputs(tb):
    p = tb.LinearMaxwellMaterial().params()
    assert host_eval(tb, p, np.eye(3), np.zeros(6), 0.0)[0] == tb._lib.TB_ERR_BAD_ARG
    dp = C.POINTER(C.c_double)
    F = np.eye(3)
    assert tb.lib().tb_host_maxwell_eval(p.ctypes.data_as(dp), 5, F.ctypes.data_as(dp), None, 0.1, None, None, None) == tb._lib.TB_OK
    with pytest.raises(ValueError):
        tb.material_routine(tb.LinearMaxwellMaterial(), F)


def test_creep_recurrence(tb):
    """ten steps of Δt = 0.1 at ε₁₁ = 0.05 with the default parameters; the end values were computed from the reference's formulas"""
    mat = tb.LinearMaxwellMaterial()
    F = np.eye(3)
    F[0, 0] += 0.05
    Q = np.zeros(6)
    hist = [Q]
    for _ in range(10):
        Q = tb.material_routine(mat, F, Qknown=Q, dt=0.1)[0]
        hist.append(Q)
    hist = np.array(hist)
    assert abs(Q[0] - 0.04999699936779986) <= 1e-14
    assert abs(Q[3] - 1.4999026457761e-06) <= 1e-14 and abs(Q[5] - 1.4999026457761e-06) <= 1e-14
    assert (Q[[1, 2, 4]] == 0.0).all()
    assert (np.diff(hist[:, 0]) >= 0.0).all()
    assert np.abs(hist - R.creep_recurrence(R.Maxwell(), 0.05, 0.1, 10)).max() <= 1e-14


def test_material_keeps_its_name_defaults_and_newmark_refusal(tb):
    m = tb.LinearMaxwellMaterial()
    assert (m.E0, m.E1, m.mu, m.eta1, m.nu) == (70e3, 20e3, 1e3, 1e3, 0.3)
    assert tb.dynamics.LinearMaxwellMaterial is tb.LinearMaxwellMaterial
    with pytest.raises(NotImplementedError):
        tb.dynamics._refuse_unsupported_material(m)


def test_new_entries_are_declared_bound_and_documented(tb):
    header = open(os.path.join(ROOT, "include", "tbhip.h"), encoding="utf-8").read()
    julia = open(os.path.join(ROOT, "julia", "ThunderboltHIPBackend.jl"), encoding="utf-8").read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md"), encoding="utf-8").read()
    for name in ("tb_viscoelastic_create", "tb_host_maxwell_eval"):
        assert name + "(" in header and name in tb._lib.SIGNATURES and ":" + name in julia and name in integration, name
        assert hasattr(tb.lib(), name)
    assert "materials.jl:1816-2008" in integration
    assert int(re.search(r"#define\s+TB_ABI_REVISION\s+(\d+)", header).group(1)) == 10
    assert tb._lib.TB_FORM_VISCOELASTIC == int(re.search(r"TB_FORM_VISCOELASTIC\s*=\s*(\d+)", header).group(1))
