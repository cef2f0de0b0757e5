"""Host side of the 3D-0D chamber coupling: closed forms that pin the NumPy checker (tests/chamber_reference.py), the lumped circulation and
the Schur complement solver on the reference's own two systems (test/test_solver.jl:5-36)."""
import itertools

import numpy as np
import pytest

import chamber_reference as ref


def affine_case():
    a, b, c = 1.3, 0.7, 0.9
    xyz, conn, facets = ref.box_mesh(a, b, c, (2, 1, 2))
    A = np.array([[1.10, 0.05, -0.03], [0.02, 0.93, 0.04], [-0.06, 0.01, 1.07]])
    assert np.linalg.det(A) > 0
    u = (xyz @ (A - np.eye(3)).T).reshape(-1)
    cell_dofs = (3 * conn[:, :, None] + np.arange(3)).reshape(len(conn), -1)
    return (a, b, c), xyz, conn, facets, A, u, cell_dofs


@pytest.mark.parametrize("nq", [1, 2, 3])
def test_closed_forms_on_a_box(nq):
    """All six faces of an a×b×c box under u = (A − I)x with outward normals: RSAFDQ2022 with unit h and any b gives −det(A)·abc (the flux of
    (h·(x' − b)) h through the closed deformed surface), Hirschvogel −3·det(A)·abc (divergence theorem)."""
    (a, b, c), xyz, conn, facets, A, u, cell_dofs = affine_case()
    vol = np.linalg.det(A) * a * b * c
    h = np.array([1.0, 2.0, -0.5]); h /= np.linalg.norm(h)
    for bb in ([0.0, 0.0, -0.1], [0.3, -1.2, 0.8]):
        out = ref.assemble(xyz, conn, cell_dofs, 1, facets, nq, u, 0.0, ref.RSAFDQ2022(h, bb))
        assert abs(out["volume"] + vol) < 1e-13 * vol
    out = ref.assemble(xyz, conn, cell_dofs, 1, facets, nq, u, 0.0, ref.Hirschvogel2017())
    assert abs(out["volume"] + 3.0 * vol) < 1e-13 * vol


def test_col_against_translation_is_the_flux():
    """col summed against a constant translation c equals Σ J F⁻ᵀn₀ · c dΓ; on one face of the affine box that is det(A) A⁻ᵀ n₀ · c · area"""
    (a, b, c), xyz, conn, facets, A, u, cell_dofs = affine_case()
    top = facets[facets[:, 1] == 5]                           # z = c, n₀ = e_z, area a·b
    out = ref.assemble(xyz, conn, cell_dofs, 1, top, 2, u, 0.7, ref.RSAFDQ2022())
    cvec = np.array([0.3, -0.2, 0.9])
    flux = np.linalg.det(A) * (np.linalg.inv(A).T @ np.array([0.0, 0.0, 1.0])) @ cvec * a * b
    assert abs(out["col"] @ np.tile(cvec, len(xyz)) - flux) < 1e-13 * abs(flux)
    assert np.allclose(out["r"], 0.7 * out["col"], rtol=0, atol=1e-15)
    # closed surface: the follower load of a uniform pressure has no resultant
    allf = ref.assemble(xyz, conn, cell_dofs, 1, facets, 2, u, 0.7, ref.RSAFDQ2022())
    assert np.abs(allf["col"].reshape(-1, 3).sum(axis=0)).max() < 1e-14


def test_row_is_the_derivative_of_the_volume():
    """the complex-step row of the checker against a central difference of its own volume (Q2 field on one distorted cell)"""
    rng = np.random.default_rng(3)
    xyz, conn, facets = ref.box_mesh(1.0, 0.8, 0.9)
    xyz = xyz + rng.uniform(-0.08, 0.08, xyz.shape)
    cell_dofs = np.arange(81).reshape(1, 81)
    u = rng.uniform(-0.03, 0.03, 81)
    dirn = rng.uniform(-1, 1, 81)
    for method in (ref.RSAFDQ2022(), ref.Hirschvogel2017()):
        o = ref.assemble(xyz, conn, cell_dofs, 2, facets[:2], 3, u, 0.0, method)
        eps = 1e-6
        vp = ref.assemble(xyz, conn, cell_dofs, 2, facets[:2], 3, u + eps * dirn, 0.0, method)["volume"]
        vm = ref.assemble(xyz, conn, cell_dofs, 2, facets[:2], 3, u - eps * dirn, 0.0, method)["volume"]
        assert abs(o["row"] @ dirn - (vp - vm) / (2 * eps)) < 1e-8 * abs(o["row"] @ dirn)


# ------------------------------------------------------------------------------------------------ circuit
def test_phi_rsafdq2022(tb):
    tC, TC, TR, THB = 100.0, 200.0, 150.0, 800.0
    tR = tC + TC
    phi = lambda t: tb.Φ_RSAFDQ2022(t, tC, tR, TC, TR, THB)
    assert phi(tC) == 0.0 and abs(phi(tC + TC / 2) - 0.5) < 1e-15
    assert abs(phi(tR) - 1.0) < 1e-15 and abs(phi(tR + TR / 2) - 0.5) < 1e-15
    assert abs(phi(tR - 1e-9) - 1.0) < 1e-12                  # continuous across the contraction / relaxation boundary
    assert phi(tR + TR) == 0.0 and phi(tR + TR + 10.0) == 0.0 and phi(50.0) == 0.0
    assert phi(tC + TC / 2 + 3 * THB) == pytest.approx(0.5, abs=1e-12)      # periodic
    assert tb.elastance_RSAFDQ2022(tC + TC / 2, 0.1, 2.0, tC, tR, TC, TR, THB) == pytest.approx(1.1, abs=1e-14)


def test_circuit_conserves_blood(tb):
    m = tb.RSAFDQ2022LumpedCicuitModel()
    assert m.num_states() == 12 and len(m.state_symbols()) == 12 and m.num_unknown_pressures() == 0
    rng = np.random.default_rng(0)
    C = np.array([m.Csysar, m.Csysven, m.Cpular, m.Cpulven])
    for t in (0.0, 60.0, 200.0, 410.0, 650.0):
        u = m.default_initial_state() * rng.uniform(0.7, 1.3, 12) + np.r_[np.zeros(8), rng.uniform(-50, 50, 4)]
        du = m.lumped_driver(np.zeros(12), u, t, ())
        total = du[:4].sum() + (C * du[4:8]).sum()
        assert abs(total) < 1e-12 * np.abs(np.r_[du[:4], C * du[4:8]]).max()
    u0 = m.default_initial_state()
    u1 = tb.integrate_circuit(m, u0, 0.0, 50.0)
    blood = lambda u: u[:4].sum() + (C * u[4:8]).sum()
    assert abs(blood(u1) - blood(u0)) < 1e-11 * blood(u0) and not np.allclose(u1, u0)
    # the fixed-step integrator converges: halving the step changes the state at fourth order
    e1 = np.abs(tb.integrate_circuit(m, u0, 0.0, 50.0, substeps=100) - tb.integrate_circuit(m, u0, 0.0, 50.0, substeps=400)).max()
    assert e1 < 1e-3


def test_pressure_index_rules(tb):
    """lumped.jl:191-261, statement by statement (0-based here): the counter advances for every earlier chamber whose pressure is GIVEN"""
    for lv, rv, la, ra in itertools.product([True, False], repeat=4):
        m = tb.RSAFDQ2022LumpedCicuitModel(lv_pressure_given=lv, rv_pressure_given=rv, la_pressure_given=la, ra_pressure_given=ra)
        assert m.num_unknown_pressures() == [lv, rv, la, ra].count(False)
        assert m.lumped_circuit_relative_lv_pressure_index() == 0
        assert m.lumped_circuit_relative_rv_pressure_index() == int(lv)
        assert m.lumped_circuit_relative_la_pressure_index() == int(lv) + int(rv)
        assert m.lumped_circuit_relative_ra_pressure_index() == int(lv) + int(rv) + int(la)
        for sym, given in (("pₗᵥ", lv), ("pᵣᵥ", rv), ("pₗₐ", la), ("pᵣₐ", ra)):
            if given:
                with pytest.raises(KeyError):
                    m.get_parameter_symbol_index(sym)
    m = tb.RSAFDQ2022LumpedCicuitModel(lv_pressure_given=False)
    assert m.get_parameter_symbol_index("pₗᵥ") == 0 and m.get_variable_symbol_index("Vₗᵥ") == 1 and m.get_variable_symbol_index("Qpulᵥₑₙ") == 11
    with pytest.raises(KeyError):
        m.get_variable_symbol_index("nope")
    d = tb.DummyLumpedCircuitModel(lambda t: 3.0 + t)
    assert d.num_states() == 1 and d.num_unknown_pressures() == 1 and d.get_variable_symbol_index("anything") == 0
    assert d.default_initial_state()[0] == 3.0 and d.lumped_driver(np.zeros(1), np.array([1.0]), 2.0, ())[0] == 4.0


def test_external_lv_pressure_is_used(tb):
    given = tb.RSAFDQ2022LumpedCicuitModel()
    ext = tb.RSAFDQ2022LumpedCicuitModel(lv_pressure_given=False)
    u, t = given.default_initial_state(), 100.0
    E = tb.elastance_RSAFDQ2022(t, given.Epasslv, given.Eactmaxlv, given.tClv, given.tClv + given.TClv, given.TClv, given.TRlv, given.THB)
    plv = E * (u[1] - given.V0lv)
    a = given.lumped_driver(np.zeros(12), u, t, ())
    b = ext.lumped_driver(np.zeros(12), u, t, [plv])
    assert np.array_equal(a, b)
    c = ext.lumped_driver(np.zeros(12), u, t, [plv + 1.0])
    assert c[1] != a[1] and np.array_equal(c[[2, 3, 5, 6, 7]], a[[2, 3, 5, 6, 7]])


# ------------------------------------------------------------------------------------------------ Schur complement solver
def test_schur_solver_on_the_reference_systems(tb):
    """test/test_solver.jl:5-36: the 1 + 1 system with A₂₂ = 0 and a random 5 + 3 system with a full A₂₂"""
    rng = np.random.default_rng(42)
    alg = tb.SchurComplementLinearSolver(lambda A, b: np.linalg.solve(A, b))
    for s1, s2, A in ((1, 1, np.array([[1.0, 1.0], [1.0, 0.0]])), (5, 3, rng.random((8, 8)))):
        b = rng.random(s1 + s2)
        u1, u2, ok = alg.solve(A[:s1, :s1], [A[:s1, s1 + i] for i in range(s2)], [A[s1 + k, :s1] for k in range(s2)], A[s1:, s1:], b[:s1], b[s1:])
        assert ok and np.abs(np.r_[u1, u2] - np.linalg.solve(A, b)).max() < 1e-10
    # a failed inner solve fails the outer solve
    bad = tb.SchurComplementLinearSolver(lambda A, b: (np.zeros_like(b), False))
    assert bad.solve(np.eye(2), [np.ones(2)], [np.ones(2)], None, np.ones(2), np.ones(1))[2] is False


def test_volume_methods_host(tb):
    rng = np.random.default_rng(1)
    x, d, N = rng.random(3), 0.1 * rng.random(3), np.array([0.0, 0.6, 0.8])
    F = np.eye(3) + 0.1 * rng.random((3, 3))
    assert tb.RSAFDQ2022SurrogateVolume().volume_integral(x, d, F, N) == pytest.approx(ref.RSAFDQ2022().volume_integral(x, d, F, N), rel=1e-14)
    assert tb.Hirschvogel2017SurrogateVolume().volume_integral(x, d, F, N) == pytest.approx(ref.Hirschvogel2017().volume_integral(x, d, F, N), rel=1e-14)
    assert tb.ConstantChamberVolume(2.5).volume_integral(x, d, F, N) == 2.5
    assert np.array_equal(tb.RSAFDQ2022SurrogateVolume().params(), [0, 1, 0, 0, 0, -0.1])
