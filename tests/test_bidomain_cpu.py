"""Parabolic–elliptic bidomain, the part that needs no device: the dense reference of tests/bidomain_reference.py is validated on its own (symmetry,
definiteness with the ground, the null vector without it, the monodomain limit as an algebraic identity), the model and the stage refuse what they
must before they touch a device, and the new entries stand in the header, the Julia binding and the ctypes table alike."""
import os
import re
import types

import numpy as np
import pytest

import bidomain_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("tb_bidomain_create", "tb_bidomain_destroy", "tb_bidomain_set_matrices", "tb_bidomain_apply", "tb_bidomain_solve", "tb_bidomain_pack",
           "tb_bidomain_unpack")


@pytest.fixture(scope="module")
def systems(tb, oracle):
    """(rowptr, colidx, M, Kᵢ, Kₑ) per mesh from the oracle, computed once"""
    out = {}
    for name in ref.SOLVE_MESHES:
        g, dh, sp = ref.build_mesh(tb, name)
        out[name] = (sp.rowptr, sp.colidx) + ref.oracle_matrices(tb, oracle, g, dh, sp)
    return out


@pytest.mark.parametrize("name", ref.SOLVE_MESHES)
@pytest.mark.parametrize("ground", [(0,), (0, 7, 13)])
def test_reference_matrix_is_symmetric_positive_definite_with_the_ground(systems, name, ground):
    rp, ci, M, Ki, Ke = systems[name]
    A = ref.block_matrix(rp, ci, M, Ki, Ke, ref.DT, ground)
    assert ref.asymmetry(A) <= ref.EPS
    lam = np.linalg.eigvalsh(0.5 * (A + A.T))
    print("%s ground %s: λ_min %.3e  λ_max %.3e  condition %.3e" % (name, ground, lam[0], lam[-1], lam[-1] / lam[0]))
    assert lam[0] > 0.0
    n = len(rp) - 1
    for g in ground:
        e = np.zeros(2 * n)
        e[n + g] = 1.0
        assert np.array_equal(A @ e, ref.ground_diagonal(rp, ci, Ki, Ke, ref.DT) * e)


@pytest.mark.parametrize("name", ref.SOLVE_MESHES)
def test_reference_matrix_without_ground_has_the_null_vector_0_1(systems, name):
    rp, ci, M, Ki, Ke = systems[name]
    A = ref.block_matrix(rp, ci, M, Ki, Ke, ref.DT)
    n = len(rp) - 1
    v = np.concatenate([np.zeros(n), np.ones(n)])
    norm = np.linalg.norm(A, 2)
    assert ref.asymmetry(A) <= ref.EPS
    assert np.linalg.norm(A @ v) <= 1e-12 * norm
    lam = np.linalg.eigvalsh(0.5 * (A + A.T))
    assert abs(lam[0]) <= 1e-12 * norm and lam[1] > 1e-9 * norm          # positive semidefinite, the kernel one-dimensional


@pytest.mark.parametrize("name", ref.SOLVE_MESHES)
@pytest.mark.parametrize("ground", [(0,), (17,)])
def test_monodomain_limit_on_the_reference(tb, oracle, name, ground):
    """κₑ = λκᵢ: Kᵢφₑ = −Kᵢφₘ/(1 + λ), so the φₘ block of the bidomain solve is the monodomain solve with D = λ/(1 + λ)·Dᵢ (λ = 2: ⅔Dᵢ).  A ground
    at ONE vertex does not disturb it: φₑ = −φₘ/(1 + λ) + c solves the eliminated system too, c chosen so that φₑ vanishes there (the block rows sum
    to zero, constants are in the kernel of K).  Several ground vertices pin φₑ = 0 at points where −φₘ/(1 + λ) + c cannot vanish together: the
    identity does not hold then (measured on the hexahedra with the ground (0, 7, 13): 2.4e-3 relative), so the limit is checked with one."""
    g, dh, sp = ref.build_mesh(tb, name)
    M, Ki, Ke = ref.oracle_matrices(tb, oracle, g, dh, sp, kappa_e=2.0 * ref.KAPPA_I)
    assert np.abs(Ke - 2.0 * Ki).max() <= 1e-15 * np.abs(Ki).max()
    n = dh.ndofs
    rng = np.random.default_rng(5)
    phi = rng.uniform(-1.0, 1.0, n)
    A = ref.block_matrix(sp.rowptr, sp.colidx, M, Ki, Ke, ref.DT, ground)
    b = np.concatenate([ref.dense_of_csr(sp.rowptr, sp.colidx, M) @ phi, np.zeros(n)])
    x = np.linalg.solve(A, b)
    mono = np.linalg.solve(ref.heat_matrix(sp.rowptr, sp.colidx, M, (2.0 / 3.0) * Ki, ref.DT), b[:n])
    err = np.linalg.norm(x[:n] - mono)
    print("%s ground %s: |phi_m(bidomain) - phi_m(monodomain, 2/3 D_i)| = %.3e  (|phi_m| = %.3e), max |phi_e| = %.3e" % (name, ground, err, np.linalg.norm(mono),
                                                                                                                        np.abs(x[n:]).max()))
    assert err <= 1e-10 * np.linalg.norm(mono)
    assert np.all(x[n + np.asarray(ground)] == 0.0)


def test_model_takes_the_reference_fields_in_the_reference_order(tb):
    ion, stim = tb.FHNModel(), tb.NoStimulationProtocol()
    ki, ke = tb.ConstantCoefficient(ref.KAPPA_I), tb.ConstantCoefficient(ref.KAPPA_E)
    m = tb.ParabolicEllipticBidomainModel(tb.ConstantCoefficient(2.0), tb.ConstantCoefficient(0.5), ki, ke, stim, ion)
    assert (m.chi.val, m.Cm.val, m.kappa_i, m.kappa_e, m.stim, m.ion) == (2.0, 0.5, ki, ke, stim, ion)
    assert (m.transmembrane_solution_symbol, m.extracellular_solution_symbol, m.internal_state_symbol) == ("φₘ", "φₑ", "s")
    m2 = tb.ParabolicEllipticBidomainModel(1.0, 1.0, ki, ke, stim, ion, phi_m_symbol="v", phi_e_symbol="ue", state_symbol="w")
    assert (m2.transmembrane_solution_symbol, m2.extracellular_solution_symbol, m2.internal_state_symbol) == ("v", "ue", "w")
    Di, De = m.diffusivities()
    assert isinstance(Di, tb.ConductivityToDiffusivityCoefficient) and Di.conductivity is ki and De.conductivity is ke
    with pytest.raises(ValueError, match="kappa_e"):
        tb.ParabolicEllipticBidomainModel(1.0, 1.0, ki, None, stim, ion)


def test_stage_refusals_that_need_no_device(tb):
    strategy = types.SimpleNamespace(device=None, code=0)
    g = tb.generate_mesh(tb.Hexahedron, (2, 2, 2))
    D = tb.ConstantCoefficient(ref.KAPPA_I)
    with pytest.raises(ValueError, match="ground"):
        tb.BidomainBackwardEulerStage(tb.BackwardEulerSolver(), strategy, tb.DofHandler(g), D, D, [])
    with pytest.raises(ValueError, match="ground"):
        tb.BidomainBackwardEulerStage(tb.BackwardEulerSolver(), strategy, tb.DofHandler(g), D, D, None)
    with pytest.raises(NotImplementedError, match="first-order"):
        tb.BidomainBackwardEulerStage(tb.BackwardEulerSolver(), strategy, tb.DofHandler(g, tb.LagrangeCollection(2)), D, D, [0])


def test_unbalanced_extracellular_current_names_its_sum(tb):
    tb.bidomain.check_balanced(np.array([0.0, 1.5, 0.0, -1.5]))
    tb.bidomain.check_balanced(np.zeros(4))
    with pytest.raises(ValueError, match=r"sums to 0\.5"):
        tb.bidomain.check_balanced(np.array([0.0, 1.5, 0.0, -1.0]))
    with pytest.raises(ValueError, match="sums to"):
        tb.bidomain.check_balanced(np.array([1.0, -1.0 + 1e-9]))
    with pytest.raises(ValueError):
        tb.bidomain.check_balanced(np.array([1.0, np.nan]))


def test_entries_stand_in_header_julia_binding_and_ctypes(tb):
    header = open(os.path.join(ROOT, "include", "tbhip.h"), encoding="utf-8").read()
    julia = open(os.path.join(ROOT, "julia", "ThunderboltHIPBackend.jl"), encoding="utf-8").read()
    makefile = open(os.path.join(ROOT, "thunderbolt.jl_amd", "csrc", "Makefile"), encoding="utf-8").read()
    for name in ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert "(:%s, libtbhip)" % name in julia, name
        assert name in tb._lib.SIGNATURES, name
    assert "tb_bidomain.hip" in makefile
    assert int(re.search(r"#define\s+TB_ABI_REVISION\s+(\d+)", header).group(1)) == 10 and tb._lib.TB_ABI_REVISION == 10
