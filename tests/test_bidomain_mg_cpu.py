"""The multigrid preconditioner of the bidomain block system, the part that needs no device: the NumPy restatement of tests/bidomain_mg_reference.py is
held to the properties the device code is later compared against — symmetric positive definite coarse operators under every ground, a symmetric positive
cycle, a coarse φₘφₑ block that really is unsymmetric when a grounded vertex is no coarse vertex, and fewer iterations than block-Jacobi."""
import numpy as np
import pytest

import bidomain_mg_reference as ref

DEGREE, RATIO = 2, 4.0


@pytest.fixture(scope="module")
def problems(tb, oracle):
    cache = {}

    def get(name, kind):
        if name not in cache:
            cache[name] = ref.build_problem(tb, oracle, name)
        if (name, kind) not in cache:
            lv = ref.reference_levels(cache[name], kind)
            lv["lmax"] = [None if v is None else 1.05 * v for v in ref.lambda_stars(lv["As"], lv["gs"])]   # what the set-up aims at: the eigenvalue inflated by 5 %
            cache[name, kind] = lv
        return cache[name], cache[name, kind]
    return get


CASES = [(m, g) for m in ref.MESHES for g in ref.GROUNDS]


@pytest.mark.parametrize("name,kind", CASES)
def test_coarse_operators_are_symmetric_positive_definite(problems, name, kind):
    _, lv = problems(name, kind)
    for l, A in enumerate(lv["As"][:-1]):
        asym = np.abs(A - A.T).max() / np.abs(A).max()
        lam = np.linalg.eigvalsh(0.5 * (A + A.T))
        print("%s ground %s level %d (%d unknowns): asymmetry %.2e, lambda_min %.3e, lambda_max %.3e" % (name, kind, l, len(A), asym, lam[0], lam[-1]))
        assert asym <= 1e-14 and lam[0] > 0.0
        n = len(lv["gs"][l])
        for g in np.flatnonzero(lv["gs"][l]):                                  # an eliminated φₑ: the diagonal alone
            assert np.count_nonzero(A[n + g]) == 1 and np.count_nonzero(A[:, n + g]) == 1 and A[n + g, n + g] > 0.0


@pytest.mark.parametrize("name", list(ref.MESHES))
def test_off_coarse_ground_makes_the_coarse_coupling_block_unsymmetric(problems, name):
    """Pᵀ A₁₂ G_f P G_c is no symmetric n × n matrix when a grounded fine vertex is no coarse vertex — so the fine level's one a₁₂ plane cannot serve a
    coarse level; with the ground on coarse vertices alone the block stays symmetric on these meshes' first coarse level"""
    def coupling_asymmetry(kind):
        _, lv = problems(name, kind)
        A = lv["As"][-2]
        n = len(A) // 2
        return np.abs(A[:n, n:] - A[:n, n:].T).max() / np.abs(A[:n, n:]).max(), lv["gs"][-2].any()
    off, any_coarse = coupling_asymmetry("off_coarse")
    print("%s: |A12 - A12^T| / |A12| on the first coarse level: off-coarse ground %.3e" % (name, off))
    assert not any_coarse                                          # neither grounded vertex survives on the coarse level
    assert off > 1e-3


@pytest.mark.parametrize("name,kind", CASES)
def test_cycle_is_symmetric_and_positive(problems, name, kind):
    _, lv = problems(name, kind)
    cyc = ref.Cycle(lv["As"], lv["Ps"], lv["gs"], lv["lmax"], DEGREE, RATIO)
    rng = np.random.default_rng(31)
    n2 = len(lv["A"])
    u, v = rng.normal(size=n2), rng.normal(size=n2)
    mu, mv = cyc(u), cyc(v)
    asym = abs(u @ mv - v @ mu) / abs(u @ mv)
    print("%s ground %s: u.M^-1 v = %.15e, v.M^-1 u = %.15e, relative difference %.2e, u.M^-1 u = %.3e" % (name, kind, u @ mv, v @ mu, asym, u @ mu))
    assert asym <= 1e-12 and u @ mu > 0.0 and v @ mv > 0.0
    assert np.all(mu[n2 // 2 + lv["ground"]] == 0.0)


@pytest.mark.parametrize("name,kind", CASES)
def test_multigrid_pcg_needs_fewer_iterations_than_block_jacobi(problems, name, kind):
    _, lv = problems(name, kind)
    A = lv["A"]
    n2 = len(A)
    b = np.random.default_rng(32).uniform(-1.0, 1.0, n2)
    b[n2 // 2 + lv["ground"]] = 0.0
    cyc = ref.Cycle(lv["As"], lv["Ps"], lv["gs"], lv["lmax"], DEGREE, RATIO)
    x_mg, it_mg = ref.pcg(A, b, cyc, 1e-10, 500)
    x_bj, it_bj = ref.pcg(A, b, ref.block_jacobi(A, lv["gs"][-1]), 1e-10, 5000)
    print("%s ground %s: multigrid PCG %d iterations, block-Jacobi PCG %d" % (name, kind, it_mg, it_bj))
    assert np.linalg.norm(b - A @ x_mg) <= 1e-10 * np.linalg.norm(b) * 1.01 and np.linalg.norm(b - A @ x_bj) <= 1e-10 * np.linalg.norm(b) * 1.01
    assert it_mg < it_bj
