"""The algebraic block cycle of the bidomain system, on the host alone: what the SciPy restatement (bidomain_amg_reference) promises of the method on
9³ Q1 boxes — Kᵢ = diag(1, .2, .2), Kₑ = diag(1, .5, .5) and an isotropic variant, Δt ∈ {0.1, 1, 10}, the ground one vertex, two vertices or a whole face."""
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import amg_reference as aref
import bidomain_amg_reference as bar

N = 9
CASES = list(itertools.product(sorted(bar.TENSORS), bar.DTS, bar.GROUNDS))
_cache = {}


def case(tensor, dt, ground):
    """the system, its hierarchy (max_coarse = 32: three levels) and the cycle, built once per case and left unchanged"""
    key = (tensor, dt, ground)
    if key not in _cache:
        A, pattern, flags = bar.box_system(N, bar.TENSORS[tensor], dt, ground)
        levels = bar.hierarchy(A, pattern, max_coarse=32)
        _cache[key] = dict(A=A, pattern=pattern, flags=flags, levels=levels, cycle=bar.Cycle(levels, flags))
    return _cache[key]


@pytest.mark.parametrize("tensor,dt,ground", CASES)
def test_levels_are_positive_definite_and_the_coarse_planes_are_what_the_method_states(tensor, dt, ground):
    c = case(tensor, dt, ground)
    levels, flags = c["levels"], c["flags"]
    assert len(levels) >= 2
    scalar = aref.hierarchy(bar.auxiliary(c["A"], c["pattern"]), None, max_coarse=32)
    assert len(scalar) == len(levels)
    for l, lev in enumerate(levels):
        Ad = lev["A"].toarray()
        assert np.linalg.eigvalsh(0.5 * (Ad + Ad.T))[0] > 0.0, "level %d is not positive definite" % l
        a11, a12, a21, a22 = bar.planes_of(lev["A"], lev["pattern"])
        # nothing of the block operator lies outside the scalar level pattern
        assert abs(bar.from_planes(lev["pattern"][0], lev["pattern"][1], (a11, a12, a21, a22)) - lev["A"]).max() == 0.0
        # the φₑφₑ plane IS the scalar hierarchy's level matrix: same terms, same order
        assert np.array_equal(a22, scalar[l]["A"].data)
        if l > 0:
            n = len(lev["pattern"][0]) - 1
            B12 = lev["A"][:n, n:]
            assert abs(B12 - B12.T).max() <= 4 * np.finfo(float).eps * abs(B12).max()
            assert np.allclose(a12, a21, rtol=0, atol=4 * np.finfo(float).eps * np.abs(a12).max())
    # grounded nodes are outside every aggregate, their rows of P are empty, and nothing of theirs reaches a coarse plane
    assert (levels[0]["agg"][flags] == -1).all()
    assert np.diff(levels[0]["P"].indptr)[flags].max() == 0


@pytest.mark.parametrize("tensor,dt,ground", CASES)
def test_the_cycle_is_symmetric_and_leaves_grounded_phi_e_at_zero(tensor, dt, ground):
    c = case(tensor, dt, ground)
    cyc, flags, n = c["cycle"], c["flags"], len(c["flags"])
    rng = np.random.default_rng(7)
    u, v = rng.normal(size=2 * n), rng.normal(size=2 * n)
    zu, zv = cyc(u), cyc(v)
    asym = abs(u @ zv - v @ zu) / abs(u @ zv)
    print(tensor, dt, ground, "|u.M^-1 v - v.M^-1 u| / |u.M^-1 v| = %.2e" % asym)
    assert asym <= 5e-14                                                    # observed on these 18 systems: 1.3e-16 … 3.1e-14
    assert (zu[n:][flags] == 0.0).all() and (zv[n:][flags] == 0.0).all()


@pytest.mark.parametrize("tensor,dt,ground", CASES)
def test_fewer_iterations_than_block_jacobi(tensor, dt, ground):
    c = case(tensor, dt, ground)
    A, flags, n = c["A"], c["flags"], len(c["flags"])
    b = np.random.default_rng(3).normal(size=2 * n)
    b[n:][flags] = 0.0
    x, it_amg = bar.pcg(A, b, c["cycle"], rtol=1e-8)
    _, it_jac = bar.pcg(A, b, bar.block_jacobi(A), rtol=1e-8)
    print(tensor, dt, ground, "levels", [len(l["pattern"][0]) - 1 for l in c["levels"]], "AMG", it_amg, "block-Jacobi", it_jac)
    assert np.linalg.norm(b - A @ x) <= 1e-8 * np.linalg.norm(b)
    assert it_amg < it_jac and it_amg <= 25


def test_ground_diag_never_reaches_a_coarse_plane():
    A, pattern, flags = bar.box_system(N, bar.TENSORS["aniso"], 1.0, "face")
    rows = np.repeat(np.arange(N ** 3), np.diff(pattern[0]))
    planes = bar.planes_of(A, pattern)
    planes[3] = planes[3].copy()
    planes[3][(rows == pattern[1]) & flags[rows]] *= 1000.0
    A2 = bar.from_planes(pattern[0], pattern[1], planes)
    l1 = bar.hierarchy(A, pattern, max_coarse=32)
    l2 = bar.hierarchy(A2, pattern, lam_scalar=[lev["lam"] for lev in l1[:-1]], max_coarse=32)   # (the same ω: an eigenvalue solver's last bits are its own)
    assert len(l1) == len(l2) >= 2
    for a, b in zip(l1[1:], l2[1:]):
        assert abs(a["A"] - b["A"]).max() == 0.0
