"""tests/mpc_structure_model.py against masks derived by hand from the equations of
bh_mpc_common_check, and the properties of the rho^i weights the soundness
argument rests on.  Integers mod r only."""
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mpc_structure_model as sm  # noqa: E402

R = sm.R
TAU, ALPHA, BETA = (0x5AB3F1C2D4E6978877665544332211FFEEDDCCBBAA99887766554433221100FF % R,
                    0x6F0E1D2C3B4A59687786A5B4C3D2E1F00112233445566778899AABBCCDDEEFF1 % R,
                    0x1234567890ABCDEF1122334455667788)
RHO = 0x2B7E151628AED2A6ABF7158809CF4F3C762E7160F38B4DA56A784D9045190CFE % R
N = 8


def _rhos(count, seed=20250107):
    rng = random.Random(seed)
    return [rng.randrange(1, R) for _ in range(count)]


def expected_bits(name, i, n):
    """The equations a change of one element (by a nonzero amount) breaks.  By hand:
    tau_g1[i] enters L (i < n-1) and R (i >= 1) with different weights, S(tau_g1), and through it the
    right-hand sides of equations 5 and 7; tau_g2[i] enters S(tau_g2), and element 1 is the G2 factor
    of equation 3; a G1 alpha_mul_tau element is the left-hand side of 5 and 6, a G2 one the right-hand
    side of 6; alpha_g2 is in 1 and the right-hand side of 5, alpha_g1 in 1 only; beta likewise.
    Element 0 of the tau pair is also compared with the generator."""
    if name == "tau_g1":
        return sm.POWERS | sm.TAU_G2 | sm.ALPHA_TAU | sm.BETA_TAU | (sm.FIRST if i == 0 else 0)
    if name == "tau_g2":
        return sm.TAU_G2 | (sm.FIRST if i == 0 else 0) | (sm.POWERS if i == 1 and n >= 2 else 0)
    return {"alpha_mul_tau_g1": sm.ALPHA_TAU | sm.ALPHA_TAU_G2, "alpha_mul_tau_g2": sm.ALPHA_TAU_G2,
            "beta_mul_tau_g1": sm.BETA_TAU | sm.BETA_TAU_G2, "beta_mul_tau_g2": sm.BETA_TAU_G2,
            "alpha_g1": sm.ALPHA, "alpha_g2": sm.ALPHA | sm.ALPHA_TAU,
            "beta_g1": sm.BETA, "beta_g2": sm.BETA | sm.BETA_TAU}[name]


def changed(s, name, i, delta):
    t = {k: (list(v) if isinstance(v, list) else v) for k, v in s.items()}
    if name in sm.POINTS:
        t[name] = (t[name] + delta) % R
    else:
        t[name][i] = (t[name][i] + delta) % R
    return t


@pytest.mark.parametrize("n", [0, 1, 2, 3, 8, 257])
def test_honest_logs_pass(n):
    assert sm.check_mask(sm.well_formed(n), RHO) == 0  # the initial storage
    s = sm.well_formed(n, TAU, ALPHA, BETA)
    assert sm.check_mask(s, RHO) == 0
    assert sm.check_mask(s, 1) == 0 and sm.check_mask(s, R - 1) == 0
    new, mine = sm.contribute(s, 3, BETA, ALPHA)
    assert new == sm.well_formed(n, TAU * ALPHA % R, ALPHA * 3 % R, BETA * BETA % R)
    assert sm.verify_mask(s, new, mine, RHO) == 0


@pytest.mark.parametrize("name", sm.VECTORS)
@pytest.mark.parametrize("i", [0, 1, 4, 7])
def test_one_vector_element(name, i):
    s = sm.well_formed(N, TAU, ALPHA, BETA)
    assert sm.check_mask(changed(s, name, i, 1), RHO) == expected_bits(name, i, N)
    assert sm.check_mask(changed(s, name, i, R - 12345), RHO) == expected_bits(name, i, N)


@pytest.mark.parametrize("name", sm.POINTS)
def test_one_point(name):
    s = sm.well_formed(N, TAU, ALPHA, BETA)
    assert sm.check_mask(changed(s, name, None, 7), RHO) == expected_bits(name, None, N)
    # length 0 evaluates the point equations only
    assert sm.check_mask(changed(sm.well_formed(0, TAU, ALPHA, BETA), name, None, 7), RHO) == \
        expected_bits(name, None, 0) & (sm.ALPHA | sm.BETA)


def test_short_lengths():
    s = sm.well_formed(1, TAU, ALPHA, BETA)
    assert sm.check_mask(changed(s, "tau_g1", 0, 1), RHO) == sm.FIRST | sm.TAU_G2 | sm.ALPHA_TAU | sm.BETA_TAU
    s = sm.well_formed(2, TAU, ALPHA, BETA)
    # tau_g1[1] is all of R, tau_g2[1] the factor of L = tau_g1[0]
    assert sm.check_mask(changed(s, "tau_g1", 1, 1), RHO) == sm.POWERS | sm.TAU_G2 | sm.ALPHA_TAU | sm.BETA_TAU
    assert sm.check_mask(changed(s, "tau_g2", 1, 1), RHO) == sm.POWERS | sm.TAU_G2


def test_no_defect_is_masked_under_random_rho():
    """100 seeded draws: every single-element change shows in exactly the bits derived by hand."""
    s = sm.well_formed(N, TAU, ALPHA, BETA)
    rng = random.Random(99)
    for rho in _rhos(100):
        name = rng.choice(sm.VECTORS + sm.POINTS)
        i = rng.randrange(N)
        delta = rng.randrange(1, R)
        assert sm.check_mask(changed(s, name, i, delta), rho) == expected_bits(name, i, N), (name, i, hex(rho))


def cancelling_pair(s, name, j, k, delta, rho):
    """s with name[j] += delta and name[k] -= delta rho^(j-k): the two defects cancel in S(name) under
    this rho and under no other weight base (up to the roots of one polynomial)."""
    t = changed(s, name, j, delta)
    return changed(t, name, k, -delta * pow(rho, j - k, R) % R)


def test_cancelling_pair_passes_for_its_rho_only():
    s = sm.well_formed(N, TAU, ALPHA, BETA)
    for j, k in ((5, 2), (2, 5), (7, 0)):
        t = cancelling_pair(s, "alpha_mul_tau_g2", j, k, 0xD1FF, RHO)
        assert sm.check_mask(t, RHO) == 0
        assert sm.check_mask(t, RHO + 1) == sm.ALPHA_TAU_G2
        for rho in _rhos(20, seed=j):
            assert sm.check_mask(t, rho) == sm.ALPHA_TAU_G2


def test_rho_one_is_blind_to_opposite_defects():
    """Why rho must be random: with rho = 1 all weights are equal and any +d, -d pair cancels."""
    s = sm.well_formed(N, TAU, ALPHA, BETA)
    for name, bit in (("tau_g2", sm.TAU_G2), ("alpha_mul_tau_g2", sm.ALPHA_TAU_G2), ("beta_mul_tau_g2", sm.BETA_TAU_G2)):
        for j, k, d in ((2, 6, 1), (7, 3, R - 99), (4, 5, TAU)):
            t = changed(changed(s, name, j, d), name, k, -d)
            assert sm.check_mask(t, 1) == 0
            assert sm.check_mask(t, RHO) == bit


def test_verify_mask():
    old = sm.well_formed(N, TAU, ALPHA, BETA)
    new, mine = sm.contribute(old, 5, 7, RHO)
    assert sm.verify_mask(old, new, mine, RHO) == 0
    # the three "mine" elements that are read, one bit each; no other element of the lists is
    for name, bit in (("alpha_g2", sm.ALPHA_RATIO), ("beta_g2", sm.BETA_RATIO)):
        assert sm.verify_mask(old, new, changed(mine, name, None, 1), RHO) == bit
    assert sm.verify_mask(old, new, changed(mine, "tau_g2", 1, 1), RHO) == sm.TAU_RATIO
    for name in sm.VECTORS:
        for i in range(N):
            if (name, i) != ("tau_g2", 1):
                assert sm.verify_mask(old, new, changed(mine, name, i, 1), RHO) == 0
    assert sm.verify_mask(old, new, changed(mine, "alpha_g1", None, 1), RHO) == 0
    # results: the check's bits, and the ratio the element is part of
    assert sm.verify_mask(old, changed(new, "alpha_g1", None, 1), mine, RHO) == sm.ALPHA | sm.ALPHA_RATIO
    assert sm.verify_mask(old, changed(new, "beta_g1", None, 1), mine, RHO) == sm.BETA | sm.BETA_RATIO
    assert sm.verify_mask(old, changed(new, "tau_g1", 1, 1), mine, RHO) == expected_bits("tau_g1", 1, N) | sm.TAU_RATIO
    # a short vector: the length bit alone, whatever else is wrong
    short = dict(new, beta_mul_tau_g1=new["beta_mul_tau_g1"][:-1], alpha_g1=0)
    assert sm.verify_mask(old, short, mine, RHO) == sm.LENGTHS
    assert sm.verify_mask(old, new, dict(mine, tau_g1=mine["tau_g1"] + [1]), RHO) == sm.LENGTHS


def test_factors_that_are_no_powers():
    """What bh_mpc_common_verify lets through: tau results k_i * old_i with a consistent "mine" list."""
    old = sm.well_formed(N, TAU, ALPHA, BETA)
    ks = [1, 5, 6, 7, 8, 9, 10, 11]
    new, mine = sm.contribute(old, 5, 7, 5, factors=ks)
    assert all(new["tau_g1"][i] == old["tau_g1"][i] * mine["tau_g2"][i] % R for i in range(N))
    mask = sm.verify_mask(old, new, mine, RHO)
    assert mask & sm.POWERS and not mask & (sm.FIRST | sm.TAU_G2 | sm.TAU_RATIO | sm.ALPHA_RATIO | sm.BETA_RATIO)
    assert mask == sm.POWERS | sm.ALPHA_TAU | sm.BETA_TAU
