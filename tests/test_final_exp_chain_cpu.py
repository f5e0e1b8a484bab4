"""The final exponentiation chain of csrc/final_exp_chain.h on the host
(bh_selftest_final_exponentiation_chain: the program and constants that the device kernel
k_fexp_steps interprets) against bh_final_exponentiation, the square-and-multiply ladder over
(p^12 - 1) / r, on chosen and random values; and the chain's exponent identity in Python integers.
Every comparison is an equality.  The same values go to the device in tests/test_gpu_final_exp.py."""
import pytest

import proof_cases as pc
from oracle import pairing as pr

from final_exp_values import C, ONE, P, R, SPECIAL, X, ZERO, call, chain, golden_miller_values, ladder, random_values, \
    special_values, to_bytes


def test_exponent_identity_in_integers():
    assert (X - 1) ** 2 % 3 == 0 and C == (X - 1) ** 2 // 3          # c is an integer
    assert C.bit_length() == 126 and bin(C).count("1") == 48
    assert (P ** 4 - P ** 2 + 1) % R == 0
    h = (P ** 4 - P ** 2 + 1) // R
    assert C * (X + P) * (X * X + P * P - 1) + 1 == h
    assert (P ** 12 - 1) % R == 0 and (P ** 12 - 1) // R == (P ** 6 - 1) * (P ** 2 + 1) * h
    assert P % 6 == 1                                                 # the Frobenius constants' exponents are integers


@pytest.mark.parametrize("name", SPECIAL)
def test_chain_equals_the_ladder_on_chosen_values(name):
    value = dict(special_values())[name]
    want = ladder(to_bytes(value))
    assert chain(value) == want
    if name in ("one", "only_c0", "only_c0_real"):
        assert want == ONE
    if name == "zero":
        assert want == ZERO


def test_chain_equals_the_ladder_on_random_values():
    for v in random_values(12):
        assert chain(v) == ladder(to_bytes(v))


def test_chain_is_multiplicative_on_miller_values():
    """the final exponentiation of a product is the product of the final exponentiations"""
    f, g = golden_miller_values()
    assert chain(pr.f12_mul(f, g)) == pr.f12_mul(chain(f), chain(g))


def test_chain_rejects_a_coefficient_equal_to_p():
    bad = [(0, 0)] * 4 + [(0, P)] + [(0, 0)]
    assert call("bh_selftest_final_exponentiation_chain", bad)[0] == pc.INVALID_ENCODING
    assert call("bh_final_exponentiation", bad)[0] == pc.INVALID_ENCODING
