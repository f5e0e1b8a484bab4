"""The reference's own ceremony (mpc.rs:864-888, 959-991: length 8, three players per round) run
through tests/mpc_oracle.py must reproduce the constants the reference asserts
(generator.rs:573-577, 606-611).  This pins the restatement the GPU tests compare against."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import mpc_oracle as mo  # noqa: E402

COMMON_PLAYERS = [(1, 2, 1), (2, 3, 1), (3, 4, 2)]
UNCOMMON_PLAYERS = [(1, 2), (2, 3), (3, 4)]


@pytest.fixture(scope="module")
def ceremony():
    st = mo.initial_common_paramters(8)
    contribs = []
    for player in COMMON_PLAYERS:
        c = mo.mpc_common_paramters_generator(st, player)
        contribs.append((st, c))
        st = mo.verify_common_paramter(st, c, pairings=False)
        assert st is not None
    h1, h2 = mo.h_basis(st, 4)
    matrix = {"front_g1": st.alpha_mul_tau_g1[:3], "front_g2": st.alpha_mul_tau_g2[:3],
              "back_g1": st.beta_mul_tau_g1[:2], "back_g2": st.beta_mul_tau_g2[:2], "h_g1": h1, "h_g2": h2}
    ust = mo.initial_uncommon_paramters(matrix)
    for player in UNCOMMON_PLAYERS:
        c = mo.mpc_uncommon_paramters_generator(ust, player)
        ust = mo.verify_uncommon_paramter(matrix, ust, c, pairings=False)
        assert ust is not None
    return st, ust, matrix, contribs


def test_common_round_constants(ceremony):
    st = ceremony[0]
    assert st.tau_g1[0] == mo.GEN1
    assert st.tau_g1[1] == mo.g1(2)
    assert st.alpha_mul_tau_g1[:2] == [mo.g1(6), mo.g1(12)]
    assert st.beta_mul_tau_g1[:2] == [mo.g1(24), mo.g1(48)]
    assert st.alpha_g1 == mo.g1(6) and st.alpha_g2 == mo.g2(6)
    assert st.beta_g1 == mo.g1(24) and st.beta_g2 == mo.g2(24)
    assert st.tau_g2[7] == mo.g2(2 ** 7)
    assert len(st.tau_g1) == 8


def test_uncommon_round_constants(ceremony):
    st, ust, matrix, _ = ceremony
    assert ust.gamma_g2 == mo.g2(6) and ust.gamma_g1 == mo.g1(6)
    assert ust.delta_g1 == mo.g1(24) and ust.delta_g2 == mo.g2(24)
    # h_i = (tau^(4+i) - tau^i) / delta, kin / gamma, kout / delta
    inv24, inv6 = pow(24, -1, mo.R), pow(6, -1, mo.R)
    assert ust.h_g1 == [mo.g1((2 ** (4 + i) - 2 ** i) * inv24) for i in range(4)]
    assert ust.kin_g1 == [mo.g1(6 * 2 ** i * inv6) for i in range(3)]
    assert ust.kout_g2 == [mo.g2(24 * 2 ** i * inv24) for i in range(2)]


def test_one_contribution_passes_the_pairing_checks(ceremony):
    st, c = ceremony[3][1]  # player 2 against player 1's storage
    assert mo.verify_new_paramter(c.alpha, st.alpha_g1)
    wrong = mo.ParameterPair(mo.g1(5), c.alpha.g2_result, c.alpha.g1_mine, c.alpha.g2_mine)
    assert not mo.verify_new_paramter(wrong, st.alpha_g1)


def test_bytes_layout(ceremony):
    st, ust = ceremony[0], ceremony[1]
    assert len(mo.common_storage_bytes(st)) == 4 + 2 * (96 + 192) + 3 * 8 * (96 + 192)
    assert len(mo.uncommon_storage_bytes(ust)) == 2 * (96 + 192) + 6 * 4 + (3 + 2 + 4) * (96 + 192)
    assert len(ceremony[3][0][1].bytes()) == 2 * 576 + 3 * (4 + 8 * 576)
