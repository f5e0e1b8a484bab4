"""tests/qap_cases.py against the oracle alone (no GPU): every spec reaches the values it prescribes,
the oracle's Parameters have the lengths those values imply (-1 kept, 0 filtered, an aux e = 0
refused), and the limb model of fe_is_zero accepts what csrc/field.cuh documents."""
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import qap_cases as qc  # noqa: E402

R, P = qc.R, qc.P


# ------------------------------------------------------------------ 1. the specs reach their targets
@pytest.mark.parametrize("which", ["full", "fork"])
@pytest.mark.parametrize("name", sorted(qc.ALL))
def test_spec_reaches_its_targets(name, which):
    toxic = qc.toxic_of(which)
    spec = qc.ALL[name]
    pre = qc.prescribe(toxic["tau"], toxic, spec)
    lag = qc.lagrange(toxic["tau"], spec["nc"] + spec["ni"])
    u, v, w = qc.eval_columns(pre.circuit, lag)
    assert (u, v, w) == (pre.u, pre.v, pre.w)
    ni = spec["ni"]
    for j in range(ni + spec["na"]):
        for key, got in (("u", u), ("v", v)):
            t = spec[key][j][0]
            if t is not None:
                assert got[j] == qc.target(t), (key, j)
        k_inv = qc.inv(toxic["gamma"] if j < ni else toxic["delta"])
        e = (toxic["beta"] * u[j] + toxic["alpha"] * v[j] + w[j]) * k_inv % R
        assert e == qc.target(spec["e"][j][0]) == pre.e[j], ("e", j)


def test_ways_give_the_column_lengths_they_name():
    """empty: no term; zero_coeff and one: one; two: two rows; segments: S + 1; long: S S + 1 (an
    input's A column has the appended row's term on top, which the library adds)."""
    S = qc.SEGMENT
    want = {"empty": 0, "zero_coeff": 1, "one": 1, "two": 2, "segments": S + 1, "long": S * S + 1}
    seen = set()
    for spec in qc.ALL.values():
        pre = qc.prescribe(qc.FULL["tau"], qc.FULL, spec)
        for key, M in (("u", pre.circuit.A), ("v", pre.circuit.B), ("e", pre.circuit.C)):
            for (t, way), col in zip(spec[key], M):
                assert len(col) == want[way]
                if way == "two":
                    assert col[0][1] != col[1][1]
                if way == "zero_coeff":
                    assert col[0][0] == 0
                seen.add((key, t if isinstance(t, str) else "small", way))
    # what the issue lists: 0 by every way, -1 by every non-empty way, for u, v and e
    for key in ("u", "v"):
        assert {w for k, t, w in seen if k == key and t == "0"} >= set(qc.WAYS) - {"one"}  # (0 by "one" is zero_coeff)
    assert {w for k, t, w in seen if k == "e" and t == "0"} >= set(qc.NONEMPTY) | {"empty"}
    for key in ("u", "v", "e"):
        assert {w for k, t, w in seen if k == key and t == "-1"} == set(qc.NONEMPTY)
        assert {t for k, t, w in seen if k == key} >= set(qc.TARGETS)


def test_rotation_puts_every_target_at_every_place():
    for place in range(4):
        for key, lists in (("u", (qc.COMBOS_INPUT_U, qc.COMBOS)), ("v", (qc.COMBOS, qc.COMBOS)),
                           ("e", (qc.COMBOS_E_INPUT, qc.COMBOS_E_AUX))):
            got = set()
            for k in range(qc.ROTATIONS):
                spec = qc.SPECS[f"rot{k:02d}"]
                j = (0, spec["ni"] - 1, spec["ni"], spec["ni"] + spec["na"] - 1)[place]
                got.add(spec[key][j])
            assert got == set(lists[place >= 2]), (key, place)
    assert {qc.SPECS[f"rot{k:02d}"]["nc"] + qc.SPECS[f"rot{k:02d}"]["ni"] for k in range(qc.ROTATIONS)} == {7, 15}


def test_lanes260_straddles_the_block_edge():
    pre, _, _ = qc.expected("lanes260")
    m1 = R - 1
    assert len(pre.u) == 260
    assert pre.u[254:258] == [m1, 0, m1, 3] and pre.v[254:258] == [5, m1, 0, m1]
    others = [x for vec in (pre.u, pre.v, pre.e) for j, x in enumerate(vec) if not 254 <= j <= 257 and j >= 2]
    assert all(0 < x < 1 << qc.SMALL_BITS for x in others)


# ------------------------------------------------------------------ 2. what the oracle makes of them
@pytest.mark.parametrize("name", sorted(qc.SPECS) + sorted(qc.CEREMONY))
def test_oracle_lengths_are_what_the_targets_imply(name):
    pre, data, lengths = qc.expected(name)
    assert not pre.unconstrained and lengths == pre.lengths
    spec = qc.ALL[name]
    for key, vec in (("u", "a"), ("v", "b_g1")):
        kept = sum(1 for t, _ in spec[key] if t is None or qc.target(t) != 0)
        assert lengths[vec] == kept                      # -1 is kept, only 0 is filtered
    m = 8 if spec["nc"] + spec["ni"] <= 8 else 16
    points = 3 + lengths["ic"] + (m - 1) + lengths["l"] + lengths["a"] + lengths["b_g1"]
    assert len(data) == 96 * points + 192 * (3 + lengths["b_g2"]) + 4 * 6


def test_oracle_with_the_forks_toxic_waste():
    pre, data, lengths = qc.expected("rot01", "fork")
    assert lengths == pre.lengths and data != qc.expected("rot01")[1]


@pytest.mark.parametrize("name", sorted(qc.UNCONSTRAINED))
def test_oracle_refuses_aux_e_zero(name):
    pre, data, lengths = qc.expected(name)
    assert pre.unconstrained and data is None and lengths is None


def test_oracle_accepts_aux_e_minus_one():
    for name in qc.CONSTRAINED_M1:
        pre, data, lengths = qc.expected(name)
        assert (R - 1) in pre.e[pre.spec["ni"]:] and 0 not in pre.e[pre.spec["ni"]:] and data is not None
    assert qc.expected("aux_e_m1_twice")[0].e.count(R - 1) == 2


def test_input_e_zero_is_the_identity_point():
    pre, data, _ = qc.expected("input_e_zero")
    assert pre.e[:2] == [0, 0]
    ic = data[3 * 96 + 3 * 192 + 4:][:2 * 96]
    identity = bytes([0x40]) + bytes(95)
    assert ic == identity * 2


# ------------------------------------------------------------------ 3. the model of fe_is_zero
def _wraps():
    return {k: k * R - qc.FR_TOP for k in range(71, 128)}


def test_model_fr_accepts_the_multiples_and_the_57_wraps():
    n, top = qc.FR_LIMBS, qc.FR_TOP
    assert 70 * R < top < 71 * R and 127 * R < 2 * top and qc.fe_is_zero_kmax(R, n) == 70
    wraps = _wraps()
    assert len(wraps) == 57 and all(0 < x < top for x in wraps.values())
    # every one of them is the device Montgomery form of -1, and the two below 2r are all a kernel holds
    assert all(x % R == -top % R == (R - 1) * top % R for x in wraps.values())
    assert [k for k, x in wraps.items() if x < 2 * R] == [71, 72] and wraps[72] == wraps[71] + R
    accepted = {k * R % top for k in range(128)}
    assert accepted == {k * R for k in range(71)} | set(wraps.values()) and len(accepted) == 128
    assert all(qc.fe_is_zero_model(x, R, n) for x in accepted)
    # the bounded predicate: the multiples alone
    assert all(qc.fe_is_zero_model(k * R, R, n, 70) for k in range(71))
    assert not any(qc.fe_is_zero_model(x, R, n, 70) for x in wraps.values())
    # nothing else: the model compares x with (k r mod 2^261) for the k its low limb names, so a
    # value outside the 128 can only be accepted if that comparison is wrong.  Neighbours, single
    # flipped limbs under an unchanged low limb, and random values
    rng = random.Random(261)
    others = set()
    for x in accepted:
        others |= {x + 1, x - 1, x ^ (1 << qc.BITS), x ^ (1 << (qc.BITS * rng.randrange(1, n) + rng.randrange(qc.BITS)))}
        others.add((rng.randrange(top) >> qc.BITS << qc.BITS) | (x & ((1 << qc.BITS) - 1)))
    others |= {rng.randrange(top) for _ in range(4096)}
    others = {x for x in others if 0 <= x < top} - accepted
    for kmax in (127, 70):
        assert not any(qc.fe_is_zero_model(x, R, n, kmax) for x in others)


def test_model_fp_has_no_false_positive():
    n = qc.FP_LIMBS
    # 128 p fits the 14 limbs with 18 bits to spare, so no multiple the predicate tries wraps
    assert (128 * P).bit_length() == 388 <= qc.BITS * n == 406 and qc.fe_is_zero_kmax(P, n) == 127
    top = 1 << (qc.BITS * n)
    assert {k * P % top for k in range(128)} == {k * P for k in range(128)}
    rng = random.Random(406)
    for k in range(128):
        assert qc.fe_is_zero_model(k * P, P, n)
        for x in (k * P + top - (1 << 388), k * P + (1 << 388), (k * P + (rng.randrange(1, 1 << 17) << 388)),
                  k * P + 1, k * P + P - 1):
            if 0 <= x < top and x % P:
                assert not qc.fe_is_zero_model(x, P, n), (k, hex(x))
        # the wraps the predicate would need to be fooled: k p +- 2^406 lies outside 14 limbs
        assert not 0 <= k * P - top and k * P + top >= top
