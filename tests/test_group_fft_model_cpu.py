"""tests/group_fft_model.py (the stage schedule, twiddle index, gather map, w = 1 shortcut, 1/n pass
and column sum of csrc/group_fft.hip, over exponents) against oracle/bellman.py."""
import random

import pytest

from oracle import bellman as bm
from tests import group_fft_model as gm

E = bm.BLS12_381
R = gm.R


def _oracle(x, inverse):
    d = bm.EvaluationDomain(E, list(x))
    assert len(d.coeffs) == len(x)
    (d.ifft if inverse else d.fft)()
    return d.coeffs, d.omega


@pytest.mark.parametrize("n", [2, 4, 8, 64])
@pytest.mark.parametrize("inverse", [False, True])
def test_transform_matches_evaluation_domain(n, inverse):
    rng = random.Random(1000 + n)
    x = [rng.randrange(R) for _ in range(n)]
    want, omega = _oracle(x, inverse)
    stats = {}
    assert gm.fft_model(x, omega, inverse=inverse, stats=stats) == want
    assert stats["skipped"] == n // 2                     # the whole first stage
    assert stats["skipped"] + stats["muls_by_one"] == n - 1   # of the n - 1 butterflies with w = 1
    assert stats["muls"] + stats["skipped"] == (n // 2) * (n.bit_length() - 1)
    # small chunks: several launches per range, and the four output runs of each
    for chunk in (2, 4):                                  # (the device's is a power of two, 2 at the least)
        assert gm.fft_model(x, omega, inverse=inverse, chunk=chunk) == want
    # the measurement modes: every butterfly multiplies, or every stage's w = 1 prefix skips
    stats = {}
    assert gm.fft_model(x, omega, inverse=inverse, w1="none", chunk=4, stats=stats) == want
    assert stats["skipped"] == 0 and stats["muls_by_one"] == n - 1
    stats = {}
    assert gm.fft_model(x, omega, inverse=inverse, w1="prefix", chunk=4, stats=stats) == want
    assert stats["skipped"] == n - 1 and stats["muls_by_one"] == 0


@pytest.mark.parametrize("n", [2, 8, 64])
def test_unscaled_inverse_is_n_times_the_inverse(n):
    rng = random.Random(7 + n)
    x = [rng.randrange(R) for _ in range(n)]
    want, omega = _oracle(x, True)
    got = gm.fft_model(x, omega, inverse=True, scale=False)
    assert got == [v * n % R for v in want]


def test_gather_and_twiddles():
    for L in range(1, 8):
        n = 1 << L
        assert sorted(gm.gather_source(q, L) for q in range(n)) == list(range(n))
        for q in range(n):
            assert gm.rotr(gm.rotl(q, L), L) == q
        for s in range(L):
            ones = [b for b in range(n // 2) if gm.twiddle_index(s, b, L) == 0]
            assert ones == list(range(1 << (L - 1 - s)))  # the w = 1 butterflies are a prefix
        assert [gm.twiddle_index(L - 1, b, L) for b in range(n // 2)] == list(range(n // 2))


def test_column_sum_against_keypair_assembly():
    rng = random.Random(99)
    m = 64
    asm = bm.KeypairAssembly()
    one = asm.alloc_input("", lambda: 1)
    inp = asm.alloc_input("", lambda: 1)
    aux = [asm.alloc("", lambda: 1) for _ in range(5)]
    V = bm.LinearCombination
    big = aux[0]      # 1 100 terms in A: duplicates of (variable, row), more than R1CS_S segments
    canc = aux[1]     # c and r - c on one row
    for i in range(1100):
        row_vars = [(big, rng.randrange(1, R))]
        if i == 3:
            c = rng.randrange(1, R)
            row_vars += [(canc, c), (canc, R - c)]
        if i % 7 == 0:
            row_vars.append((aux[2 + i % 3], rng.randrange(R)))
        if i % 50 == 0:
            row_vars.append((inp, rng.randrange(R)))
        # 1 100 terms on the 50 rows the domain leaves after the inputs' appended rows
        asm.num_constraints = i % 50
        asm.enforce("", lambda lc, rv=row_vars: V(list(lc.terms) + rv), lambda lc: lc + one, lambda lc: lc + aux[4])
    asm.num_constraints = 50
    lag = [rng.randrange(R) for _ in range(m)]
    for cols in (asm.at_inputs + asm.at_aux, asm.bt_inputs + asm.bt_aux, asm.ct_inputs + asm.ct_aux):
        want = [sum(c * lag[i] for c, i in col) % R for col in cols]   # eval_at_tau, generator.rs:485-499
        assert gm.column_sums(cols, lag, m) == want
        assert gm.column_sums(cols, lag, m, chunk=40) == want          # chunks of one segment
    a_cols = asm.at_inputs + asm.at_aux
    assert len(a_cols[2]) == 1100
    _, _, seg, colseg, longcols = gm.segment_scheme(a_cols)
    assert longcols == [2] and colseg[3] - colseg[2] == 35
    assert gm.column_sums(a_cols, lag, m)[3] == 0 and len(a_cols[3]) == 2
