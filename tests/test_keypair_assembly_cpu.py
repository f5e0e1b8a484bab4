"""The Python KeypairAssembly (generator.rs:44-156) against the oracle's, and the flattening to
the ptr / row / coeff arrays bh_r1cs_create takes.  Host logic only."""
import numpy as np
import pytest

import bellman_hip as bh
from oracle import bellman as bm
from oracle import circuits as cc

R = bh.R_MODULUS
LISTS = ("at_inputs", "bt_inputs", "ct_inputs", "at_aux", "bt_aux", "ct_aux")

CIRCUITS = {
    "xor": lambda: cc.XorDemo(None, None),
    "and": lambda: cc.AndDemo(None, None),
    "add": lambda: cc.AddDemo(None, None),
    "chain_r7": lambda: cc.chain_circuit(R, 7, witness=False),
}


def _both(name):
    mine = bh.synthesize_keypair(CIRCUITS[name]())
    ref = bm.KeypairAssembly()
    ref.alloc_input("", lambda: 1)
    CIRCUITS[name]().synthesize(ref)
    return mine, ref


@pytest.mark.parametrize("name", sorted(CIRCUITS))
def test_term_lists_match_the_oracle(name):
    mine, ref = _both(name)
    assert (mine.num_inputs, mine.num_aux, mine.num_constraints) == (ref.num_inputs, ref.num_aux, ref.num_constraints)
    for k in LISTS:
        want = [[(c % R, row) for c, row in col] for col in getattr(ref, k)]
        assert getattr(mine, k) == want, k
    if name == "xor":  # the cases the device tests lean on: r - 1, a duplicate (variable, row) pair
        assert mine.at_aux[0] == [(R - 1, 0), (1, 2), (1, 2)]
        assert mine.bt_inputs == [[], []]


@pytest.mark.parametrize("name", sorted(CIRCUITS))
def test_flattening_round_trips(name):
    mine, _ = _both(name)
    n = mine.num_inputs + mine.num_aux
    for (ptr, row, coeff), ins, auxs in zip(mine.matrices(), (mine.at_inputs, mine.bt_inputs, mine.ct_inputs),
                                            (mine.at_aux, mine.bt_aux, mine.ct_aux)):
        assert ptr.dtype == np.uint64 and row.dtype == np.uint32 and coeff.dtype == np.uint64
        assert ptr.shape == (n + 1,) and ptr[0] == 0 and coeff.shape == (len(row), 4) and ptr[-1] == len(row)
        assert bh.unflatten_columns(ptr, row, coeff) == ins + auxs


def test_flattening_of_no_columns_and_empty_columns():
    ptr, row, coeff = bh.flatten_columns([[], [(5, 3)], []])
    assert ptr.tolist() == [0, 0, 1, 1] and row.tolist() == [3] and bh.fr_from_mont(coeff) == [5]
    ptr, row, coeff = bh.flatten_columns([])
    assert ptr.tolist() == [0] and row.shape == (0,) and coeff.shape == (0, 4)
