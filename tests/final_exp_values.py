"""Fp12 values for the final exponentiation's tests and the host yardstick on them: the operands
that the chain's helpers (conjugation, Frobenius maps, the inversion through norms, the products'
lazy bounds) can get wrong, Miller values of golden proofs, seeded random values.  Shared by
tests/test_final_exp_chain_cpu.py (the chain on the host) and tests/test_gpu_final_exp.py (the
kernels).  Not a test module."""
import ctypes
import functools
import random

import numpy as np

import proof_cases as pc
from oracle import bls12_381 as bls
from oracle import pairing as pr

P, R = bls.P, bls.R
X = -0xd201000000010000
C = 0x396c8c005555e1568c00aaab0000aaab
ZERO = [(0, 0)] * 6
ONE = [(1, 0)] + [(0, 0)] * 5


def _bh():
    import bellman_hip as bh
    return bh


def to_bytes(f):
    return b"".join(int(x).to_bytes(48, "big") for c in f for x in c)


def from_bytes(b):
    c = [int.from_bytes(b[48 * k:48 * k + 48], "big") for k in range(12)]
    return [(c[2 * i], c[2 * i + 1]) for i in range(6)]


def call(name, f):
    """a host entry point of the form (f[576], out[576]) -> (status, value)"""
    fn = getattr(_bh().lib(), name)
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    src = np.frombuffer(to_bytes(f), dtype=np.uint8)
    out = np.full(576, 0xAA, dtype=np.uint8)
    st = fn(src.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p))
    return st, from_bytes(out.tobytes())


@functools.lru_cache(maxsize=None)
def ladder(key):
    """bh_final_exponentiation, the yardstick, kept per distinct value (key: the value's bytes)"""
    st, v = call("bh_final_exponentiation", from_bytes(key))
    assert st == 0
    return v


def chain(f):
    st, v = call("bh_selftest_final_exponentiation_chain", f)
    assert st == 0
    return v


@functools.lru_cache(maxsize=None)
def golden_miller_values():
    """f(A, B) of the first golden proof of two verifying keys"""
    out = []
    batches = list(pc.golden_batches().items())
    for _, items in batches[:2]:
        a, b, _ = pr.proof_from_bytes(items[0][0])
        out.append(pr.multi_miller_loop([(a, b)]))
    return out


SPECIAL = ["one", "zero", "only_c0", "only_c0_real", "only_odd", "only_even", "all_p_minus_1", "only_c3", "c1_halves",
           "near_limb_maxima", "golden_miller_0", "golden_miller_1"]


@functools.lru_cache(maxsize=None)
def special_values():
    """[(name, value)] in SPECIAL's order: the operands the chain's helpers can get wrong"""
    rng = random.Random(20251021)
    fp = lambda: rng.randrange(P)  # noqa: E731
    vals = [("one", ONE), ("zero", ZERO),
            ("only_c0", [(fp(), fp())] + [(0, 0)] * 5),            # in Fp2: the easy part sends it to one
            ("only_c0_real", [(fp(), 0)] + [(0, 0)] * 5),
            ("only_odd", [(fp(), fp()) if k & 1 else (0, 0) for k in range(6)]),
            ("only_even", [(0, 0) if k & 1 else (fp(), fp()) for k in range(6)]),  # in Fp6
            ("all_p_minus_1", [(P - 1, P - 1)] * 6),
            ("only_c3", [(0, 0)] * 3 + [(1, 0)] + [(0, 0)] * 2),   # w^3
            ("c1_halves", [(0, 0), (P - 1, 0), (0, 0), (0, P - 1), (0, 0), (0, 0)]),
            ("near_limb_maxima", [(P - 1 - (1 << 28), P - 2)] * 6)]
    vals += [(f"golden_miller_{i}", v) for i, v in enumerate(golden_miller_values())]
    assert [n for n, _ in vals] == SPECIAL
    return vals


def random_values(n, seed=7):
    rng = random.Random(seed)
    return [[(rng.randrange(P), rng.randrange(P)) for _ in range(6)] for _ in range(n)]
