"""Per-proof verdicts on the device (bh_verify_each_device: csrc/verify.cpp, verify_each.hip and the
final exponentiation kernels of pairing_dev.hip) against bh_verify_proof, the host verifier, item by
item: for every j, (status[j], valid[j]) equals what the host returns and sets for that item, and
one bad item leaves the others alone.  Every comparison is an equality.

The host costs about 40 ms per item and is asked once per distinct (key, proof, inputs).  Batches
of 70 and 130 items cross a wave and a 64-thread block; replaced items stand at j = 0, 63, 64 and
k - 1.  The accumulation kernel's exceptional cases (an accumulator that is the identity, equal or
opposite to the point being added) cannot be reached through a golden key, whose ic_i have unknown
discrete logarithms, so they run on synthetic keys made of known multiples of the generators, for
which a valid proof can be forged for any inputs: the verdict 1 then depends on the accumulated
point being right, the identity included."""
import ctypes
import functools
import random

import numpy as np
import pytest

import proof_cases as pc
from oracle import bls12_381 as bls

pytestmark = pytest.mark.gpu

P, R = bls.P, bls.R
G1, G2 = bls.G1, bls.G2
EOF_STATUS = 2  # BH_ERR_UNEXPECTED_EOF


def _bh():
    import bellman_hip as bh
    return bh


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@functools.lru_cache(maxsize=None)
def host_item(vk, proof, inputs):
    """bh_verify_proof on raw words -> (status, valid); inputs: a tuple of ints below 2^256, unreduced"""
    vkb = np.frombuffer(vk, dtype=np.uint8)
    pf = np.frombuffer(proof, dtype=np.uint8)
    ins = np.array(pc.words(inputs) or [0] * 4, dtype=np.uint64)
    ok = ctypes.c_int(-1)
    st = _bh().lib().bh_verify_proof(_p(vkb), vkb.size, _p(pf), _p(ins), len(inputs), ctypes.byref(ok))
    return int(st), ok.value


def each(ctx, vk, proofs, inputs, num_inputs=None):
    """bh_verify_each_device on raw words -> (return value, [(status, valid)])"""
    k = len(proofs)
    vkb = np.frombuffer(bytes(vk), dtype=np.uint8)
    pf = np.frombuffer(b"".join(proofs) or b"\0", dtype=np.uint8)
    if num_inputs is None:
        num_inputs = len(inputs[0]) if k else 0
    ins = np.array(pc.words([x for row in inputs for x in row]) or [0] * 4, dtype=np.uint64)
    st = np.full(max(k, 1), 0xAAAAAAAA, dtype=np.uint32)
    ok = np.full(max(k, 1), 0xAA, dtype=np.uint8)
    ret = _bh().lib().bh_verify_each_device(ctx.h, _p(vkb), vkb.size, _p(pf), _p(ins), num_inputs, k, _p(st), _p(ok))
    return int(ret), [(int(s), int(v)) for s, v in zip(st[:k], ok[:k])]


def same_as_host(ctx, vk, proofs, inputs):
    """the device's answers, checked item by item against the host's"""
    ret, got = each(ctx, vk, proofs, inputs)
    assert ret == 0
    want = [host_item(bytes(vk), bytes(p), tuple(i)) for p, i in zip(proofs, inputs)]
    assert got == want, [(j, g, w) for j, (g, w) in enumerate(zip(got, want)) if g != w]
    return got


GOLDEN = [(params, items[0][0], items[0][1]) for params, items in pc.golden_batches().items()]
EDGES = lambda k: (0, 63, 64, k - 1)  # noqa: E731


def _swap_ac(p):
    return p[144:] + p[48:144] + p[:48]


def _flip_b(p):
    e = bytearray(p)
    e[48] ^= 0x20
    return bytes(e)


# ------------------------------------------------------------------ 1. golden proofs, tiled
@pytest.mark.parametrize("k", [70, 130])
@pytest.mark.parametrize("which", range(len(GOLDEN)))
def test_golden_proofs_tiled_are_all_valid(ctx, which, k):
    vk, proof, public = GOLDEN[which]
    assert same_as_host(ctx, vk, [proof] * k, [public] * k) == [(0, 1)] * k


@pytest.mark.parametrize("k", [70, 130])
@pytest.mark.parametrize("which", range(len(GOLDEN)))
def test_replaced_items_at_the_edges(ctx, which, k):
    vk, proof, public = GOLDEN[which]
    foreign_c = GOLDEN[(which + 1) % len(GOLDEN)][1][144:]
    proofs, inputs = [proof] * k, [list(public) for _ in range(k)]
    j0, j1, j2, j3 = EDGES(k)
    proofs[j0] = _swap_ac(proof)
    proofs[j1] = _flip_b(proof)
    inputs[j2] = [(public[0] + 1) % R] + public[1:]
    proofs[j3] = proof[:144] + foreign_c
    got = same_as_host(ctx, vk, proofs, inputs)
    assert got == [(0, 0) if j in EDGES(k) else (0, 1) for j in range(k)]


# ------------------------------------------------------------------ 2. malformed encodings
def _crafted_ids():
    return [name for name, _, _ in pc.proof_cases(GOLDEN[0][1])]


@pytest.mark.parametrize("idx", range(len(_crafted_ids())), ids=_crafted_ids())
def test_each_crafted_encoding_affects_its_item_only(ctx, idx):
    vk, proof, public = GOLDEN[0]
    name, crafted, status = pc.proof_cases(proof)[idx]
    for j in (33, 69):  # different waves
        proofs = [proof] * 70
        proofs[j] = crafted
        got = same_as_host(ctx, vk, proofs, [public] * 70)
        assert got[j] == (status, 0), (name, j)
        assert [g for i, g in enumerate(got) if i != j] == [(0, 1)] * 69, (name, j)


def _case(proof, name):
    return next(p for n, p, _ in pc.proof_cases(proof) if n == name)


def test_an_input_not_below_r_fails_its_item_only(ctx):
    vk, proof, public = GOLDEN[1]
    k = 70
    inputs = [list(public) for _ in range(k)]
    inputs[5], inputs[64], inputs[69] = [R], [R + public[0]], [(1 << 256) - 1]
    proofs = [proof] * k
    proofs[64] = _case(proof, "B:off_subgroup_sign0")   # with a bad input: the proof's status comes first
    proofs[40] = _case(proof, "C:x_equals_p")
    got = same_as_host(ctx, vk, proofs, inputs)
    want = {5: (pc.INVALID_ARGUMENT, 0), 64: (pc.NOT_IN_SUBGROUP, 0), 69: (pc.INVALID_ARGUMENT, 0),
            40: (pc.INVALID_ENCODING, 0)}
    assert got == [want.get(j, (0, 1)) for j in range(k)]


# ------------------------------------------------------------------ 3. the accumulation's exceptional cases
class SyntheticKey:
    """A verifying key of known multiples of the generators: alpha = a G1, beta = b G2, gamma = g G2,
    delta = d G2, ic_i = s_i G1 -- encoded with the oracle's encoders in VerifyingKey::write's
    layout.  forge(inputs) is a proof that verifies for those inputs: A = u G1, B = v G2 and
    C = c G1 with u v = a b + acc g + c d (mod r), acc = s_0 + sum_i x_i s_(i+1)."""

    def __init__(self, ic_scalars, seed):
        rng = random.Random(seed)
        self.a, self.b, self.g, self.d = (rng.randrange(1, R) for _ in range(4))
        self.s = [x % R for x in ic_scalars]
        self.rng = rng
        g1 = lambda x: bls.g1_to_uncompressed(G1.to_affine(G1.mul(G1.generator(), x)))  # noqa: E731
        g2 = lambda x: bls.g2_to_uncompressed(G2.to_affine(G2.mul(G2.generator(), x)))  # noqa: E731
        self.bytes = (g1(self.a) + g1(rng.randrange(1, R)) + g2(self.b) + g2(self.g) + g1(self.d) + g2(self.d) +
                      len(self.s).to_bytes(4, "big") + b"".join(g1(x) for x in self.s))

    def acc(self, inputs):
        return (self.s[0] + sum(x * s for x, s in zip(inputs, self.s[1:]))) % R

    def forge(self, inputs):
        while True:
            u, v = self.rng.randrange(1, R), self.rng.randrange(1, R)
            c = (u * v - self.a * self.b - self.acc(inputs) * self.g) * pow(self.d, -1, R) % R
            if c:
                break
        return (bls.g1_to_compressed(G1.to_affine(G1.mul(G1.generator(), u))) +
                bls.g2_to_compressed(G2.to_affine(G2.mul(G2.generator(), v))) +
                bls.g1_to_compressed(G1.to_affine(G1.mul(G1.generator(), c))))


S0, S1 = 0x1234567 ** 5 % R, 0x7654321 ** 7 % R
INV16 = pow(16, -1, R)
# name: (ic scalars, [inputs], acc is the identity)
EXCEPTIONAL = {
    # acc = ic_0 - ic_0: the last addition meets its opposite, the result is the identity
    "ic1_is_minus_ic0_input_1": ([S0, -S0], [[1]]),
    # acc = ic_0 + ic_0: the last addition doubles
    "ic1_is_ic0_input_1": ([S0, S0], [[1]]),
    # two bases, one point: the second addition of the last window doubles the first's result
    "ic2_is_ic1_inputs_1_1": ([S0, S1, S1], [[1, 1]]),
    # the second addition cancels the first: the accumulator returns to the identity mid-way
    "ic2_is_minus_ic1_inputs_1_1": ([S0, S1, -S1], [[1, 1]]),
    # window 1 leaves ic_1, four doublings make 16 ic_1, and window 0 adds 1 (16 ic_1): a doubling
    # away from the last window; then 2 (16 ic_1) - ... with digit -8: the table's top multiple
    "ic2_is_16_ic1": ([S0, S1, 16 * S1], [[16, 1], [16, 8], [1, R - INV16]]),
    "zero_inputs": ([S0, S1, 3 * S1], [[0, 0]]),
    "r_minus_1": ([S0, S1], [[R - 1], [R - 2], [(1 << 254) + 5], [0x8888888888888888], [8], [7], [9]]),
    "sum_is_the_identity": ([S0, S1, 5], [[2, (-(S0 + 2 * S1)) * pow(5, -1, R) % R]]),
}


@functools.lru_cache(maxsize=None)
def _synthetic(name):
    ic, rows = EXCEPTIONAL[name]
    key = SyntheticKey(ic, seed=len(name))
    return key, [(key.forge(row), row) for row in rows]


@pytest.mark.parametrize("name", list(EXCEPTIONAL))
def test_exceptional_accumulations_on_a_synthetic_key(ctx, name):
    key, items = _synthetic(name)
    if name in ("ic1_is_minus_ic0_input_1", "sum_is_the_identity"):
        assert all(key.acc(row) == 0 for _, row in items)
    proofs, inputs = [p for p, _ in items], [row for _, row in items]
    # every forged proof verifies for its inputs and for no others
    proofs, inputs = proofs + proofs, inputs + [[(row[0] + 1) % R] + row[1:] for row in inputs]
    got = same_as_host(ctx, key.bytes, proofs, inputs)
    assert got == [(0, 1)] * len(items) + [(0, 0)] * len(items)


def test_exceptional_items_among_ordinary_ones(ctx):
    """the identity lane beside full lanes, past a wave: k = 70"""
    key, items = _synthetic("ic1_is_minus_ic0_input_1")
    proof, row = items[0]
    other = key.forge([12345])
    proofs, inputs = [other] * 70, [[12345]] * 70
    for j in (0, 31, 32, 63, 64, 69):  # 31 / 32: the normalisation's group edge
        proofs[j], inputs[j] = proof, row
    proofs[33], inputs[33] = proof, [2]
    got = same_as_host(ctx, key.bytes, proofs, inputs)
    assert got == [(0, 0) if j == 33 else (0, 1) for j in range(70)]


# ------------------------------------------------------------------ 4. what is common to all items
def test_no_items_and_one_item(ctx):
    vk, proof, public = GOLDEN[2]
    assert each(ctx, vk, [], [], num_inputs=len(public)) == (0, [])
    assert same_as_host(ctx, vk, [proof], [public]) == [(0, 1)]
    assert same_as_host(ctx, vk, [_swap_ac(proof)], [public]) == [(0, 0)]


def test_the_return_value_reports_the_key_and_the_input_count(ctx):
    vk, proof, public = GOLDEN[3]
    for k in (0, 3):
        ret, got = each(ctx, vk[:100], [proof] * k, [public] * k, num_inputs=len(public))
        assert ret == host_item(vk[:100], proof, tuple(public))[0] == EOF_STATUS
        assert got == [(0xAAAAAAAA, 0xAA)] * k                     # nothing written
        ret, got = each(ctx, vk, [proof] * k, [public + [1]] * k, num_inputs=len(public) + 1)
        assert ret == host_item(vk, proof, tuple(public + [1]))[0] == pc.INVALID_ARGUMENT
    f = _bh().lib().bh_verify_each_device
    buf = np.zeros(4096, dtype=np.uint8)
    assert f(None, _p(buf), 10, _p(buf), _p(buf), 1, 1, _p(buf), _p(buf)) == pc.INVALID_ARGUMENT
    assert f(ctx.h, _p(buf), 10, None, _p(buf), 1, 1, _p(buf), _p(buf)) == pc.INVALID_ARGUMENT
    assert f(ctx.h, _p(buf), 10, _p(buf), _p(buf), 1, 1, None, _p(buf)) == pc.INVALID_ARGUMENT


def test_device_made_proofs_and_rotated_inputs(ctx):
    """four prove_batch proofs with distinct witnesses (tests/test_gpu_parity.py's c5 batch)"""
    bh = _bh()
    rounds = (1 << 11) - 1
    params = bh.Parameters.chain(ctx, rounds)
    ws = [bh.Witness.chain(ctx, rounds, seed=7, preimage_seed=20 + i) for i in range(4)]
    proofs = bh.prove_batch(ctx, params, ws, 27134, 17146)
    vk = params.vk_bytes()
    publics = [bh.fr_from_mont(bh.chain_assignment(rounds, seed=7, preimage_seed=20 + i)["inputs"])[1:]
               for i in range(4)]
    assert same_as_host(ctx, vk, proofs, publics) == [(0, 1)] * 4
    assert same_as_host(ctx, vk, proofs, publics[1:] + publics[:1]) == [(0, 0)] * 4
    assert bh.verify_each(ctx, vk, proofs, publics[:2] + publics[1:2] + publics[3:]) == ([0] * 4, [True, True, False, True])


def test_python_verifier_verify_each(ctx):
    bh = _bh()
    vk, proof, public = GOLDEN[1]
    v = bh.Verifier()
    for p in (proof, _swap_ac(proof), _case(proof, "A:non_residue"), proof):
        v.queue((p, public))
    with pytest.raises(bh.SynthesisError):  # the batch stops at its first malformed proof
        v.verify(random.Random(3), vk, ctx=ctx)
    assert v.verify_each(vk, ctx) == ([0, 0, pc.INVALID_ENCODING, 0], [True, False, False, True])
    assert bh.Verifier().verify_each(vk, ctx) == ([], [])
    with pytest.raises(bh.SynthesisError) as e:
        bh.verify_each(ctx, vk[:100], [proof], [public])
    assert e.value.code == EOF_STATUS
