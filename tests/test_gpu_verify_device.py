"""The device batch verifier (csrc/proofs_dev.hip, bh_proofs_decode, bh_verify_batch_device):

1. the decode kernels' square-root routine (bh_selftest_field_sqrt) against Python integers;
2. bh_proofs_decode: coordinates against oracle/pairing.py's decompression, statuses against the
   host verifier's on the same batch (the crafted encodings of tests/proof_cases.py);
3. bh_verify_batch_device: status and verdict equal to bh_verify_batch on the same arguments.

Every comparison is an equality: field arithmetic is exact and both verifiers are deterministic in
the caller's z."""
import ctypes
import random

import numpy as np
import pytest

import proof_cases as pc
from oracle import bls12_381 as bls
from oracle import pairing as pr

pytestmark = pytest.mark.gpu

P, R = bls.P, bls.R
F2 = bls.Fp2Ops
G1, G2 = bls.G1, bls.G2


def _bh():
    import bellman_hip as bh
    return bh


def _host(*a, **kw):
    return pc.call_batch(_bh().lib().bh_verify_batch, *a, **kw)


def _device(ctx, *a, **kw):
    return pc.call_batch(_bh().lib().bh_verify_batch_device, *a, ctx=ctx, **kw)


def _same(ctx, *a, **kw):
    """both verifiers on the same arguments: equal (status, valid); returned"""
    want = _host(*a, **kw)
    got = _device(ctx, *a, **kw)
    assert got == want, (got, want)
    return got


# ------------------------------------------------------------------ 1. square roots
def _sqrt(field, values):
    """bh_selftest_field_sqrt -> [(is_square, root)]; values: ints (field 1) or (c0, c1) (field 2)"""
    f = _bh().lib().bh_selftest_field_sqrt
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    flat = [c for v in values for c in ((v,) if field == 1 else v)]
    src = np.frombuffer(b"".join(int(c).to_bytes(48, "little") for c in flat), dtype=np.uint32).copy()
    pw = 12 * field
    out = np.full(len(values) * (pw + 1), 0xAAAAAAAA, dtype=np.uint32)
    st = f(0, field, src.ctypes.data_as(ctypes.c_void_p), len(values), out.ctypes.data_as(ctypes.c_void_p))
    assert st == 0, st
    res = []
    for i in range(len(values)):
        rec = out[i * (pw + 1):(i + 1) * (pw + 1)]
        comps = [int.from_bytes(rec[1 + 12 * c:13 + 12 * c].tobytes(), "little") for c in range(field)]
        assert rec[0] in (0, 1) and all(c < P for c in comps)
        res.append((bool(rec[0]), comps[0] if field == 1 else tuple(comps)))
    return res


def _fp_non_residue(rng):
    while True:
        a = rng.randrange(1, P)
        if pow(a, (P - 1) // 2, P) == P - 1:
            return a


def _fp2_is_square(a):
    n = (a[0] * a[0] + a[1] * a[1]) % P  # a is a square in Fp2 iff its norm is one in Fp
    return n == 0 or pow(n, (P - 1) // 2, P) == 1


def test_fp_square_roots_are_exact(ctx):
    rng = random.Random(31)
    ts = [rng.randrange(P) for _ in range(64)]
    values = [0, 1, 4, P - 1] + [t * t % P for t in ts] + [_fp_non_residue(rng) for _ in range(64)]
    values += [P - 1 - d for d in (1, 2, 3, 1 << 28, (1 << 29) - 1)]  # every limb near its maximum
    for (sq, r), a in zip(_sqrt(1, values), values):
        assert sq == (a == 0 or pow(a, (P - 1) // 2, P) == 1), a  # Euler's criterion
        if sq:
            assert r * r % P == a, a
    assert not _sqrt(1, [P - 1])[0][0]  # p = 3 mod 4: -1 is not a square


def test_fp2_square_roots_are_exact(ctx):
    rng = random.Random(32)
    values = [(0, 0), (1, 0), (P - 1, 0), (0, 1)]
    for _ in range(16):
        t, s = rng.randrange(1, P), rng.randrange(1, P)
        values += [F2.sqr((t, 0)), F2.sqr((0, t)), F2.sqr((t, s))]  # (0, t)^2 = -t^2: alpha = -1
    squares = len(values)
    while len(values) < squares + 24:  # non-squares
        a = (rng.randrange(P), rng.randrange(P))
        if not _fp2_is_square(a):
            values.append(a)
    values += [(P - 1, P - 1), (P - 2, P - 1 - (1 << 28))]
    got = _sqrt(2, values)
    for i, ((sq, r), a) in enumerate(zip(got, values)):
        assert sq == _fp2_is_square(a), a
        if sq:
            assert F2.sqr(r) == (a[0] % P, a[1] % P), a
    assert all(sq for sq, _ in got[:squares])
    assert got[2][0] and F2.sqr(got[2][1]) == (P - 1, 0)  # sqrt(-1) = +-u


def test_field_sqrt_rejects_noncanonical_input(ctx):
    f = _bh().lib().bh_selftest_field_sqrt
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    src = np.frombuffer(P.to_bytes(48, "little"), dtype=np.uint32).copy()
    out = np.zeros(13, dtype=np.uint32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    assert f(0, 1, p(src), 1, p(out)) == pc.INVALID_ARGUMENT
    assert f(0, 3, p(src), 1, p(out)) == pc.INVALID_ARGUMENT


# ------------------------------------------------------------------ 2. decode
K_DECODE = 70  # crosses a wave boundary


class _Points:
    """70 'proofs' of oracle multiples of the generators (a_i G1, b_i G2, c_i G1), by repeated
    addition, compressed with the oracle's encoders; well-formed, not valid proofs."""

    def __init__(self):
        rng = random.Random(20250611)

        def walk(G, n):
            p = G.mul(G.generator(), rng.getrandbits(64) | 1)
            step = G.mul(G.generator(), rng.getrandbits(64) | 1)
            out = []
            for _ in range(n):
                out.append(G.to_affine(p))
                p = G.add(p, step)
            return out

        self.a, self.b, self.c = walk(G1, K_DECODE), walk(G2, K_DECODE), walk(G1, K_DECODE)
        self.proofs = [bls.g1_to_compressed(a) + bls.g2_to_compressed(b) + bls.g1_to_compressed(c)
                       for a, b, c in zip(self.a, self.b, self.c)]
        # a verifying key with one public input, so that the host verifier can walk these batches
        self.params = next(p for p, items in pc.golden_batches().items() if len(items[0][1]) == 1)
        self.inputs = [[1]] * K_DECODE
        self.zs = [rng.randrange(1, R) for _ in range(K_DECODE)]


@pytest.fixture(scope="module")
def points():
    return _Points()


def _decode(ctx, proofs):
    """bh_proofs_decode -> (return value, statuses, (ha, hb, hc) raw handles)"""
    bh = _bh()
    k = len(proofs)
    pf = np.frombuffer(b"".join(proofs) or b"\0", dtype=np.uint8)
    st = np.full(max(k, 1), 0xAAAAAAAA, dtype=np.uint32)
    hs = [ctypes.c_void_p(0xDEAD) for _ in range(3)]
    code = bh.lib().bh_proofs_decode(ctx.h, pf.ctypes.data_as(ctypes.c_void_p), k, st.ctypes.data_as(ctypes.c_void_p),
                                     *[ctypes.byref(h) for h in hs])
    return code, [int(x) for x in st[:k]], hs


def _free(hs):
    for h in hs:
        if h.value:
            assert _bh().lib().bh_srs_free(h) == 0


def test_decode_matches_the_oracle_decompression(ctx, points):
    bh = _bh()
    for slot, pts in (("A", points.a), ("B", points.b), ("C", points.c)):
        lo = pc.SLOTS[slot][0]
        assert {bool(p[lo] & 0x20) for p in points.proofs} == {False, True}, slot  # both sign flags
    A, B, C, st = bh.proofs_decode(ctx, points.proofs)
    assert st == [0] * K_DECODE and len(A) == len(B) == len(C) == K_DECODE
    for j, p in enumerate(points.proofs):
        a, b, c = pr.proof_from_bytes(p)
        assert (a, b, c) == (points.a[j], points.b[j], points.c[j])
        assert A.get(j) == bls.g1_to_uncompressed(a), j
        assert B.get(j) == bls.g2_to_uncompressed(b), j
        assert C.get(j) == bls.g1_to_uncompressed(c), j


def test_decode_of_no_proofs_gives_three_empty_vectors(ctx):
    A, B, C, st = _bh().proofs_decode(ctx, [])
    assert st == [] and len(A) == len(B) == len(C) == 0
    assert (A.group, B.group, C.group) == (_bh().BH_G1, _bh().BH_G2, _bh().BH_G1)


def _crafted_ids():
    proof = next(iter(pc.golden_batches().values()))[0][0]
    return [name for name, _, _ in pc.proof_cases(proof)]


@pytest.mark.parametrize("idx", range(len(_crafted_ids())), ids=_crafted_ids())
def test_decode_status_of_each_crafted_case(ctx, points, idx):
    """the case at j = 0, in the middle and at j = k - 1 of an otherwise valid batch"""
    for j in (0, K_DECODE // 2 - 2, K_DECODE - 1):  # 33 and 69 sit in different waves
        name, crafted, status = pc.proof_cases(points.proofs[j])[idx]
        batch = points.proofs[:j] + [crafted] + points.proofs[j + 1:]
        code, st, hs = _decode(ctx, batch)
        if status == pc.OK:  # well-formed: decodes to the negated point
            assert code == 0 and st == [0] * K_DECODE and all(h.value for h in hs), (name, j)
            _free(hs)
            continue
        host_status, _ = _host(points.params, batch, points.inputs, points.zs)
        assert host_status == status, (name, j, host_status)
        assert code == host_status and st[j] == host_status, (name, j, code, st[j])
        assert [s for i, s in enumerate(st) if i != j] == [0] * (K_DECODE - 1), (name, j)
        assert [h.value for h in hs] == [None] * 3, (name, j)


def test_flipped_sign_flag_decodes_to_the_negated_point(ctx, points):
    bh = _bh()
    batch = list(points.proofs)
    for slot, j in (("A", 3), ("B", 64), ("C", 69)):
        lo = pc.SLOTS[slot][0]
        e = bytearray(batch[j])
        e[lo] ^= 0x20
        batch[j] = bytes(e)
    A, B, C, st = bh.proofs_decode(ctx, batch)
    assert st == [0] * K_DECODE
    ax, ay = points.a[3]
    assert A.get(3) == bls.g1_to_uncompressed((ax, (P - ay) % P))
    bx, by = points.b[64]
    assert B.get(64) == bls.g2_to_uncompressed((bx, F2.neg(by)))
    cx, cy = points.c[69]
    assert C.get(69) == bls.g1_to_uncompressed((cx, (P - cy) % P))
    assert A.get(4) == bls.g1_to_uncompressed(points.a[4])


def _case(proof, name):
    return next(p for n, p, _ in pc.proof_cases(proof) if n == name)


def test_two_failures_in_one_batch_the_lower_index_wins(ctx, points):
    batch = list(points.proofs)
    batch[65] = _case(batch[65], "A:x_equals_p")              # INVALID_ENCODING
    batch[12] = _case(batch[12], "C:off_subgroup_sign1")      # NOT_IN_SUBGROUP, lower index
    code, st, hs = _decode(ctx, batch)
    assert code == pc.NOT_IN_SUBGROUP and st[12] == pc.NOT_IN_SUBGROUP and st[65] == pc.INVALID_ENCODING
    assert sum(1 for s in st if s) == 2 and [h.value for h in hs] == [None] * 3
    assert _host(points.params, batch, points.inputs, points.zs)[0] == code


def test_two_failures_in_one_proof_a_before_b_before_c(ctx, points):
    j = 40
    p = points.proofs[j]
    a_sub = _case(p, "A:off_subgroup_sign0")[0:48]
    b_enc = _case(p, "B:non_residue")[48:144]
    b_sub = _case(p, "B:off_subgroup_sign1")[48:144]
    c_enc = _case(p, "C:compression_flag_cleared")[144:192]
    for proof, want in ((a_sub + b_enc + p[144:], pc.NOT_IN_SUBGROUP),   # A wins over B
                        (p[:48] + b_sub + c_enc, pc.NOT_IN_SUBGROUP)):   # B wins over C
        batch = points.proofs[:j] + [proof] + points.proofs[j + 1:]
        code, st, hs = _decode(ctx, batch)
        assert code == want and st[j] == want and sum(1 for s in st if s) == 1
        assert _host(points.params, batch, points.inputs, points.zs)[0] == want


# ------------------------------------------------------------------ 3. verdicts
def _golden3():
    """[(params, proofs, inputs)]: each verifying key's golden proofs three times over"""
    return [(params, [p for p, _ in items] * 3, [i for _, i in items] * 3)
            for params, items in pc.golden_batches().items()]


def _swap_ac(p):
    return p[144:] + p[48:144] + p[:48]


@pytest.mark.parametrize("which", range(len(_golden3())))
def test_golden_batches_valid_and_tampered(ctx, which):
    params, proofs, inputs = _golden3()[which]
    rng = random.Random(11 + which)
    zs = [rng.randrange(1, R) for _ in proofs]
    assert _same(ctx, params, proofs, inputs, zs) == (0, 1)
    assert _same(ctx, params, [_swap_ac(proofs[0])] + proofs[1:], inputs, zs) == (0, 0)
    bad_inputs = inputs[:1] + [[(inputs[1][0] + 1) % R] + inputs[1][1:]] + inputs[2:]
    assert _same(ctx, params, proofs, bad_inputs, zs) == (0, 0)
    flipped = bytearray(proofs[-1])
    flipped[48] ^= 0x20  # B's sign flag: -B
    assert _same(ctx, params, proofs[:-1] + [bytes(flipped)], inputs, zs) == (0, 0)
    same_z = [zs[0]] * len(proofs)
    assert _same(ctx, params, proofs, inputs, same_z) == (0, 1)
    assert _same(ctx, params, proofs[:1] + [_swap_ac(proofs[1])] + proofs[2:], inputs, same_z) == (0, 0)


def test_invalid_arguments_raise_with_the_host_status(ctx):
    params, proofs, inputs = _golden3()[0]
    zs = [5, 6, 7]
    E = (pc.INVALID_ARGUMENT, 0)
    assert _same(ctx, params, proofs, inputs, [5, 0, 7]) == E          # z = 0
    assert _same(ctx, params, proofs, inputs, [5, 6, R]) == E          # z = r
    assert _same(ctx, params, proofs, [inputs[0], [R], inputs[2]], zs) == E  # an input = r
    two = [i + [1] for i in inputs]
    assert _same(ctx, params, proofs, two, zs) == E                    # a wrong input count
    assert _same(ctx, params[:100], proofs, inputs, zs)[0] != 0        # a truncated verifying key
    bh = _bh()
    with pytest.raises(bh.SynthesisError) as dev:
        bh.verify_batch_device(ctx, params, proofs, inputs, [5, 0, 7])
    with pytest.raises(bh.SynthesisError) as host:
        bh.verify_batch(params, proofs, inputs, [5, 0, 7])
    assert dev.value.code == host.value.code == pc.INVALID_ARGUMENT


def test_error_precedence_follows_the_host_walk(ctx):
    params, proofs, inputs = _golden3()[0]
    proofs, inputs = proofs * 2, inputs * 2  # k = 6
    bad3 = proofs[:3] + [_case(proofs[3], "B:off_subgroup_sign0")] + proofs[4:]
    zs = [3, 4, 5, 6, 7, 0]  # z_5 = 0 comes after proof 3
    assert _same(ctx, params, bad3, inputs, zs) == (pc.NOT_IN_SUBGROUP, 0)
    zs = [3, 0, 5, 6, 7, 8]  # z_1 = 0 comes before proof 3
    assert _same(ctx, params, bad3, inputs, zs) == (pc.INVALID_ARGUMENT, 0)
    # inputs of proof 2 (>= r) come before proof 3, inputs of proof 3 after it
    zs = [3, 4, 5, 6, 7, 8]
    assert _same(ctx, params, bad3, inputs[:2] + [[R + 1]] + inputs[3:], zs) == (pc.INVALID_ARGUMENT, 0)
    assert _same(ctx, params, bad3, inputs[:3] + [[R + 1]] + inputs[4:], zs) == (pc.NOT_IN_SUBGROUP, 0)
    enc3 = proofs[:3] + [_case(proofs[3], "C:x_all_ones")] + proofs[4:]
    assert _same(ctx, params, enc3, inputs, zs) == (pc.INVALID_ENCODING, 0)


def test_empty_and_single_batches(ctx):
    params, proofs, inputs = _golden3()[0]
    assert _same(ctx, params, [], [], [], num_inputs=len(inputs[0])) == (0, 1)
    assert _same(ctx, params, proofs[:1], inputs[:1], [R - 2]) == (0, 1)
    assert _same(ctx, params, [_swap_ac(proofs[0])], inputs[:1], [R - 2]) == (0, 0)


def test_narrow_and_full_width_z(ctx):
    params, proofs, inputs = _golden3()[1]
    rng = random.Random(77)
    narrow = [rng.getrandbits(128) | 1 for _ in proofs]
    assert _same(ctx, params, proofs, inputs, narrow) == (0, 1)
    assert _same(ctx, params, proofs, inputs, [1, 1, 1]) == (0, 1)
    full = [R - 1, rng.randrange(1 << 254, R), 1]
    assert _same(ctx, params, proofs, inputs, full) == (0, 1)
    assert _same(ctx, params, proofs[:2] + [_swap_ac(proofs[2])], inputs, full) == (0, 0)


def test_device_made_proofs(ctx):
    """four prove_batch proofs with distinct witnesses (tests/test_gpu_parity.py's c5 batch)"""
    bh = _bh()
    rounds = (1 << 11) - 1
    params = bh.Parameters.chain(ctx, rounds)
    ws = [bh.Witness.chain(ctx, rounds, seed=7, preimage_seed=20 + i) for i in range(4)]
    proofs = bh.prove_batch(ctx, params, ws, 27134, 17146)
    vk = params.vk_bytes()
    publics = [bh.fr_from_mont(bh.chain_assignment(rounds, seed=7, preimage_seed=20 + i)["inputs"])[1:]
               for i in range(4)]
    rng = random.Random(5)
    zs = [rng.randrange(1, R) for _ in proofs]
    assert _same(ctx, vk, proofs, publics, zs) == (0, 1)
    assert _same(ctx, vk, proofs, publics[1:] + publics[:1], zs) == (0, 0)


@pytest.fixture(scope="module")
def tiled():
    """k = 257 by tiling two verifying-key-mates: crosses a 256-thread block"""
    params, proofs, inputs = _golden3()[2]
    k = 257
    rng = random.Random(257)
    return params, (proofs * k)[:k], (inputs * k)[:k], [rng.getrandbits(128) | 1 for _ in range(k)]


def test_k257_valid(ctx, tiled):
    params, proofs, inputs, zs = tiled
    assert _same(ctx, params, proofs, inputs, zs) == (0, 1)


def test_k257_last_c_replaced(ctx, tiled, points):
    params, proofs, inputs, zs = tiled
    last = proofs[-1][:144] + points.proofs[0][144:]  # another (well-formed) C
    assert _same(ctx, params, proofs[:-1] + [last], inputs, zs) == (0, 0)


def test_k257_last_a_malformed(ctx, tiled):
    params, proofs, inputs, zs = tiled
    last = _case(proofs[-1], "A:non_residue")
    assert _same(ctx, params, proofs[:-1] + [last], inputs, zs) == (pc.INVALID_ENCODING, 0)


def test_python_verifier_with_and_without_a_context(ctx):
    bh = _bh()
    params, proofs, inputs = _golden3()[3]
    good, bad = bh.Verifier(), bh.Verifier()
    for p, i in zip(proofs, inputs):
        good.queue((p, i))
    for p, i in zip([_swap_ac(proofs[0])] + proofs[1:], inputs):
        bad.queue((p, i))
    zs = [random.Random(9).randrange(1, R) for _ in proofs]
    assert good.verify(zs, params) is True and good.verify(zs, params, ctx=ctx) is True
    assert bad.verify(zs, params) is False and bad.verify(zs, params, ctx=ctx) is False
    assert good.verify(random.Random(1), params, ctx=ctx) is True  # an rng draws nonzero z below r
    assert bad.verify(random.Random(1), params) is False
