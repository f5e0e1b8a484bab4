"""The device codec for vectors of compressed points (point_codec.hip) through
bh_srs_upload_compressed / bh_srs_read_compressed and the ceremony's compressed serializers.  Every
expected byte comes from oracle/bls12_381.py (tests/point_codec_points.py; its premises are pinned
by tests/test_point_codec_cpu.py), never from the code under test.

Lengths 0, 1, 63, 64, 65 and 257 sit around the kernels' 64-lane block; 257 has five blocks and a
last block of one lane."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import point_codec_points as pc  # noqa: E402
from oracle import bls12_381 as bls  # noqa: E402

pytestmark = pytest.mark.gpu

P, R = bls.P, bls.R
UNEXPECTED_EOF, INVALID_ENCODING, NOT_IN_SUBGROUP = 2, 11, 14
GROUPS = (1, 2)


def _bh():
    import bellman_hip as bh
    return bh


def _status(fn, *a, **kw):
    with pytest.raises(_bh().SynthesisError) as e:
        fn(*a, **kw)
    return e.value.code


def _infinity(group, uncompressed=False):
    n = pc.record_bytes(group) * (2 if uncompressed else 1)
    return bytes([0x40 if uncompressed else 0xC0]) + bytes(n - 1)


@pytest.fixture(scope="module")
def vectors(ctx):
    """Per group: the 257 chosen points as an uncompressed-uploaded device vector, their oracle
    bytes in both forms.  The device vector is k_i * G by mul_each, read back and uploaded again."""
    bh = _bh()
    out = {}
    gens = bh.initial_common_paramters(ctx, pc.NPOINTS)
    for group in GROUPS:
        pts = pc.points(group)
        unc = gens.vector(group - 1).mul_each(pc.scalars()).read(0, pc.NPOINTS)
        assert unc == pc.uncompressed(group, pts), "mul_each differs from the oracle: not a codec failure"
        out[group] = dict(pts=pts, unc=unc, comp=pc.compressed(group, pts))
    return out


def _slice(v, group, lo, n, form):
    rec = pc.record_bytes(group) * (2 if form == "unc" else 1)
    return v[group][form][lo * rec:(lo + n) * rec]


# ---------------------------------------------------------------- 1. encode
@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("n", pc.LENGTHS)
def test_encode_matches_the_oracle(ctx, vectors, group, n):
    bases = _bh().Bases(ctx, group, _slice(vectors, group, 0, n, "unc"))
    assert bases.read(0, n, compressed=True) == _slice(vectors, group, 0, n, "comp")
    assert bases.to_compressed() == _slice(vectors, group, 0, n, "comp")
    if n > 1:  # both values of the sort flag
        assert {b >> 5 for b in bases.to_compressed()[::pc.record_bytes(group)]} == {4, 5}
    windows = [(1, n - 2)] if n >= 2 else []
    windows += [(63, 2)] if n >= 65 else []
    for first, cnt in windows:
        assert bases.read(first, cnt, compressed=True) == _slice(vectors, group, first, cnt, "comp")


# ---------------------------------------------------------------- 2. decode
@pytest.mark.parametrize("checked", (False, True))
@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("n", pc.LENGTHS)
def test_decode_gives_the_uncompressed_bytes(ctx, vectors, group, n, checked):
    bases = _bh().Bases.from_compressed(ctx, group, _slice(vectors, group, 0, n, "comp"), checked=checked)
    assert len(bases) == n
    assert bases.read(0, n) == _slice(vectors, group, 0, n, "unc")


@pytest.mark.parametrize("group", GROUPS)
def test_multiexp_over_a_decoded_vector(ctx, vectors, group):
    bh = _bh()
    n = 65
    exps = [pow(0x1234567 * (i + 1), 5, R) for i in range(n)]
    plain = bh.Bases(ctx, group, _slice(vectors, group, 0, n, "unc"))
    decoded = bh.Bases.from_compressed(ctx, group, _slice(vectors, group, 0, n, "comp"))
    want = bh.multiexp(ctx, plain, 0, None, exps)
    assert bh.multiexp(ctx, decoded, 0, None, exps) == want
    # and the oracle's value of that sum
    E = bls.G1 if group == 1 else bls.G2
    k = sum(e * s for e, s in zip(exps, pc.scalars())) % R
    assert want == pc.uncompressed(group, [E.to_affine(E.mul(E.generator(), k))])


# ---------------------------------------------------------------- 3. the Fp2 sign rule at c1 = 0
def test_fp2_sort_flag_falls_to_c0_when_c1_is_zero(ctx):
    bh = _bh()
    _, (x, y) = pc.c1_zero_point()
    pts = [(x, y), (x, bls.Fp2Ops.neg(y))]
    unc, comp = pc.uncompressed(2, pts), pc.compressed(2, pts)
    bases = bh.Bases(ctx, 2, unc, checked=False)  # a curve point, not in the subgroup
    enc = bases.to_compressed()
    assert enc == comp
    assert enc[0] ^ enc[96] == 0x20 and enc[1:96] == enc[97:]
    assert bh.Bases.from_compressed(ctx, 2, enc, checked=False).read(0, 2) == unc


# ---------------------------------------------------------------- 4. the identity
@pytest.mark.parametrize("group", GROUPS)
def test_identities_round_trip(ctx, vectors, group):
    bh = _bh()
    n, at = 65, (0, 31, 64)
    pts = [None if i in at else a for i, a in enumerate(vectors[group]["pts"][:n])]
    unc, comp = pc.uncompressed(group, pts), pc.compressed(group, pts)
    rec = pc.record_bytes(group)
    for i in at:
        assert comp[i * rec:(i + 1) * rec] == _infinity(group)
        assert unc[2 * i * rec:2 * (i + 1) * rec] == _infinity(group, uncompressed=True)
    assert bh.Bases(ctx, group, unc).to_compressed() == comp
    for checked in (False, True):
        assert bh.Bases.from_compressed(ctx, group, comp, checked=checked).read(0, n) == unc
    good = vectors[group]["comp"][:n * rec]
    for i in at:
        sort_set = bytearray(good)
        sort_set[i * rec:(i + 1) * rec] = bytes([0xE0]) + bytes(rec - 1)
        assert _status(bh.Bases.from_compressed, ctx, group, bytes(sort_set), checked=False) == INVALID_ENCODING
        for byte in (0, rec // 2, rec - 1):  # a payload bit under the flags, in the middle, at the end
            payload = bytearray(good)
            payload[i * rec:(i + 1) * rec] = _infinity(group)
            payload[i * rec + byte] |= 0x01
            assert _status(bh.Bases.from_compressed, ctx, group, bytes(payload), checked=False) == INVALID_ENCODING


# ---------------------------------------------------------------- 5. malformed input
@pytest.mark.parametrize("group,case", pc.MALFORMED)
def test_malformed_records_are_refused(ctx, vectors, group, case):
    bh = _bh()
    n, rec = pc.NPOINTS, pc.record_bytes(group)
    good = vectors[group]["comp"]
    for lane in (0, 63, 64, n - 1):
        data = bytearray(good)
        data[lane * rec:(lane + 1) * rec] = pc.malformed(group, case, good[lane * rec:(lane + 1) * rec])
        assert _status(bh.Bases.from_compressed, ctx, group, bytes(data), checked=False) == INVALID_ENCODING


# ---------------------------------------------------------------- 6. the subgroup
@pytest.mark.parametrize("group", GROUPS)
def test_subgroup_is_what_checked_adds(ctx, vectors, group):
    bh = _bh()
    n, rec = 65, pc.record_bytes(group)
    off = pc.g1_lift(4, True) if group == 1 else pc.g2_lift((0, 1), False)
    pts = list(vectors[group]["pts"][:n])
    pts[40] = off
    comp, unc = pc.compressed(group, pts), pc.uncompressed(group, pts)
    assert _status(bh.Bases.from_compressed, ctx, group, comp, checked=True) == NOT_IN_SUBGROUP
    accepted = bh.Bases.from_compressed(ctx, group, comp, checked=False)
    assert accepted.read(0, n) == unc and accepted.to_compressed() == comp
    # a malformed record beside it wins, before and behind the off-subgroup point
    for lane in (3, 64):
        both = bytearray(comp)
        both[lane * rec:(lane + 1) * rec] = pc.malformed(group, "non_square", b"")
        assert _status(bh.Bases.from_compressed, ctx, group, bytes(both), checked=True) == INVALID_ENCODING


# ---------------------------------------------------------------- 7. the ceremony
PLAYER1 = (0x3C6EF372FE94F82BE7A1B0C5D2E3F4051627384950617283A4B5C6D7E8F90A1B % R,
           0x510E527FADE682D19B05688C2B3E6C1F1F83D9ABFB41BD6B5BE0CD19137E2179 % R,
           0x243F6A8885A308D313198A2E03707344A4093822299F31D0082EFA98EC4E6C89 % R)
PLAYER2 = (0x2B7E151628AED2A6ABF7158809CF4F3C762E7160F38B4DA56A784D9045190CFE % R,
           0x6F0E1D2C3B4A59687786A5B4C3D2E1F00112233445566778899AABBCCDDEEFF1 % R)
RHO = 0x5AB3F1C2D4E6978877665544332211FFEEDDCCBBAA99887766554433221100FF % R


@pytest.fixture(scope="module")
def round_one(ctx):
    """len -> (initial storage, a contribution to it)."""
    bh = _bh()
    out = {}
    for n in (4, 65):
        st = bh.initial_common_paramters(ctx, n)
        out[n] = (st, bh.mpc_common_paramters_generator(ctx, st, PLAYER1))
    return out


@pytest.fixture(scope="module")
def round_two(ctx, round_one):
    """(storage, contribution) of round two on the matrix of a 16-row chain over the len-65 storage."""
    bh = _bh()
    st, contrib = round_one[65]
    nxt = bh.verify_common_paramter_structure(ctx, st, contrib, rho=RHO)
    assert nxt is not None
    ust = bh.initial_uncommon_paramters(ctx, nxt.matrix(bh.R1CS.chain(ctx, 3)))
    return ust, bh.mpc_uncommon_paramters_generator(ctx, ust, PLAYER2)


def _round_trip(ctx, handle, want_size):
    plain = handle.write()
    comp = handle.write(compressed=True)
    assert len(comp) == want_size
    back = type(handle).read(ctx, comp, compressed=True)
    assert back.write() == plain
    assert type(handle).read(ctx, comp, checked=False, compressed=True).write() == plain
    return comp, back


@pytest.mark.parametrize("n", (4, 65))
def test_round_one_compressed_bytes(ctx, round_one, n):
    bh = _bh()
    st, contrib = round_one[n]
    _round_trip(ctx, st, 4 + 288 + 432 * n)
    _, back = _round_trip(ctx, contrib, 576 + 3 * (4 + 288 * n))
    assert bh.verify_common_paramter_structure(ctx, st, back, rho=RHO) is not None


def test_round_two_compressed_bytes(ctx, round_two):
    ust, ucontrib = round_two
    lens = [len(ust.vector(k)) for k in range(6)]
    assert lens[0] == lens[1] and lens[2] == lens[3] and lens[4] == lens[5] and min(lens) > 0
    _round_trip(ctx, ust, 288 + sum(4 + (96 if k & 1 else 48) * lens[k] for k in range(6)))
    _round_trip(ctx, ucontrib, 576 + sum(4 + 288 * lens[2 * j] for j in range(3)))


@pytest.mark.parametrize("which", ("storage", "contrib", "ustorage", "ucontrib"))
def test_ceremony_readers_refuse_bad_input(ctx, round_one, round_two, which):
    handle = dict(storage=round_one[4][0], contrib=round_one[4][1], ustorage=round_two[0],
                  ucontrib=round_two[1])[which]
    read = type(handle).read
    comp = handle.write(compressed=True)
    for checked in (False, True):
        assert _status(read, ctx, comp[:-1], checked=checked, compressed=True) == UNEXPECTED_EOF
        assert _status(read, ctx, comp + b"\x00", checked=checked, compressed=True) == INVALID_ENCODING
    # uncompressed bytes are not a compressed file: some error, and the library goes on working
    assert _status(read, ctx, handle.write(), compressed=True) in (UNEXPECTED_EOF, INVALID_ENCODING)
    assert read(ctx, comp, compressed=True).write(compressed=True) == comp


def test_compressed_identity_inside_a_storage_is_refused(ctx, round_one):
    bh = _bh()
    st, contrib = round_one[4]
    good = st.write(compressed=True)
    # tau_g1[2], then tau_g2[1]
    for at, group in ((4 + 288 + 2 * 48, 1), (4 + 288 + 4 * 48 + 96, 2)):
        data = bytearray(good)
        data[at:at + pc.record_bytes(group)] = _infinity(group)
        for checked in (False, True):
            assert _status(bh.CommonParamterInStorage.read, ctx, bytes(data), checked=checked,
                           compressed=True) == INVALID_ENCODING
    # a single point (alpha_g1) as the identity, through the host decoder
    head = bytearray(st.write(compressed=True))
    head[4:52] = _infinity(1)
    assert _status(bh.CommonParamterInStorage.read, ctx, bytes(head), compressed=True) == INVALID_ENCODING
    # and inside a contribution's interleaved list: element 1's g2_mine of the first list
    c = bytearray(contrib.write(compressed=True))
    at = 576 + 4 + 288 + 48 + 96 + 48
    c[at:at + 96] = _infinity(2)
    assert _status(bh.CommonParamter.read, ctx, bytes(c), compressed=True) == INVALID_ENCODING
