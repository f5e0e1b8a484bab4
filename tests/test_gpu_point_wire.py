"""The device codec for vectors of UNCOMPRESSED points (point_codec.hip's k_points_from_wire /
k_points_to_wire) through bh_srs_upload / bh_srs_read, Parameters (both encodings) and the ceremony's
uncompressed serializers, each also under BH_POINT_CODEC_HOST=1, which keeps the host loops.  Every
expected byte comes from oracle/bls12_381.py (tests/point_codec_points.py,
tests/params_compressed_model.py; their premises are pinned by tests/test_point_codec_cpu.py and
tests/test_params_compressed_cpu.py), never from the code under test.

Lengths 0, 1, 63, 64, 65, 255, 256 and 257 sit around the kernels' 64-lane block and the subgroup
kernel's 256-lane block; 257 has five blocks of 64 and a last block of one lane."""
import contextlib
import ctypes
import json
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import params_compressed_model as pm  # noqa: E402
import point_codec_points as pc  # noqa: E402
from oracle import bls12_381 as bls  # noqa: E402

pytestmark = pytest.mark.gpu

P, R = bls.P, bls.R
HERE = os.path.dirname(os.path.abspath(__file__))
INVALID_ENCODING, NOT_ON_CURVE, NOT_IN_SUBGROUP = 11, 12, 14
GROUPS = (1, 2)
LENGTHS = (0, 1, 63, 64, 65, 255, 256, 257)
LANES = (0, 63, 64, 255, 256)  # 256 is the last of 257
KNOB = "BH_POINT_CODEC_HOST"


def _bh():
    import bellman_hip as bh
    return bh


@contextlib.contextmanager
def codec(path):
    """Run the body on the device codec ("device": the knob unset) or on the host loops ("host")."""
    before = os.environ.pop(KNOB, None)
    if path == "host":
        os.environ[KNOB] = "1"
    try:
        yield 0 if path == "host" else 1
    finally:
        os.environ.pop(KNOB, None)
        if before is not None:
            os.environ[KNOB] = before


def _last():
    return _bh().lib().bh_srs_last_codec_device()


def _status(fn, *a, **kw):
    with pytest.raises(_bh().SynthesisError) as e:
        fn(*a, **kw)
    return e.value.code


def _both_statuses(fn, *a, indicator=True, **kw):
    """The status of a failing call on the device codec, after checking that the host loops agree."""
    out = []
    for path in ("device", "host"):
        with codec(path) as want:
            out.append(_status(fn, *a, **kw))
            assert not indicator or _last() == want
    assert out[0] == out[1], "the device codec and the host loops disagree: %r" % (out,)
    return out[0]


@pytest.fixture(scope="module")
def vectors(ctx):
    """Per group: the 257 chosen points, their oracle bytes in both forms."""
    out = {}
    for group in GROUPS:
        pts = pc.points(group)
        out[group] = dict(pts=pts, unc=pc.uncompressed(group, pts), comp=pc.compressed(group, pts))
    return out


def _slice(v, group, lo, n, form):
    rec = pm.wire_bytes(group, form == "comp")
    return v[group][form][lo * rec:(lo + n) * rec]


# ---------------------------------------------------------------- 1. lengths
@pytest.mark.parametrize("checked", (False, True))
@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("n", LENGTHS)
def test_upload_and_read_at_every_length(ctx, vectors, group, n, checked):
    bh = _bh()
    unc, comp = _slice(vectors, group, 0, n, "unc"), _slice(vectors, group, 0, n, "comp")
    for path in ("device", "host"):
        with codec(path) as want:
            bases = bh.Bases(ctx, group, unc, checked=checked)
            assert _last() == want
            assert len(bases) == n
            assert bases.read(0, n) == unc
            assert _last() == want
        with codec("host" if path == "device" else "device") as other:  # the read looks at the knob itself
            assert bases.read(0, n) == unc
            assert _last() == (other if n else want)  # an empty read codes nothing
        assert bases.read(0, n, compressed=True) == comp
        if n:
            exps = [pow(0x1234567 * (i + 1), 5, R) for i in range(n)]
            E = bls.G1 if group == 1 else bls.G2
            k = sum(e * s for e, s in zip(exps, pc.scalars())) % R
            want_sum = pc.uncompressed(group, [E.to_affine(E.mul(E.generator(), k))])
            assert bh.multiexp(ctx, bases, 0, None, exps) == want_sum


# ---------------------------------------------------------------- 2. against the host loops
def _coordinate_records(group):
    """Records of in-range components that need not lie on the curve: every edge value in every
    component slot beside random values, and all-random records up to 70 (two blocks)."""
    rng = random.Random(0xC0DEC + group)
    slots = pm.slots(group)
    recs = []
    for k in range(slots):
        for v in pm.edge_values():
            comps = [rng.randrange(P) for _ in range(slots)]
            comps[k] = v
            recs.append(comps)
    recs.append([P - 1] * slots)
    recs.append([1] * slots)
    while len(recs) < 70:
        recs.append([rng.randrange(P) for _ in range(slots)])
    return b"".join(c.to_bytes(48, "big") for comps in recs for c in comps), len(recs)


@pytest.mark.parametrize("group", GROUPS)
def test_differential_against_the_host_loops(ctx, group):
    bh = _bh()
    data, n = _coordinate_records(group)
    assert n == 70 and len(data) == n * pm.wire_bytes(group)
    for up in ("device", "host"):
        with codec(up) as want:
            bases = bh.Bases(ctx, group, data, checked=False)
            assert _last() == want
        for down in ("device", "host"):
            with codec(down) as want:
                assert bases.read(0, n) == data, (up, down)
                assert _last() == want
                assert bases.read(3, 66) == data[3 * pm.wire_bytes(group):69 * pm.wire_bytes(group)]


# ---------------------------------------------------------------- 3. windows and identities
WINDOWS = ((0, 257), (1, 62), (1, 63), (62, 3), (63, 1), (63, 2), (64, 1), (31, 1), (0, 1), (250, 7), (255, 2),
           (256, 1), (130, 127), (257, 0))


@pytest.mark.parametrize("group", GROUPS)
def test_windows_and_identities(ctx, vectors, group):
    bh = _bh()
    n, at = pc.NPOINTS, (0, 31, pc.NPOINTS - 1)
    pts = [None if i in at else a for i, a in enumerate(vectors[group]["pts"])]
    unc, comp = pc.uncompressed(group, pts), pc.compressed(group, pts)
    rec = pm.wire_bytes(group)
    for i in at:
        assert unc[i * rec:(i + 1) * rec] == bytes([0x40]) + bytes(rec - 1)
    for up in ("device", "host"):
        for checked in (False, True):
            with codec(up):
                bases = bh.Bases(ctx, group, unc, checked=checked)
            for down in ("device", "host"):
                with codec(down):
                    for first, cnt in WINDOWS:
                        assert bases.read(first, cnt) == unc[first * rec:(first + cnt) * rec], (up, down, first, cnt)
            assert bases.to_compressed() == comp


# ---------------------------------------------------------------- 4. malformed records
def _cases():
    return [(g, c) for g in GROUPS for c in pm.invalid_cases(g)]


@pytest.mark.parametrize("group,case", _cases())
def test_invalid_records_are_refused(ctx, vectors, group, case):
    bh = _bh()
    rec, good = pm.wire_bytes(group), vectors[group]["unc"]
    for lane in LANES:
        data = bytearray(good)
        data[lane * rec:(lane + 1) * rec] = pm.invalid_record(group, case, good[lane * rec:(lane + 1) * rec])
        for checked in (False, True):
            assert _both_statuses(bh.Bases, ctx, group, bytes(data), checked=checked) == INVALID_ENCODING, (lane, checked)


@pytest.mark.parametrize("group", GROUPS)
def test_off_curve_points(ctx, vectors, group):
    bh = _bh()
    rec, good = pm.wire_bytes(group), vectors[group]["unc"]
    off = pc.uncompressed(group, [pm.off_curve_point(group)])
    for lane in LANES:
        data = bytearray(good)
        data[lane * rec:(lane + 1) * rec] = off
        assert _both_statuses(bh.Bases, ctx, group, bytes(data), checked=True) == NOT_ON_CURVE, lane
        for path in ("device", "host"):
            with codec(path):
                assert bh.Bases(ctx, group, bytes(data), checked=False).read(0, pc.NPOINTS) == bytes(data)


@pytest.mark.parametrize("group", GROUPS)
def test_off_subgroup_points(ctx, vectors, group):
    bh = _bh()
    rec, good = pm.wire_bytes(group), vectors[group]["unc"]
    sub = pc.uncompressed(group, [pm.off_subgroup_point(group)])
    for lane in LANES:
        data = bytearray(good)
        data[lane * rec:(lane + 1) * rec] = sub
        assert _both_statuses(bh.Bases, ctx, group, bytes(data), checked=True) == NOT_IN_SUBGROUP, lane
        for path in ("device", "host"):
            with codec(path):
                assert bh.Bases(ctx, group, bytes(data), checked=False).read(0, pc.NPOINTS) == bytes(data)


@pytest.mark.parametrize("group", GROUPS)
def test_status_precedence(ctx, vectors, group):
    """An invalid record wins wherever it sits, then a point off the curve, then the subgroup."""
    bh = _bh()
    rec, good = pm.wire_bytes(group), vectors[group]["unc"]
    data = bytearray(good)
    data[10 * rec:11 * rec] = pc.uncompressed(group, [pm.off_curve_point(group)])
    data[100 * rec:101 * rec] = pc.uncompressed(group, [pm.off_subgroup_point(group)])
    assert _both_statuses(bh.Bases, ctx, group, bytes(data), checked=True) == NOT_ON_CURVE
    data[200 * rec:201 * rec] = pm.invalid_record(group, "slot1_eq_p", good[200 * rec:201 * rec])
    assert _both_statuses(bh.Bases, ctx, group, bytes(data), checked=True) == INVALID_ENCODING
    assert _both_statuses(bh.Bases, ctx, group, bytes(data), checked=False) == INVALID_ENCODING
    data[10 * rec:11 * rec] = good[10 * rec:11 * rec]
    assert _both_statuses(bh.Bases, ctx, group, bytes(data), checked=True) == INVALID_ENCODING
    data[200 * rec:201 * rec] = good[200 * rec:201 * rec]
    assert _both_statuses(bh.Bases, ctx, group, bytes(data), checked=True) == NOT_IN_SUBGROUP


# ---------------------------------------------------------------- 5. Parameters
@pytest.fixture(scope="module")
def mimc322():
    with open(os.path.join(HERE, "golden", "mimc322_params.bin"), "rb") as f:
        plain = f.read()
    with open(os.path.join(HERE, "golden", "mimc322.json")) as f:
        fx = json.load(f)
    return dict(plain=plain, comp=pm.compress_params(plain), fx=fx)


def _size_query(params, compressed):
    lib = _bh().lib()
    fn = lib.bh_params_write_compressed if compressed else lib.bh_params_write
    n = ctypes.c_size_t()
    assert fn(params.h, None, 0, ctypes.byref(n)) == 0
    return n.value


def test_parameters_in_both_encodings(ctx, mimc322):
    bh = _bh()
    plain, comp, fx = mimc322["plain"], mimc322["comp"], mimc322["fx"]
    for path in ("device", "host"):
        with codec(path):
            params = bh.Parameters.read(ctx, plain)
            assert params.write() == plain
            assert params.write(compressed=True) == comp
            assert _size_query(params, False) == len(plain) and _size_query(params, True) == len(comp)
            for checked in (True, False):
                back = bh.Parameters.read(ctx, comp, checked=checked, compressed=True)
                assert back.write() == plain
                assert back.write(compressed=True) == comp
                assert back.sizes() == params.sizes()
    proof = bh.prove_witness(ctx, back, bh.Witness.chain(ctx, fx["rounds"]), fx["r"], fx["s"])
    assert proof.hex() == fx["proof"]


def test_truncated_compressed_parameters(ctx, mimc322):
    bh = _bh()
    comp = mimc322["comp"]
    cuts = [0, len(comp) - 1]
    for name, group, start, n in pm.sections(comp, True):
        w = pm.wire_bytes(group, True)
        cuts += [start + w // 2, start + (n - 1) * w + w - 1]  # inside the first and the last point
        if not name.startswith("vk"):
            cuts += [start - 2, start]  # inside the length, and behind it
    for cut in sorted(set(cuts)):
        for checked in (False, True):
            assert _status(bh.Parameters.read, ctx, comp[:cut], checked=checked, compressed=True) == INVALID_ENCODING, cut


def test_identity_in_compressed_parameters(ctx, mimc322):
    bh = _bh()
    comp, plain = mimc322["comp"], mimc322["plain"]
    both = {name: (group, start, n) for name, group, start, n in pm.sections(plain, False)}
    for name, group, start, n in pm.sections(comp, True):
        if name.startswith("vk"):
            continue
        w, at = pm.wire_bytes(group, True), min(n - 1, 65)
        data = bytearray(comp)
        data[start + at * w:start + (at + 1) * w] = pc.compressed(group, [None])
        for checked in (False, True):
            assert _status(bh.Parameters.read, ctx, bytes(data), checked=checked, compressed=True) == INVALID_ENCODING
        # the uncompressed reader's status for the same defect
        _, ustart, _ = both[name]
        udata = bytearray(plain)
        udata[ustart + at * 2 * w:ustart + (at + 1) * 2 * w] = pc.uncompressed(group, [None])
        assert _both_statuses(bh.Parameters.read, ctx, bytes(udata), checked=False, indicator=False) == INVALID_ENCODING


def test_off_subgroup_point_in_l(ctx, mimc322):
    bh = _bh()
    comp, plain = mimc322["comp"], mimc322["plain"]
    _, group, start, n = [s for s in pm.sections(comp, True) if s[0] == "l"][0]
    _, _, ustart, _ = [s for s in pm.sections(plain, False) if s[0] == "l"][0]
    assert group == 1 and n > 70
    sub = pm.off_subgroup_point(1)
    data, udata = bytearray(comp), bytearray(plain)
    data[start + 70 * 48:start + 71 * 48] = pc.compressed(1, [sub])
    udata[ustart + 70 * 96:ustart + 71 * 96] = pc.uncompressed(1, [sub])
    want = _both_statuses(bh.Parameters.read, ctx, bytes(udata), checked=True)
    assert want == NOT_IN_SUBGROUP
    assert _status(bh.Parameters.read, ctx, bytes(data), checked=True, compressed=True) == want
    loaded = bh.Parameters.read(ctx, bytes(data), checked=False, compressed=True)
    assert loaded.write(compressed=True) == bytes(data) and loaded.write() == bytes(udata)
    for path in ("device", "host"):
        with codec(path):
            assert bh.Parameters.read(ctx, bytes(udata), checked=False).write() == bytes(udata)


# ---------------------------------------------------------------- 6. the ceremony
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
    """len -> (storage, contribution) of round two: on the matrix of a 16-row chain over the len-65
    storage, and on the six len-4 vectors of the small storage taken as they are (round two asks
    nothing of its vectors but their groups and pairwise lengths)."""
    bh = _bh()
    st, contrib = round_one[65]
    nxt = bh.verify_common_paramter_structure(ctx, st, contrib, rho=RHO)
    assert nxt is not None
    ust = bh.initial_uncommon_paramters(ctx, nxt.matrix(bh.R1CS.chain(ctx, 3)))
    small = bh.initial_uncommon_paramters(ctx, *[round_one[4][0].vector(k) for k in range(6)])
    return {4: (small, bh.mpc_uncommon_paramters_generator(ctx, small, PLAYER2)),
            65: (ust, bh.mpc_uncommon_paramters_generator(ctx, ust, PLAYER2))}


def _wire_round_trip(ctx, handle, want_size):
    """write() on both paths, read back on both paths: always the same bytes."""
    with codec("device") as want:
        plain = handle.write()
        assert _last() == want
    assert len(plain) == want_size
    with codec("host") as want:
        assert handle.write() == plain
        assert _last() == want
    back = None
    for path in ("device", "host"):
        for checked in (True, False):
            with codec(path) as want:
                back = type(handle).read(ctx, plain, checked=checked)
                assert _last() == want
            assert back.write() == plain
            assert back.write(compressed=True) == handle.write(compressed=True)
    return plain, back


@pytest.mark.parametrize("n", (4, 65))
def test_round_one_uncompressed_bytes(ctx, round_one, n):
    bh = _bh()
    st, contrib = round_one[n]
    _wire_round_trip(ctx, st, 4 + 576 + 864 * n)
    plain, _ = _wire_round_trip(ctx, contrib, 1152 + 3 * (4 + 576 * n))
    with codec("device"):
        back = bh.CommonParamter.read(ctx, plain)
    assert bh.verify_common_paramter_structure(ctx, st, back, rho=RHO) is not None


@pytest.mark.parametrize("n", (4, 65))
def test_round_two_uncompressed_bytes(ctx, round_two, n):
    ust, ucontrib = round_two[n]
    lens = [len(ust.vector(k)) for k in range(6)]
    assert lens[0] == lens[1] and lens[2] == lens[3] and lens[4] == lens[5] and min(lens) > 0
    assert n != 4 or lens == [4] * 6
    _wire_round_trip(ctx, ust, 576 + sum(4 + (192 if k & 1 else 96) * lens[k] for k in range(6)))
    _wire_round_trip(ctx, ucontrib, 1152 + sum(4 + 576 * lens[2 * j] for j in range(3)))


def test_ceremony_readers_keep_their_statuses(ctx, round_one):
    """A malformed record inside a contribution's interleaved list, and inside a storage vector."""
    bh = _bh()
    st, contrib = round_one[65]
    good = contrib.write()
    # element 64's g2_mine of the first list: the last lane of the second block
    at = 1152 + 4 + 64 * 576 + 384
    for case, want in (("slot2_eq_p", INVALID_ENCODING), ("sort_flag", INVALID_ENCODING)):
        data = bytearray(good)
        data[at:at + 192] = pm.invalid_record(2, case, good[at:at + 192])
        for checked in (False, True):
            assert _both_statuses(bh.CommonParamter.read, ctx, bytes(data), checked=checked) == want
    data = bytearray(good)
    data[at:at + 192] = pc.uncompressed(2, [pm.off_curve_point(2)])
    assert _both_statuses(bh.CommonParamter.read, ctx, bytes(data), checked=True) == NOT_ON_CURVE
    data[at:at + 192] = pc.uncompressed(2, [None])
    assert _both_statuses(bh.CommonParamter.read, ctx, bytes(data), checked=False) == INVALID_ENCODING
    sgood = st.write()
    sat = 4 + 576 + 64 * 96  # tau_g1[64]
    sdata = bytearray(sgood)
    sdata[sat:sat + 96] = pc.uncompressed(1, [pm.off_subgroup_point(1)])
    assert _both_statuses(bh.CommonParamterInStorage.read, ctx, bytes(sdata), checked=True) == NOT_IN_SUBGROUP
    for path in ("device", "host"):
        with codec(path):
            assert bh.CommonParamterInStorage.read(ctx, bytes(sdata), checked=False).write() == bytes(sdata)
