"""The compressed Parameters model (tests/params_compressed_model.py) on the oracle's mimc322
Parameters, and the premises of every malformed record tests/test_gpu_point_wire.py feeds to the
device.  No GPU: everything here is oracle/bls12_381.py arithmetic."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import params_compressed_model as pm  # noqa: E402
import point_codec_points as pc  # noqa: E402
from oracle import bls12_381 as bls  # noqa: E402

P, R = bls.P, bls.R
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def fixture_bytes():
    with open(os.path.join(HERE, "golden", "mimc322_params.bin"), "rb") as f:
        return f.read()


def test_round_trip_is_the_identity_and_the_size_is_the_formula(fixture_bytes):
    plain = fixture_bytes
    counts = {name: n for name, _, _, n in pm.sections(plain, False) if not name.startswith("vk")}
    assert min(counts.values()) > 0
    assert len(plain) == pm.size(counts, False)
    comp = pm.compress_params(plain)
    assert len(comp) == pm.size(counts, True)
    assert {name: n for name, _, _, n in pm.sections(comp, True) if not name.startswith("vk")} == counts
    # every point carries the compression flag; both sort flags occur
    tops = set()
    for name, group, start, n in pm.sections(comp, True):
        w = pm.wire_bytes(group, True)
        tops |= {comp[start + i * w] >> 5 for i in range(n)}
    assert tops == {4, 5}
    assert pm.decompress_params(comp) == plain
    assert pm.compress_params(pm.decompress_params(comp)) == comp


def test_point_recode_matches_the_oracle_encoders():
    for group in (1, 2):
        pts = list(pc.points(group)[:6]) + [None]
        unc, comp = pc.uncompressed(group, pts), pc.compressed(group, pts)
        wu, wc = pm.wire_bytes(group), pm.wire_bytes(group, True)
        for i in range(len(pts)):
            assert pm.recode(group, unc[i * wu:(i + 1) * wu], True) == comp[i * wc:(i + 1) * wc]
            assert pm.recode(group, comp[i * wc:(i + 1) * wc], False) == unc[i * wu:(i + 1) * wu]


def _decode(group, rec, checked):
    return (bls.g1_from_uncompressed if group == 1 else bls.g2_from_uncompressed)(rec, checked=checked)


@pytest.mark.parametrize("group", (1, 2))
def test_invalid_records_are_what_they_claim(group):
    good = pc.uncompressed(group, [pc.points(group)[3]])
    assert _decode(group, good, True) == (True, pc.points(group)[3])
    cases = pm.invalid_cases(group)
    assert len(cases) == 5 + 3 * pm.slots(group) - 1
    for case in cases:
        rec = pm.invalid_record(group, case, good)
        assert len(rec) == len(good) and rec != good
        assert _decode(group, rec, False)[0] is False, case
    # what each one changes, and nothing else
    assert pm.invalid_record(group, "compression_flag", good)[0] >> 5 == 4
    assert pm.invalid_record(group, "sort_flag", good)[0] >> 5 == 1
    for where, at in (("first", 0), ("middle", len(good) // 2), ("last", len(good) - 1)):
        rec = pm.invalid_record(group, "inf_stray_" + where, good)
        assert rec[0] >> 5 == 2 and sum(bin(b).count("1") for b in rec) == 2 and rec[at] & 1
    for k in range(pm.slots(group)):
        for case, value in (("slot%d_eq_p" % k, P), ("slot%d_all_ones" % k, (1 << 381) - 1)):
            rec = pm.invalid_record(group, case, good)
            assert int.from_bytes(rec[48 * k:48 * k + 48], "big") == value >= P
            assert rec[0] >> 5 == 0, "no flag is set: the value alone is out of range"
            assert rec[:48 * k] == good[:48 * k] and rec[48 * k + 48:] == good[48 * k + 48:]
        if k:
            rec = pm.invalid_record(group, "slot%d_top_bits" % k, good)
            value = int.from_bytes(rec[48 * k:48 * k + 48], "big")
            assert value >= 1 << 383 and value & ((1 << 381) - 1) < P  # in range only if wrongly masked
            assert value & ((1 << 381) - 1) == int.from_bytes(good[48 * k:48 * k + 48], "big")


@pytest.mark.parametrize("group", (1, 2))
def test_off_curve_and_off_subgroup_points(group):
    E = bls.G1 if group == 1 else bls.G2
    off = pm.off_curve_point(group)
    rec = pc.uncompressed(group, [off])
    assert _decode(group, rec, False) == (True, off), "in range, flags clear"
    assert not E.on_curve_affine(off)
    assert _decode(group, rec, True)[0] is False
    sub = pm.off_subgroup_point(group)
    assert sub is not None and E.on_curve_affine(sub)
    assert not E.is_identity(E.mul(E.from_affine(sub), R))
    assert _decode(group, pc.uncompressed(group, [sub]), False) == (True, sub)
    assert _decode(group, pc.uncompressed(group, [sub]), True)[0] is False


def test_edge_values_are_in_range():
    vals = pm.edge_values()
    assert vals[:3] == (0, 1, P - 1) and all(0 <= v < P for v in vals)
    assert vals[3] == 1 << 380 and vals[3].bit_length() == P.bit_length() == 381
    assert vals[4] >> 96 == 0, "the top limbs are zero"


def test_identity_records():
    for group in (1, 2):
        assert pc.uncompressed(group, [None]) == bytes([0x40]) + bytes(pm.wire_bytes(group) - 1)
        assert pc.compressed(group, [None]) == bytes([0xC0]) + bytes(pm.wire_bytes(group, True) - 1)
