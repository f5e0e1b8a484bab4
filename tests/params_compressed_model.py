"""Model of the compressed Parameters layout and the uncompressed records the point-wire tests feed
to the device, computed with oracle/bls12_381.py and tests/point_codec_points.py only.

The compressed layout is Parameters::write's (groth16/mod.rs:260-290) with every point compressed:
alpha_g1, beta_g1 (48 B), beta_g2, gamma_g2 (96 B), delta_g1 (48 B), delta_g2 (96 B), the u32-BE ic
length and ic (48 B each), then h, l, a, b_g1 (48 B per point) and b_g2 (96 B per point), each
behind its u32-BE length.  tests/test_params_compressed_cpu.py pins every premise stated here."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import point_codec_points as pc  # noqa: E402
from oracle import bls12_381 as bls  # noqa: E402

P = bls.P
VK_GROUPS = (1, 1, 2, 2, 1, 2)
VECTORS = (("h", 1), ("l", 1), ("a", 1), ("b_g1", 1), ("b_g2", 2))


def wire_bytes(group, compressed=False):
    return pc.record_bytes(group) * (1 if compressed else 2)


# ---------------------------------------------------------------- one point
def point_from_uncompressed(group, rec):
    """The affine point of an uncompressed record (None: the identity); range and flags only."""
    ok, pt = (bls.g1_from_uncompressed if group == 1 else bls.g2_from_uncompressed)(rec, checked=False)
    assert ok, "not an uncompressed point"
    return pt


def point_from_compressed(group, rec):
    """The affine point of a compressed record: the root of x^3 + b the sort flag names."""
    flags = rec[0] >> 5
    assert flags & 4, "compression flag clear"
    if flags & 2:
        assert flags == 6 and not any(rec[1:]) and not rec[0] & 0x1F
        return None
    head = int.from_bytes(bytes([rec[0] & 0x1F]) + rec[1:48], "big")
    if group == 1:
        pt = pc.g1_lift(head, bool(flags & 1))
    else:
        pt = pc.g2_lift((int.from_bytes(rec[48:96], "big"), head), bool(flags & 1))
    assert pt is not None, "x^3 + b is no square"
    return pt


def recode(group, rec, to_compressed):
    if to_compressed:
        return pc.compressed(group, [point_from_uncompressed(group, rec)])
    return pc.uncompressed(group, [point_from_compressed(group, rec)])


# ---------------------------------------------------------------- the file
def sections(data, compressed):
    """[(name, group, start, count)] of every run of points in a Parameters file of either form; a
    length prefix sits in the four bytes before the runs named ic, h, l, a, b_g1, b_g2."""
    out, off = [], 0
    for k, group in enumerate(VK_GROUPS):
        out.append(("vk%d" % k, group, off, 1))
        off += wire_bytes(group, compressed)
    for name, group in (("ic", 1),) + VECTORS:
        n = int.from_bytes(data[off:off + 4], "big")
        off += 4
        out.append((name, group, off, n))
        off += n * wire_bytes(group, compressed)
    assert off == len(data), "trailing or missing bytes"
    return out


def convert(data, to_compressed):
    """Parameters bytes of one form -> the other."""
    out = bytearray()
    for name, group, start, n in sections(data, not to_compressed):
        if not name.startswith("vk"):
            out += n.to_bytes(4, "big")
        w = wire_bytes(group, not to_compressed)
        for i in range(n):
            out += recode(group, data[start + i * w:start + (i + 1) * w], to_compressed)
    return bytes(out)


def compress_params(data):
    return convert(data, True)


def decompress_params(data):
    return convert(data, False)


def size(counts, compressed):
    """The file size from the lengths alone; counts: dict ic, h, l, a, b_g1, b_g2."""
    g1, g2 = wire_bytes(1, compressed), wire_bytes(2, compressed)
    return (3 * g1 + 3 * g2 + 4 + counts["ic"] * g1 + 5 * 4
            + (counts["h"] + counts["l"] + counts["a"] + counts["b_g1"]) * g1 + counts["b_g2"] * g2)


# ---------------------------------------------------------------- uncompressed records that must fail
def slots(group):
    return 2 * group  # 48-byte components of an uncompressed record: 2 (G1), 4 (G2)


def _with_slot(good, k, value):
    return good[:48 * k] + value.to_bytes(48, "big") + good[48 * (k + 1):]


def invalid_cases(group):
    """Names of the records that every decoder must refuse as an invalid encoding."""
    n = slots(group)
    return (["compression_flag", "sort_flag", "inf_stray_first", "inf_stray_middle", "inf_stray_last"]
            + ["slot%d_eq_p" % k for k in range(n)] + ["slot%d_all_ones" % k for k in range(n)]
            + ["slot%d_top_bits" % k for k in range(1, n)])


def invalid_record(group, case, good):
    """An uncompressed record that must be refused, made from the valid record `good`."""
    size_ = wire_bytes(group)
    if case == "compression_flag":
        return bytes([good[0] | 0x80]) + good[1:]
    if case == "sort_flag":
        return bytes([good[0] | 0x20]) + good[1:]
    if case.startswith("inf_stray_"):
        b = bytearray(bytes([0x40]) + bytes(size_ - 1))
        b[dict(first=0, middle=size_ // 2, last=size_ - 1)[case[10:]]] |= 0x01
        return bytes(b)
    k = int(case[4:case.index("_")])
    if case.endswith("_eq_p"):
        return _with_slot(good, k, P)
    if case.endswith("_all_ones"):  # 2^381 - 1: every value bit under the flags
        return _with_slot(good, k, (1 << 381) - 1)
    if case.endswith("_top_bits"):  # a valid component with the three top bits set: no flags there
        return good[:48 * k] + bytes([good[48 * k] | 0xE0]) + good[48 * k + 1:]
    raise KeyError(case)


def off_curve_point(group):
    """In range, not on the curve: (1, 1) and (1 + 0u, 1 + 0u)."""
    return (1, 1) if group == 1 else ((1, 0), (1, 0))


def off_subgroup_point(group):
    """On the curve, outside the subgroup (tests/test_point_codec_cpu.py pins both)."""
    return pc.g1_lift(4, True) if group == 1 else pc.g2_lift((0, 1), False)


def edge_values():
    """Component values for the differential test: the ends of the range, a value with bit 380 set
    below p, and one whose top limbs are zero."""
    return (0, 1, P - 1, 1 << 380, (1 << 64) + 5)
