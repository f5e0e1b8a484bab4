"""The premises of tests/test_gpu_point_codec.py, checked with oracle/bls12_381.py alone, so that a
failure on the GPU points at a kernel and not at an input."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import point_codec_points as pc  # noqa: E402
from oracle import bls12_381 as bls  # noqa: E402

P, R = bls.P, bls.R


def _off_subgroup(E, a):
    return E.on_curve_affine(a) and not E.is_identity(E.mul(E.from_affine(a), R))


def test_square_roots_of_the_helper():
    for a in (4, 68, P - 1, 2):
        y = pc.fp_sqrt(a)
        assert y is None or y * y % P == a
    assert pc.fp_sqrt(4) in (2, P - 2) and pc.fp_sqrt(P - 1) is None  # p = 3 mod 4: -1 is no square
    for a in ((0, 1), (3, 0), (P - 1, 0), (5, 7)):
        sq = bls.Fp2Ops.sqr(a)
        y = pc.fp2_sqrt(sq)
        assert y in (a, bls.Fp2Ops.neg(a))
    assert pc.fp2_sqrt((0, 0)) == (0, 0)


def test_g1_x1_is_no_curve_point_and_x4_is_off_the_subgroup():
    assert pc.fp_sqrt(pc.g1_rhs(1)) is None
    for largest in (False, True):
        a = pc.g1_lift(4, largest)
        assert a is not None and bls.fp_lex_largest(a[1]) == largest
        assert _off_subgroup(bls.G1, a)


def test_g2_x0_x1_are_no_curve_points_and_xu_is_off_the_subgroup():
    assert pc.fp2_sqrt(pc.g2_rhs((0, 0))) is None
    assert pc.fp2_sqrt(pc.g2_rhs((1, 0))) is None
    for largest in (False, True):
        a = pc.g2_lift((0, 1), largest)
        assert a is not None and bls.fp2_lex_largest(a[1]) == largest
        assert _off_subgroup(bls.G2, a)


def test_the_search_finds_a_g2_point_with_real_y_at_b_2():
    b, (x, y) = pc.c1_zero_point()
    assert b == 2 and x[1] == 2 and y[1] == 0 and y[0] != 0
    assert bls.G2.on_curve_affine((x, y))
    neg = (x, bls.Fp2Ops.neg(y))
    # c1 = 0: the sort flag falls to c0, and the two points' flags differ
    assert not bls.fp2_lex_largest(y) and bls.fp2_lex_largest(neg[1])
    enc, enc_neg = bls.g2_to_compressed((x, y)), bls.g2_to_compressed(neg)
    assert enc[0] ^ enc_neg[0] == 0x20 and enc[1:] == enc_neg[1:]


def test_generators_compress_to_the_standard_constants():
    g1 = bls.g1_to_compressed(bls.G1_GEN)
    g2 = bls.g2_to_compressed(bls.G2_GEN)
    assert len(g1) == 48 and len(g2) == 96
    # the zcash test vectors' generator encodings begin with these bytes
    assert g1[:8].hex() == "97f1d3a73197d794"
    assert g2[:8].hex() == "93e02b6052719f60"


def test_chosen_vector_has_both_signs_in_every_block():
    for group in (1, 2):
        pts = pc.points(group)
        assert len(pts) == pc.NPOINTS and len(set(pts)) == pc.NPOINTS
        enc = pc.compressed(group, pts)
        n = pc.record_bytes(group)
        flags = [enc[i * n] >> 5 for i in range(pc.NPOINTS)]
        for lo in range(0, pc.NPOINTS - 1, 64):
            assert {4, 5} <= set(flags[lo:lo + 64]) or lo + 1 >= pc.NPOINTS
        # the points are the scalars' multiples: spot-check the oracle against itself
        E = bls.G1 if group == 1 else bls.G2
        for i in (0, 1, 5):
            assert E.to_affine(E.mul(E.generator(), pc.scalars()[i])) == pts[i]


def test_malformed_records_are_what_they_claim():
    for group, case in pc.MALFORMED:
        n = pc.record_bytes(group)
        good = pc.compressed(group, pc.points(group)[:1])
        bad = pc.malformed(group, case, good)
        assert len(bad) == n
        c_first = int.from_bytes(bytes([bad[0] & 0x1F]) + bad[1:48], "big")
        if case == "flag_clear":
            assert bad[0] >> 7 == 0 and bad[1:] == good[1:]
            continue
        assert bad[0] >> 5 == 4  # compressed, not infinity, sort clear
        if case == "x_eq_p":
            assert c_first == P
        elif case == "c0_eq_p":
            assert c_first == 1 and int.from_bytes(bad[48:], "big") == P
        else:
            assert c_first == 1 if group == 1 else (c_first == 0 and int.from_bytes(bad[48:], "big") == 1)
