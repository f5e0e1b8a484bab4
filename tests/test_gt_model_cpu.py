"""The yardsticks of the target group's tests on the CPU (tests/gt_values.py): the relation between
the library's pairing convention and the crate's, pinned by the reference's known answer; the
gt_format codec; and the model of the cyclotomic-squaring formula against the dense square -- equal
on the cyclotomic subgroup, different elsewhere."""
import hashlib

import gt_values as gv
from oracle import pairing as pr


def test_generator_pairing_encodes_to_the_fixture():
    enc = gv.gt_format(gv.generator_pairing())
    assert enc == gv.fixture_bytes()
    assert enc[:8].hex() == "0f41e58663bf08cf" and enc[-8:].hex() == "a84305aaca1789b6"
    assert hashlib.sha256(enc).hexdigest() == "300e47c99502f3af33ad2080847d528cabd90365a90ab98bc174565c27928591"


def test_only_the_conjugate_cubed_matches_the_fixture():
    e0 = gv.library_pairing()
    cube = pr.f12_mul(pr.f12_sqr(e0), e0)
    want = gv.fixture_bytes()
    assert [gv.gt_format(v) == want for v in (e0, gv.conj(e0), cube, gv.conj(cube))] == [False, False, False, True]


def test_generator_pairing_has_order_r():
    e = gv.generator_pairing()
    assert pr.f12_pow(e, gv.R) == gv.ONE
    assert e != gv.ONE


def test_gt_parse_inverts_gt_format():
    for f in (gv.generator_pairing(), gv.random_f12(3), gv.ONE, gv.ZERO):
        b = gv.gt_format(f)
        assert len(b) == 576 and gv.gt_parse(b) == [tuple(c) for c in f]
        assert gv.gt_format(gv.gt_parse(b)) == b
    # the order: w^0's c0 is the last 48 bytes, w^5's c1 the first
    f = [(2 * k + 1, 2 * k + 2) for k in range(6)]
    b = gv.gt_format(f)
    assert int.from_bytes(b[-48:], "big") == 1 and int.from_bytes(b[:48], "big") == 12
    assert gv.flat_parse(gv.flat_bytes(f)) == f


def test_python_layer_codec_is_the_same():
    import bellman_hip as bh
    f = gv.random_f12(4)
    assert bh.gt_format(f) == gv.gt_format(f)
    assert bh.gt_parse(gv.gt_format(f)) == f


def test_model_equals_the_dense_square_on_the_cyclotomic_subgroup():
    for f in [gv.generator_pairing()] + [gv.easy_part_image(s) for s in (1, 2, 3)]:
        assert gv.cyclotomic_square_model(f) == pr.f12_sqr(f)


def test_model_differs_from_the_dense_square_on_a_random_value():
    f = gv.random_f12(5)
    assert gv.cyclotomic_square_model(f) != pr.f12_sqr(f)
    assert gv.cyclotomic_square_model(gv.ZERO) == gv.ZERO


def test_the_chosen_non_member_is_cyclotomic_and_outside_gt():
    m = gv.non_member()
    assert pr.f12_mul(m, gv.conj(m)) == gv.ONE
    assert pr.f12_pow(m, gv.R) != gv.ONE


def test_chosen_scalars_are_canonical_and_cover_the_digit_edges():
    s = gv.chosen_scalars()
    assert all(0 <= k < gv.R for k in s)
    assert {0, 1, 7, 8, 9, 15, 16, gv.R - 1, 1 << 254, gv.X_ABS} <= set(s)
    assert gv.power(gv.R - 1) == gv.conj(gv.generator_pairing())
