"""The batched final exponentiation on the device (csrc/pairing_dev.hip: k_fexp_load, k_fexp_steps,
k_fexp_store; bh_final_exponentiation_batch) against bh_final_exponentiation, the host's ladder, on
the values of tests/final_exp_values.py.  Field arithmetic is exact: every comparison is an
equality, all twelve coefficients.

Sizes sit on the edges of a wave and of a 64-thread block (63, 64, 65 values; 130: a third block,
short); the chosen values -- the ones that the new Fp12 helpers' lazy bounds can get wrong -- stand
in lanes 0, 63, 64 and n - 1, seeded random values elsewhere.  The host yardstick costs about 40 ms
per value and is kept per distinct value: a test uses at most 4 chosen and 30 random ones."""
import ctypes

import numpy as np
import pytest

import proof_cases as pc
from final_exp_values import ONE, P, SPECIAL, ladder, random_values, special_values, to_bytes, from_bytes
from oracle import bls12_381 as bls

pytestmark = pytest.mark.gpu

G1, G2 = bls.G1, bls.G2


def _bh():
    import bellman_hip as bh
    return bh


def _raw(ctx, blob, n, fill=0xAA):
    """bh_final_exponentiation_batch on raw bytes -> (status, output bytes)"""
    src = np.frombuffer(blob or b"\0", dtype=np.uint8)
    out = np.full(max(576 * n, 1), fill, dtype=np.uint8)
    st = _bh().lib().bh_final_exponentiation_batch(ctx.h, src.ctypes.data_as(ctypes.c_void_p), n,
                                                    out.ctypes.data_as(ctypes.c_void_p))
    return int(st), out.tobytes()


def _batch(n, rnd):
    """n values: four of the chosen ones (those of round rnd) at lanes 0, 63, 64, n - 1 where the batch
    has them, 30 random values tiled over the other lanes"""
    pool = random_values(30, seed=11)
    vals = [pool[(7 * i + rnd) % 30] for i in range(n)]
    chosen = special_values()[4 * rnd:4 * rnd + 4]
    for (_, v), lane in zip(chosen, sorted({0, 63, 64, n - 1})):
        if 0 <= lane < n:
            vals[lane] = v
    return vals


@pytest.mark.parametrize("rnd", range(len(SPECIAL) // 4))
@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_batch_equals_the_host_ladder(ctx, n, rnd):
    vals = _batch(n, rnd)
    got = _bh().final_exponentiation_batch(ctx, vals)
    assert len(got) == n
    for lane, (g, v) in enumerate(zip(got, vals)):
        assert g == ladder(to_bytes(v)), (n, rnd, lane)


def test_every_chosen_value_alone(ctx):
    """n = 1 per value, and all of them in one batch"""
    vals = [v for _, v in special_values()]
    want = [ladder(to_bytes(v)) for v in vals]
    assert _bh().final_exponentiation_batch(ctx, vals) == want
    for v, w in zip(vals, want):
        assert _bh().final_exponentiation_batch(ctx, [v]) == [w]


def test_no_values(ctx):
    assert _raw(ctx, b"", 0) == (0, b"\xaa")
    assert _bh().final_exponentiation_batch(ctx, []) == []


def test_output_may_be_the_input(ctx):
    vals = _batch(65, 1)
    buf = np.frombuffer(b"".join(to_bytes(v) for v in vals), dtype=np.uint8).copy()
    p = buf.ctypes.data_as(ctypes.c_void_p)
    assert _bh().lib().bh_final_exponentiation_batch(ctx.h, p, 65, p) == 0
    raw = buf.tobytes()
    assert [from_bytes(raw[576 * i:576 * i + 576]) for i in range(65)] == [ladder(to_bytes(v)) for v in vals]


@pytest.mark.parametrize("coefficient", [0, 5, 11])
def test_a_coefficient_equal_to_p_is_rejected_and_nothing_written(ctx, coefficient):
    vals = _batch(130, 0)
    blob = bytearray(b"".join(to_bytes(v) for v in vals))
    off = 576 * 64 + 48 * coefficient
    blob[off:off + 48] = P.to_bytes(48, "big")
    st, out = _raw(ctx, bytes(blob), 130)
    assert st == pc.INVALID_ENCODING
    assert out == b"\xaa" * (576 * 130)
    blob[off:off + 48] = (P - 1).to_bytes(48, "big")  # the largest canonical coefficient is accepted
    st, out = _raw(ctx, bytes(blob), 130)
    assert st == 0 and from_bytes(out[576 * 64:576 * 65]) == ladder(bytes(blob[576 * 64:576 * 65]))


def test_null_pointers(ctx):
    f = _bh().lib().bh_final_exponentiation_batch
    buf = np.zeros(576, dtype=np.uint8)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    assert f(None, p, 1, p) == pc.INVALID_ARGUMENT
    assert f(ctx.h, None, 1, p) == pc.INVALID_ARGUMENT
    assert f(ctx.h, p, 1, None) == pc.INVALID_ARGUMENT
    assert f(ctx.h, None, 0, None) == 0


def test_bilinearity_through_the_public_names(ctx):
    """e(a P, Q) = e(P, a Q): the Miller values differ, their final exponentiations agree"""
    bh = _bh()
    scalars = [2, 0xd201000000010001, bls.R - 1]
    p, q = G1.generator(), G2.generator()

    def miller(pp, qq):
        g1 = bh.Bases(ctx, bh.BH_G1, bls.g1_to_uncompressed(G1.to_affine(pp)), checked=False)
        g2 = bh.Bases(ctx, bh.BH_G2, bls.g2_to_uncompressed(G2.to_affine(qq)), checked=False)
        return bh.multi_miller_loop(ctx, g1, g2)

    left = [miller(G1.mul(p, a), q) for a in scalars]
    right = [miller(p, G2.mul(q, a)) for a in scalars]
    assert all(l != r for l, r in zip(left, right))
    out = bh.final_exponentiation_batch(ctx, left + right)
    assert out[:3] == out[3:]
    assert ONE not in out and len({to_bytes(v) for v in out[:3]}) == 3
    base = bh.final_exponentiation_batch(ctx, [miller(p, q)])[0]
    # e(P, Q)^(r - 1) is the inverse, which in the cyclotomic subgroup is the conjugate
    assert out[2] == [c if k % 2 == 0 else (-c[0] % P, -c[1] % P) for k, c in enumerate(base)]
    assert out[0] == bh.final_exponentiation(miller(G1.mul(p, 2), q))


def test_scratch_budget_keeps_its_worst_kernel(ctx):
    """the new kernels are in the list (six more than the Miller loop's three) and none is its worst:
    k_fexp_steps keeps 8 B per lane in its private segment"""
    _bh().final_exponentiation_batch(ctx, [ONE])
    rep = ctx.scratch_report()
    assert rep["fits"]
    assert not rep["worst_kernel"].startswith(("k_miller", "k_f12", "k_fexp", "k_each"))
    assert rep["worst_bytes_per_lane"] >= 1680
