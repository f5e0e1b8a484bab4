"""Raw device limbs <-> Python integers, and the checks every device XYZZ point must pass.

Shared by test_gpu_group_law.py, test_gpu_accumulate.py and test_gpu_reduce.py.  A device Fp value is 14 little-endian
29-bit limbs in Montgomery form (x * 2^406 mod p), any representative the bounds of
csrc/curve.cuh allow; an Fp2 value is two of them (c0, c1).  Field elements are tuples of
integer components here (1 for G1, 2 for G2); the expected points come from oracle/bls12_381.py.
"""
import numpy as np

from oracle import bls12_381 as bls

P = bls.P
BITS, MASK, NP = 29, (1 << 29) - 1, 14
RM = (1 << (BITS * NP)) % P
RINV = pow(RM, -1, P)
XB, YB, ZB = 10, 4, 2       # X < 10p, Y < 4p, ZZ, ZZZ < 2p (CurveOps with MB = 2)


class Group:
    def __init__(self, name, curve, nc):
        self.name, self.curve, self.F, self.nc = name, curve, curve.F, nc
        self.fw = nc * NP                       # words per field element
        self.pw = 4 * self.fw                   # words per XYZZ point

    def elem(self, o):
        """oracle element -> tuple of canonical components"""
        return (o,) if self.nc == 1 else tuple(o)

    def oracle(self, e):
        """tuple of components (any representatives) -> oracle element"""
        return e[0] % P if self.nc == 1 else (e[0] % P, e[1] % P)

    def mont(self, o):
        """oracle element -> canonical Montgomery components"""
        return tuple(c * RM % P for c in self.elem(o))

    def demont(self, e):
        """device components (any representatives) -> oracle element"""
        return self.oracle(tuple(c * RINV for c in e))


G1 = Group("G1", bls.G1, 1)
G2 = Group("G2", bls.G2, 2)


def limbs(v):
    """14 limbs of v; the top limb takes every bit from 2^377 up (values up to 128p fit 32 bits)"""
    assert 0 <= v < 1 << (BITS * (NP - 1) + 32)
    return [(v >> (BITS * i)) & MASK for i in range(NP - 1)] + [v >> (BITS * (NP - 1))]


def value(ls):
    return sum(int(v) << (BITS * i) for i, v in enumerate(ls))


def elem_limbs(e):
    return [w for c in e for w in limbs(c)]


def elem_value(grp, words):
    """fw words -> tuple of component integers"""
    return tuple(value(words[k * NP:(k + 1) * NP]) for k in range(grp.nc))


def point_values(grp, words):
    """pw words -> (X, Y, ZZ, ZZZ) component tuples"""
    return tuple(elem_value(grp, words[k * grp.fw:(k + 1) * grp.fw]) for k in range(4))


def check_point(grp, words, want, bounds=(XB, YB, ZB, ZB), zero_form=False, tag=None):
    """words: one device XYZZ result (pw raw words).  want: the oracle's Jacobian (X, Y, Z) point.
    Limbs below the top one < 2^29, coordinates below their bounds, ZZ^3 = ZZZ^2, the identity
    exactly when ZZ = 0 (zero_form: as all-zero limbs), else (X / ZZ, Y / ZZZ) = want."""
    F = grp.F
    words = [int(w) for w in words]
    for k in range(4 * grp.nc):
        assert all(w <= MASK for w in words[k * NP:(k + 1) * NP - 1]), ("limb", tag)
    X, Y, ZZ, ZZZ = point_values(grp, words)
    for name, e, b in zip("X Y ZZ ZZZ".split(), (X, Y, ZZ, ZZZ), bounds):
        assert all(c < b * P for c in e), ("bound", name, tag)
    x, y, zz, zzz = (grp.demont(e) for e in (X, Y, ZZ, ZZZ))
    assert F.mul(F.sqr(zz), zz) == F.sqr(zzz), ("ZZ^3 != ZZZ^2", tag)
    if grp.curve.is_identity(want):
        assert F.is_zero(zz), ("expected the identity", tag)
        if zero_form:
            assert not any(words), ("identity not in its stored all-zero form", tag)
        return
    assert not F.is_zero(zz), ("unexpected identity", tag)
    wx, wy, wz = want
    z2 = F.sqr(wz)
    assert F.mul(x, z2) == F.mul(wx, zz), ("x", tag)
    assert F.mul(y, F.mul(z2, wz)) == F.mul(wy, zzz), ("y", tag)


def as_u32(rows):
    return np.ascontiguousarray(np.array(rows, dtype=np.uint64).astype(np.uint32))
