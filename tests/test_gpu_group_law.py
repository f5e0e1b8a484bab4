"""The group law of csrc/curve.cuh on caller-chosen representatives, against oracle/bls12_381.py.

bh_selftest_group_law (csrc/selftest_group.cuh) runs one CurveOps operation per launch on raw
29-bit limbs, in three separately compiled forms: G1, G2 with schoolbook Fp2 products and
carry-seeded columns (the reduction units), and G2 with column-wise Karatsuba products and split
columns (the bucket accumulation's unit).  The formulas hold under the bounds X < 10p, Y < 4p,
ZZ, ZZZ < 2p, which a multiexp only meets at typical representatives; here every coordinate is
placed at every multiple of p its bound allows (and at the largest representative a search over
z finds), the exceptional cases (p == a, p == -a, identities) are crossed with those
representatives so that Pd = 0 arrives as many different k p, and outputs are fed back as inputs
(dbl x4 then madd, the shape of k_varbase_mul_win) to show that output bounds are valid input
bounds.  Every result is checked bit-exactly: normalised limbs, the output bounds, ZZ^3 = ZZZ^2,
the identity exactly where the oracle has it (as all-zero limbs where the code returns
identity()), else the oracle's affine point.
"""
import ctypes
import functools
import itertools
import random

import numpy as np
import pytest

from oracle import bls12_381 as bls
from xyzz_device import G1, G2, P, XB, YB, ZB, as_u32, check_point, elem_limbs, elem_value

pytestmark = pytest.mark.gpu

MADD, MADD_NEG, ADD, DBL, DBL_AFFINE, REDUCE = range(6)
NIN = {MADD: 6, MADD_NEG: 6, ADD: 8, DBL: 4, DBL_AFFINE: 2, REDUCE: 4}
# unit -> (group, BH_COLUMN_CHAIN, BH_FP2_KARATSUBA defined)
UNITS = {0: (G1, 1, 0), 1: (G2, 1, 0), 2: (G2, 0, 1)}
GROUPS = {"G1": G1, "G2": G2}
NPOOL = 16


def _run(unit, op, rows):
    import bellman_hip as bh
    f = bh.lib().bh_selftest_group_law
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                  ctypes.c_void_p]
    grp, chain, kara = UNITS[unit]
    inp = as_u32(rows)
    assert inp.shape == (len(rows), NIN[op] * grp.fw)
    out = np.zeros((len(rows), grp.pw), dtype=np.uint32)
    info = np.zeros(2, dtype=np.uint32)
    assert f(0, unit, op, inp.ctypes.data, len(rows), out.ctypes.data, info.ctypes.data) == 0
    # the unit really is the form it stands for
    assert (int(info[0]), int(info[1])) == (chain, kara), (unit, info)
    return out


# ------------------------------------------------------------------ oracle side (shared by the units)
@functools.lru_cache(maxsize=None)
def _scalars():
    rng = random.Random(381)
    return tuple(rng.randrange(1, 1 << 64) for _ in range(NPOOL))


@functools.lru_cache(maxsize=None)
def _mul_gen(name, k):
    c = GROUPS[name].curve
    return c.to_affine(c.mul(c.generator(), k % bls.R))


def _pool(grp):
    return [_mul_gen(grp.name, k) for k in _scalars()]


@functools.lru_cache(maxsize=None)
def _sum(name, a, b):
    """a + b of affine points (None: the identity), Jacobian"""
    c = GROUPS[name].curve
    return c.add(c.from_affine(a), c.from_affine(b))


def _neg(grp, a):
    return None if a is None else (a[0], grp.F.neg(a[1]))


def _ks(grp, kx, ky, kzz, kzzz):
    return tuple((k,) * grp.nc if isinstance(k, int) else tuple(k) for k in (kx, ky, kzz, kzzz))


def _xyzz(grp, a, z, ks):
    """(x z^2, y z^3, z^2, z^3) in Montgomery form plus ks[coordinate][component] * p"""
    F = grp.F
    z2 = F.sqr(z)
    z3 = F.mul(z2, z)
    coords = (F.mul(a[0], z2), F.mul(a[1], z3), z2, z3)
    return [tuple(c + k * P for c, k in zip(grp.mont(o), kk)) for o, kk in zip(coords, ks)]


def _affine(grp, a):
    return [grp.mont(a[0]), grp.mont(a[1])]


def _rand_z(grp, rng):
    return grp.oracle(tuple(rng.randrange(1, P) for _ in range(grp.nc)))


def _one(grp):
    return grp.F.one


@functools.lru_cache(maxsize=None)
def _extreme_z(name, idx, coord):
    """the z (of 512 tried, 2 048 for Fp2) whose x z^2 (coord 0) or y z^3 (coord 1) has the largest Montgomery
    residue in its smallest component: with k = 9 (or 3) the largest representative below the bound"""
    grp = GROUPS[name]
    F, a, rng = grp.F, _pool(grp)[idx], random.Random(1000 * idx + coord)
    best, best_z = -1, None
    for _ in range(512 * grp.nc * grp.nc):
        z = _rand_z(grp, rng)
        z2 = F.sqr(z)
        v = F.mul(a[0], z2) if coord == 0 else F.mul(a[1], F.mul(z2, z))
        m = min(grp.mont(v))
        if m > best:
            best, best_z = m, z
    assert best > P - P // 8
    return best_z


def _identity_forms(grp, rng):
    """the identity as stored by identity() and as ZZ = p with arbitrary X, Y inside their bounds"""
    zero = [(0,) * grp.nc] * 4
    x = tuple(rng.randrange(XB * P) for _ in range(grp.nc))
    y = tuple(rng.randrange(YB * P) for _ in range(grp.nc))
    return [zero, [x, y, (P,) * grp.nc, (P,) * grp.nc], [x, y, (0,) * grp.nc, (P,) + (0,) * (grp.nc - 1)]]


CROSS = list(itertools.product(range(XB), range(YB), range(ZB), range(ZB)))   # 160 placements


class Cases:
    def __init__(self, grp):
        self.grp, self.rows, self.meta = grp, {op: [] for op in NIN}, {op: [] for op in NIN}

    def put(self, op, elems, want, zero_form=False, tag=None, bounds=(XB, YB, ZB, ZB)):
        self.rows[op].append([w for e in elems for w in elem_limbs(e)])
        self.meta[op].append((want, zero_form, (op, tag), bounds))

    def madd(self, p_elems, pa, a, tag, neg_on_device=False):
        """p (affine value pa, None: identity) + a; neg_on_device: the base is handed over as -a
        and negated by neg_affine on the device, leaving y in (0, p]"""
        want = _sum(self.grp.name, pa, a)
        base = _affine(self.grp, _neg(self.grp, a) if neg_on_device else a)
        self.put(MADD_NEG if neg_on_device else MADD, p_elems + base, want,
                 zero_form=pa is not None and self.grp.curve.is_identity(want), tag=tag)

    def add(self, p_elems, pa, q_elems, qa, tag):
        want = _sum(self.grp.name, pa, qa)
        self.put(ADD, p_elems + q_elems, want,
                 zero_form=pa is not None and qa is not None and self.grp.curve.is_identity(want), tag=tag)

    def dbl(self, p_elems, pa, tag):
        self.put(DBL, p_elems, _sum(self.grp.name, pa, pa), tag=tag)

    def check(self, unit):
        total = 0
        for op in NIN:
            if not self.rows[op]:
                continue
            out = _run(unit, op, self.rows[op])
            for words, (want, zero_form, tag, bounds) in zip(out, self.meta[op]):
                check_point(self.grp, words, want, bounds=bounds, zero_form=zero_form, tag=tag)
            if op == REDUCE:    # coordinate by coordinate: the canonical value of the input
                fw = self.grp.fw
                for row, words in zip(self.rows[op], out):
                    for k in range(4):
                        got = elem_value(self.grp, [int(w) for w in words[k * fw:(k + 1) * fw]])
                        assert got == tuple(c % P for c in elem_value(self.grp, row[k * fw:(k + 1) * fw])), k
            total += len(out)
        return total


def _bound_cases(grp):
    rng = random.Random(10)
    cs = Cases(grp)
    pool = _pool(grp)
    one = _one(grp)
    top = _ks(grp, XB - 1, YB - 1, ZB - 1, ZB - 1)
    for n, (kx, ky, kzz, kzzz) in enumerate(CROSS):
        ks = _ks(grp, kx, ky, kzz, kzzz)
        a, b = pool[n % NPOOL], pool[(n + 5) % NPOOL]
        z, z2 = _rand_z(grp, rng), _rand_z(grp, rng)
        for dev in (False, True):
            cs.madd(_xyzz(grp, b, z, ks), b, a, ("generic", ks), dev)
            cs.madd(_xyzz(grp, a, one, ks), a, a, ("p == a, z = 1", ks), dev)
            cs.madd(_xyzz(grp, a, z, ks), a, a, ("p == a", ks), dev)
            cs.madd(_xyzz(grp, _neg(grp, a), one, ks), _neg(grp, a), a, ("p == -a, z = 1", ks), dev)
            cs.madd(_xyzz(grp, _neg(grp, a), z, ks), _neg(grp, a), a, ("p == -a", ks), dev)
        # the other operand of add gets the mirrored placement
        kq = _ks(grp, XB - 1 - kx, YB - 1 - ky, ZB - 1 - kzz, ZB - 1 - kzzz)
        cs.add(_xyzz(grp, a, z, ks), a, _xyzz(grp, b, z2, kq), b, ("generic", ks))
        cs.add(_xyzz(grp, a, z, ks), a, _xyzz(grp, a, z2, kq), a, ("p == q", ks))
        cs.add(_xyzz(grp, a, z, ks), a, _xyzz(grp, a, z2, ks), a, ("p == q, same k", ks))
        cs.add(_xyzz(grp, a, z, ks), a, _xyzz(grp, _neg(grp, a), z2, kq), _neg(grp, a), ("p == -q", ks))
        cs.add(_xyzz(grp, a, one, ks), a, _xyzz(grp, b, z2, top), b, ("z = 1, q at the maxima", ks))
        cs.dbl(_xyzz(grp, a, z, ks), a, ("generic", ks))
        cs.dbl(_xyzz(grp, b, one, ks), b, ("z = 1", ks))
        cs.put(REDUCE, _xyzz(grp, a, z, ks), _sum(grp.name, a, None), tag=("reduce", ks), bounds=(1, 1, 1, 1))
    # the largest representatives a search finds: X = 9p + (nearly p), Y = 3p + (nearly p)
    for idx in range(NPOOL):
        a, b = pool[idx], pool[(idx + 7) % NPOOL]
        for coord in (0, 1):
            z = _extreme_z(grp.name, idx, coord)
            tag = ("largest " + "XY"[coord], idx)
            for dev in (False, True):
                cs.madd(_xyzz(grp, a, z, top), a, b, tag, dev)
                cs.madd(_xyzz(grp, a, z, top), a, a, tag + ("p == a",), dev)
                cs.madd(_xyzz(grp, a, z, top), a, _neg(grp, a), tag + ("p == -a",), dev)
            zq = _extreme_z(grp.name, (idx + 7) % NPOOL, coord)
            cs.add(_xyzz(grp, a, z, top), a, _xyzz(grp, b, zq, top), b, tag)
            cs.add(_xyzz(grp, a, z, top), a, _xyzz(grp, a, _rand_z(grp, rng), top), a, tag + ("p == q",))
            cs.add(_xyzz(grp, a, z, top), a, _xyzz(grp, _neg(grp, a), _rand_z(grp, rng), top), _neg(grp, a),
                   tag + ("p == -q",))
            cs.dbl(_xyzz(grp, a, z, top), a, tag)
        cs.put(DBL_AFFINE, _affine(grp, a), _sum(grp.name, a, a), tag=idx)
        cs.put(DBL_AFFINE, _affine(grp, _neg(grp, a)), _sum(grp.name, _neg(grp, a), _neg(grp, a)), tag=-idx)
    # identities, in both stored forms
    for n, ident in enumerate(_identity_forms(grp, rng) * 4):
        a, b = pool[n % NPOOL], pool[(n + 3) % NPOOL]
        q = _xyzz(grp, b, _rand_z(grp, rng), top if n % 2 else _ks(grp, 0, 0, 0, 0))
        for dev in (False, True):
            cs.madd(ident, None, a, ("identity + a", n), dev)
        cs.add(ident, None, q, b, ("identity + q", n))
        cs.add(q, b, ident, None, ("p + identity", n))
        cs.add(ident, None, _identity_forms(grp, rng)[(n + 1) % 3], None, ("identity + identity", n))
        cs.dbl(ident, None, ("2 identity", n))
    return cs


def _random_cases(grp):
    rng = random.Random(2026)
    cs = Cases(grp)
    pool = _pool(grp)

    def rks():
        return tuple(tuple(rng.randrange(b) for _ in range(grp.nc)) for b in (XB, YB, ZB, ZB))

    def rpoint(a):
        return _xyzz(grp, a, _rand_z(grp, rng), rks())

    def partner(a):
        u = rng.random()
        return a if u < 0.125 else _neg(grp, a) if u < 0.25 else rng.choice(pool)

    for n in range(1024):
        a = rng.choice(pool)
        for dev in (False, True):
            b = partner(a)
            if rng.random() < 1 / 16:
                cs.madd(rng.choice(_identity_forms(grp, rng)), None, b, ("random", n), dev)
            else:
                cs.madd(rpoint(a), a, b, ("random", n), dev)
        b = partner(a)
        cs.add(rpoint(a), a, rpoint(b), b, ("random", n))
        cs.dbl(rpoint(a), a, ("random", n))
        d = grp.curve.to_affine(_sum(grp.name, *sorted((a, rng.choice(pool)))))
        if rng.random() < 0.5:
            d = _neg(grp, d)
        cs.put(DBL_AFFINE, _affine(grp, d), _sum(grp.name, d, d), tag=("random", n))
        # reduce takes any representative below 128p
        pt = [tuple(c + rng.randrange(127) * P for c in e) for e in _xyzz(grp, a, _rand_z(grp, rng), _ks(grp, 0, 0, 0, 0))]
        cs.put(REDUCE, pt, _sum(grp.name, a, None), tag=("random", n), bounds=(1, 1, 1, 1))
    return cs


@pytest.mark.parametrize("unit", sorted(UNITS))
def test_group_law_at_the_operand_bounds(unit):
    assert _bound_cases(UNITS[unit][0]).check(unit) > 2000


@pytest.mark.parametrize("unit", sorted(UNITS))
def test_group_law_on_random_representatives(unit):
    assert _random_cases(UNITS[unit][0]).check(unit) == 6 * 1024


@functools.lru_cache(maxsize=None)
def _feedback_plan(name):
    """lanes of (start point, its affine value, base): acc <- 16 acc + base, three rounds.  The
    first lanes choose the base so that the madd of round 1, 2 or 3 meets acc == base (a doubling
    of a lazily reduced sum) or acc == -base (the identity, then doublings of it and a restart)."""
    grp = GROUPS[name]
    rng = random.Random(77)
    r = bls.R
    lanes = []
    for i in range(48):
        k = _scalars()[i % NPOOL] + i
        special = {0: 16, 1: -16, 2: -256 * pow(15, -1, r), 3: -256 * pow(17, -1, r),
                   4: -4096 * pow(271, -1, r), 5: -4096 * pow(273, -1, r)}
        kb = k * special[i] % r if i in special else _scalars()[(5 * i + 3) % NPOOL]
        pa = _mul_gen(name, k)
        ks = tuple(tuple(rng.randrange(b) for _ in range(grp.nc)) for b in (XB, YB, ZB, ZB))
        start = [(0,) * grp.nc] * 4 if i == 6 else _xyzz(grp, pa, _rand_z(grp, rng), ks)
        lanes.append((start, None if i == 6 else pa, _mul_gen(name, kb)))
    return lanes


@pytest.mark.parametrize("unit", sorted(UNITS))
def test_outputs_re_enter_as_inputs_dbl4_madd(unit):
    grp = UNITS[unit][0]
    c = grp.curve
    lanes = _feedback_plan(grp.name)
    rows = [[w for e in start for w in elem_limbs(e)] for start, _, _ in lanes]
    want = [c.from_affine(pa) for _, pa, _ in lanes]
    bases = [[w for e in _affine(grp, a) for w in elem_limbs(e)] for _, _, a in lanes]
    exceptional = 0
    for rnd in range(3):
        for d in range(4):
            out = _run(unit, DBL, rows)
            want = [c.double(w) for w in want]
            for i, (words, w) in enumerate(zip(out, want)):
                check_point(grp, words, w, tag=("dbl", rnd, d, i))
            rows = [list(map(int, words)) for words in out]
        out = _run(unit, MADD, [row + b for row, b in zip(rows, bases)])
        for i, (words, w, (_, _, a)) in enumerate(zip(out, want, lanes)):
            s = c.add(w, c.from_affine(a))
            hit_neg = not c.is_identity(w) and c.is_identity(s)
            exceptional += hit_neg or (not c.is_identity(w) and c.to_affine(w) == a)
            check_point(grp, words, s, zero_form=hit_neg, tag=("madd", rnd, i))
            want[i] = s
        rows = [list(map(int, words)) for words in out]
    assert exceptional == 6
