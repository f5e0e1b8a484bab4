"""Chosen points for the point-codec tests, computed with oracle/bls12_381.py only: square roots
over Fp and Fp2, the curve points the tests put into their vectors, and records that must be
refused.  tests/test_point_codec_cpu.py pins every premise stated here."""
import functools

from oracle import bls12_381 as bls

P, R = bls.P, bls.R
F2 = bls.Fp2Ops
NPOINTS = 257
LENGTHS = (0, 1, 63, 64, 65, 257)  # around the 64-lane block


def fp_sqrt(a):
    """A square root of a in Fp, or None (p = 3 mod 4)."""
    y = pow(a, (P + 1) // 4, P)
    return y if y * y % P == a % P else None


def _fp2_pow(a, e):
    r = F2.one
    for bit in bin(e)[2:]:
        r = F2.sqr(r)
        if bit == "1":
            r = F2.mul(r, a)
    return r


def fp2_sqrt(a):
    """A square root of a in Fp2 = Fp[u]/(u^2 + 1), or None (Adj, Rodriguez-Henriquez, algorithm 9)."""
    if F2.is_zero(a):
        return a
    a1 = _fp2_pow(a, (P - 3) // 4)
    alpha = F2.mul(F2.sqr(a1), a)
    x0 = F2.mul(a1, a)
    if alpha == F2.neg(F2.one):
        x = ((-x0[1]) % P, x0[0])
    else:
        x = F2.mul(_fp2_pow(F2.add(F2.one, alpha), (P - 1) // 2), x0)
    return x if F2.sqr(x) == a else None


def g1_rhs(x):
    return (x * x * x + 4) % P


def g2_rhs(x):
    return F2.add(F2.mul(F2.sqr(x), x), (4, 4))


def g1_lift(x, largest):
    """The curve point with this x whose y has lex_largest(y) == largest, or None."""
    y = fp_sqrt(g1_rhs(x))
    if y is None:
        return None
    return (x, y if bls.fp_lex_largest(y) == largest else P - y)


def g2_lift(x, largest):
    y = fp2_sqrt(g2_rhs(x))
    if y is None:
        return None
    return (x, y if bls.fp2_lex_largest(y) == largest else F2.neg(y))


def magnitudes(n=NPOINTS):
    """k_i of 64 bits, every 16th of full width."""
    out = []
    for i in range(n):
        k = (0x9E3779B97F4A7C15 * (i + 1)) % (1 << 64) | 1
        out.append(pow(k, 4, R) if i % 16 == 5 else k)
    return out


def scalars(n=NPOINTS):
    """The scalars of points(): +k_i for even i, -k_i = r - k_i for odd i, so that both signs (and
    with them both values of the sort flag) occur in every block of 64."""
    return [k if i % 2 == 0 else R - k for i, k in enumerate(magnitudes(n))]


@functools.lru_cache(maxsize=None)
def points(group):
    """The affine points scalars()[i] * G, computed once."""
    E = bls.G1 if group == 1 else bls.G2
    out = []
    for i, k in enumerate(magnitudes()):
        a = E.to_affine(E.mul(E.generator(), k))
        out.append(a if i % 2 == 0 else (a[0], E.F.neg(a[1])))
    return tuple(out)


def uncompressed(group, pts):
    f = bls.g1_to_uncompressed if group == 1 else bls.g2_to_uncompressed
    return b"".join(f(a) for a in pts)


def compressed(group, pts):
    f = bls.g1_to_compressed if group == 1 else bls.g2_to_compressed
    return b"".join(f(a) for a in pts)


def record_bytes(group):
    return 48 if group == 1 else 96


@functools.lru_cache(maxsize=None)
def c1_zero_point():
    """The first b = 1, 2, ... for which x = a + b u, a^2 = (b^3 - 4) / (3 b), is a G2 curve point
    whose y = (c0, 0): the imaginary part of x^3 + 4 + 4u vanishes by the choice of a, the real part
    a^3 - 3 a b^2 + 4 must be a square c0^2.  Returns (b, point with the smaller y)."""
    for b in range(1, 64):
        a = fp_sqrt((b ** 3 - 4) * pow(3 * b, P - 2, P) % P)
        if a is None:
            continue
        for a_ in (a, P - a):
            c0 = fp_sqrt((a_ ** 3 - 3 * a_ * b * b + 4) % P)
            if c0 is not None:
                c0 = min(c0, P - c0)
                return b, ((a_, b), (c0, 0))
    raise AssertionError("no such point below b = 64")


def malformed(group, case, good):
    """A record that must be refused, made from the valid compressed record `good` or from scratch."""
    n = record_bytes(group)
    if case == "flag_clear":
        return bytes([good[0] & 0x7F]) + good[1:]
    if case == "x_eq_p":  # G2: c1 = p
        b = bytearray(P.to_bytes(48, "big") + bytes(n - 48))
    elif case == "c0_eq_p":  # G2 only: c1 = 1 < p, c0 = p
        b = bytearray((1).to_bytes(48, "big") + P.to_bytes(48, "big"))
    elif case == "non_square":  # x = 1
        b = bytearray(bytes(n - 1) + b"\x01")
    else:
        raise KeyError(case)
    b[0] |= 0x80
    return bytes(b)


MALFORMED = ((1, "flag_clear"), (1, "x_eq_p"), (1, "non_square"),
             (2, "flag_clear"), (2, "x_eq_p"), (2, "c0_eq_p"), (2, "non_square"))
