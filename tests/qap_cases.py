"""Hand-made circuits whose QAP values at tau are prescribed exactly, for the generator's identity
filter (csrc/r1cs.hip: k_r1cs_ext, k_r1cs_compact) against oracle/bellman.py:generate_parameters.

A column with the single term (c, row i) has the value c L_i(tau), and L_i(tau) is known on the
host, so u_j = A_j(tau), v_j = B_j(tau) and e_j = (beta u_j + alpha v_j + w_j) / (gamma | delta) of
every variable can be set to any field element: 0 (by an empty column, a zero coefficient or a
cancellation), -1 (whose device Montgomery forms the carry-dropping fe_is_zero of csrc/field.cuh
took for zero), the values next to them, and a full-width one.  Everything not targeted is a small
integer, which keeps the oracle's fixed-base multiplications short.  No GPU import here.
"""
import functools
import random

from oracle import bellman as bm
from oracle import circuits as cc

E = bm.BLS12_381
R = E.Fr.q
P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
BITS = 29
FR_LIMBS, FP_LIMBS = 9, 14
FR_TOP = 1 << (BITS * FR_LIMBS)   # 2^261, the device's Montgomery radix for Fr
SEGMENT = 32                      # R1CS_S of csrc/r1cs.h: bh_r1cs_sizes()["segment"]
SMALL_BITS = 16                   # every value that is not targeted is below 2^16
FORK = dict(alpha=6, beta=24, gamma=6, delta=24, tau=2)
_full = cc.fr_stream(20261021, 5, R)
FULL = dict(zip(("alpha", "beta", "gamma", "delta", "tau"), _full))
assert all(t.bit_length() > 200 for t in _full)


def inv(x):
    return pow(x % R, R - 2, R)


# the targets by name.  -1 is what the old predicate dropped; 2^261 mod r and its negative are the
# canonical values next to the wrap; +-2^-261 are the values whose device forms are 1 and r - 1
TARGETS = {
    "0": 0, "-1": R - 1, "1": 1, "-2": R - 2,
    "top": FR_TOP % R, "-top": -FR_TOP % R,
    "inv": inv(FR_TOP), "-inv": -inv(FR_TOP) % R,
    "rand": cc.fr_stream(77, 1, R)[0],
}
WAYS = ("empty", "zero_coeff", "one", "two", "segments", "long")
NONEMPTY = ("one", "two", "segments", "long")


def target(t):
    return TARGETS[t] if isinstance(t, str) else t % R


# ------------------------------------------------------------------ fe_is_zero on 29-bit limbs
def fe_is_zero_kmax(p, n):
    """The multiples k p the comparison can see: k < 128 and k p below 2^(29 n)."""
    return min(127, ((1 << (BITS * n)) - 1) // p)


def fe_is_zero_model(x, p, n, kmax=127):
    """csrc/field.cuh:fe_is_zero on the n normalised limbs of x < 2^(29 n): k from the low limb, then
    the limbs of k p, the carry out of the top limb dropped, against the limbs of x.  kmax = 127 is
    the predicate before the bound on k; fe_is_zero_kmax(p, n) the one that holds its contract."""
    assert 0 <= x < 1 << (BITS * n)
    mask = (1 << BITS) - 1
    k = (x & mask) * pow(p, -1, 1 << BITS) & mask
    if k > kmax:
        return False
    carry, diff = 0, 0
    for i in range(n):
        t = ((p >> (BITS * i)) & mask) * k + carry
        diff |= (t & mask) ^ ((x >> (BITS * i)) & mask)
        carry = t >> BITS
    return diff == 0


# ------------------------------------------------------------------ circuits of prescribed terms
class TermCircuit:
    """ni inputs (ONE, which the constraint system allocates itself, is the first), na aux variables
    and nc constraints whose linear combinations are the per-variable [(coeff, row)] lists A, B, C
    (n = ni + na lists each, row < nc).  A column keeps its number of terms, duplicates of a row
    included; its terms come out ordered by row."""

    def __init__(self, ni, na, nc, A, B, C):
        n = ni + na
        assert ni >= 1 and len(A) == len(B) == len(C) == n
        assert all(0 <= row < nc for M in (A, B, C) for col in M for _, row in col)
        self.ni, self.na, self.nc, self.A, self.B, self.C = ni, na, nc, A, B, C

    def synthesize(self, cs):
        vs = [cs.one()] + [cs.alloc_input("", lambda: None) for _ in range(self.ni - 1)]
        vs += [cs.alloc("", lambda: None) for _ in range(self.na)]
        rows = [[[] for _ in range(self.nc)] for _ in range(3)]
        for k, M in enumerate((self.A, self.B, self.C)):
            for j, col in enumerate(M):
                for c, row in col:
                    rows[k][row].append((c, vs[j]))

        def lc_of(terms):
            def f(lc):
                for t in terms:
                    lc = lc + t
                return lc
            return f

        for i in range(self.nc):
            cs.enforce("", lc_of(rows[0][i]), lc_of(rows[1][i]), lc_of(rows[2][i]))


def lagrange(tau, num_constraints):
    """L_i(tau), i < m, as generate_parameters computes them: the ifft of the powers of tau."""
    dom = bm.EvaluationDomain(E, [0] * num_constraints)
    m = len(dom.coeffs)
    assert tau % R and pow(tau, m, R) != 1, "tau must lie outside the domain"
    dom.coeffs = [pow(tau, i, R) for i in range(m)]
    dom.ifft()
    assert all(dom.coeffs)
    return dom.coeffs


def _column(rng, lag, nc, value, way, S):
    """Terms on rows < nc whose sum of coeff * L_row(tau) is value."""
    value %= R
    if way == "empty":
        assert value == 0
        return []
    if way == "zero_coeff":
        assert value == 0
        return [(0, rng.randrange(nc))]
    if way == "one":
        i = rng.randrange(nc)
        return [(value * inv(lag[i]) % R, i)]
    if way == "two":
        i, k = rng.sample(range(nc), 2)
        t = rng.randrange(1, R)
        return [(t * inv(lag[i]) % R, i), ((value - t) * inv(lag[k]) % R, k)]
    count = {"segments": S + 1, "long": S * S + 1}[way]
    first = rng.randrange(nc)
    col = [(rng.randrange(1, R), (first + t) % nc) for t in range(count - 1)]
    rest = (value - sum(c * lag[i] for c, i in col)) % R
    i = (first + count - 1) % nc
    return col + [(rest * inv(lag[i]) % R, i)]


class Prescribed:
    """What prescribe() returns: the circuit, the values it was built to have and what they imply."""

    def __init__(self, spec, circuit, u, v, w, e):
        self.spec, self.circuit, self.u, self.v, self.w, self.e = spec, circuit, u, v, w, e
        ni = spec["ni"]
        self.lengths = dict(ic=ni, l=spec["na"], a=sum(1 for x in u if x), b_g1=sum(1 for x in v if x),
                            b_g2=sum(1 for x in v if x))
        self.unconstrained = any(x == 0 for x in e[ni:])


def prescribe(tau, toxic, spec, S=SEGMENT):
    """spec: dict(name, ni, na, nc, u, v, e); u, v, e hold one (target, way) per variable, the target
    a name of TARGETS or an integer, the way one of WAYS (e's way is that of the C column, whose
    value w = (gamma | delta) e - beta u - alpha v is solved here).  An input's u includes the term
    L_{nc+j}(tau) of the row the generator appends, so its circuit terms sum to target - L_{nc+j}; the
    way "empty" with the target None leaves such a u at its natural value.  toxic: alpha, beta,
    gamma, delta."""
    ni, na, nc = spec["ni"], spec["na"], spec["nc"]
    n = ni + na
    lag = lagrange(tau, nc + ni)
    rng = random.Random("qap " + spec["name"])
    A, B, C, u, v, w, e = [], [], [], [], [], [], []
    for j in range(n):
        (ut, uway), (vt, vway), (et, eway) = spec["u"][j], spec["v"][j], spec["e"][j]
        appended = lag[nc + j] if j < ni else 0
        uj = appended if ut is None else target(ut)
        vj, ej = target(vt), target(et)
        wj = ((toxic["gamma"] if j < ni else toxic["delta"]) * ej - toxic["beta"] * uj - toxic["alpha"] * vj) % R
        A.append(_column(rng, lag, nc, uj - appended, uway, S))
        B.append(_column(rng, lag, nc, vj, vway, S))
        C.append(_column(rng, lag, nc, wj, eway, S))
        u.append(uj); v.append(vj); w.append(wj); e.append(ej)
    return Prescribed(spec, TermCircuit(ni, na, nc, A, B, C), u, v, w, e)


def eval_columns(circuit, lag):
    """u, v, w of every variable with the oracle's eval_at_tau arithmetic, on the circuit as the
    oracle's own KeypairAssembly holds it (the appended rows included)."""
    asm = bm.KeypairAssembly()
    asm.alloc_input("", lambda: 1)
    circuit.synthesize(asm)
    for i in range(asm.num_inputs):
        asm.enforce("", lambda lc, i=i: lc + bm.Variable("input", i), lambda lc: lc, lambda lc: lc)

    def at(terms):
        acc = 0
        for c, idx in terms:
            acc = (acc + lag[idx] * c) % R
        return acc

    return tuple([at(t) for t in ins + aux] for ins, aux in ((asm.at_inputs, asm.at_aux),
                                                              (asm.bt_inputs, asm.bt_aux),
                                                              (asm.ct_inputs, asm.ct_aux)))


# ------------------------------------------------------------------ the specs
def _small(rng):
    return rng.randrange(1, 1 << SMALL_BITS)


def make_spec(name, ni, na, nc, u=None, v=None, e=None):
    """Every variable small and reached by one or two terms, but for the overrides {variable: (target,
    way)}; a negative variable counts from the end."""
    n = ni + na
    rng = random.Random("spec " + name)
    spec = dict(name=name, ni=ni, na=na, nc=nc)
    for key, over in (("u", u), ("v", v), ("e", e)):
        vals = [(_small(rng), rng.choice(("one", "two"))) for _ in range(n)]
        for j, tw in (over or {}).items():
            vals[j % n] = tw
        spec[key] = vals
    return spec


# (target, way) of a column that starts empty, and of an input's A column, where the appended row
# is already there: an input's u is 0 only by a cancellation against it
_OTHERS = [(t, "one") for t in ("1", "-2", "top", "-top", "inv", "-inv", "rand")]
_M1 = [("-1", w) for w in NONEMPTY]
COMBOS = [("0", w) for w in ("empty", "zero_coeff", "two", "segments", "long")] + _M1 + _OTHERS
COMBOS_INPUT_U = [("0", w) for w in NONEMPTY] + _M1 + _OTHERS
COMBOS_E_INPUT = [("0", w) for w in NONEMPTY] + _M1 + _OTHERS
COMBOS_E_AUX = _M1 + _OTHERS      # an aux e = 0 is an error: UNCONSTRAINED below
ROTATIONS = 16


def _rotation(k):
    """Spec k of 16: the first input (ONE), the last input, the first aux and the last aux each take
    the k-th entry, shifted per place and per vector, of the list of (target, way) that applies there;
    16 specs go through every list at every place."""
    ni, na, nc = (2, 6, 5) if k % 4 else (3, 10, 12)      # m = 8, and m = 16 for every fourth
    places = (0, ni - 1, ni, -1)
    pick = lambda combos, i: combos[i % len(combos)]
    u = {p: pick(COMBOS_INPUT_U if i < 2 else COMBOS, k + 4 * i) for i, p in enumerate(places)}
    v = {p: pick(COMBOS, k + 4 * i + 2) for i, p in enumerate(places)}
    e = {p: pick(COMBOS_E_INPUT if i < 2 else COMBOS_E_AUX, k + 4 * i + 1) for i, p in enumerate(places)}
    return make_spec(f"rot{k:02d}", ni, na, nc, u, v, e)


def _lanes260():
    """260 variables; u = (-1, 0, -1, nonzero) and v = (nonzero, -1, 0, -1) on lanes 254 .. 257, either
    side of the edge between the first and the second block of 256 lanes."""
    u = {254: ("-1", "one"), 255: ("0", "two"), 256: ("-1", "two"), 257: (3, "one")}
    v = {254: (5, "one"), 255: ("-1", "two"), 256: ("0", "empty"), 257: ("-1", "one")}
    return make_spec("lanes260", 2, 258, 6, u, v)


def _all_v_zero():
    n = 8
    return make_spec("all_v_zero", 2, 6, 5, v={j: ("0", "empty" if j % 2 else "zero_coeff") for j in range(n)},
                     u={3: ("-1", "one"), 5: ("0", "empty")})


SPECS = {s["name"]: s for s in [_rotation(k) for k in range(ROTATIONS)] + [
    # the last variable filtered / kept: the lengths read back see flag 0 and flag 1
    make_spec("last_u_zero", 2, 6, 5, u={-1: ("0", "empty")}, v={-1: ("-1", "one")}),
    make_spec("last_u_m1", 2, 6, 5, u={-1: ("-1", "two")}, v={-1: ("0", "two")}),
    # ONE filtered from a (its appended row cancelled) and from b
    make_spec("first_filtered", 2, 6, 5, u={0: ("0", "one")}, v={0: ("0", "empty")}),
    _all_v_zero(),
    make_spec("both_m1", 2, 6, 5, u={4: ("-1", "one"), 1: ("-1", "two")}, v={4: ("-1", "segments"), 1: ("-1", "one")}),
    make_spec("aux_e_m1", 2, 6, 5, e={3: ("-1", "one")}, u={3: ("rand", "one")}, v={3: ("inv", "one")}),
    make_spec("aux_e_m1_twice", 2, 6, 5, e={2: ("-1", "segments"), -1: ("-1", "two")}, u={-1: ("-top", "one")}),
    make_spec("input_e_zero", 2, 6, 5, e={0: ("0", "one"), 1: ("0", "two")}),
    make_spec("input_e_m1", 2, 6, 5, e={0: ("-1", "one"), 1: ("-1", "long")}),
    _lanes260(),
]}
# aux e = 0: the generator must refuse these ...
UNCONSTRAINED = {s["name"]: s for s in [
    make_spec("e_zero_empty", 2, 6, 5, u={4: ("0", "empty")}, v={4: ("0", "empty")}, e={4: ("0", "empty")}),
    make_spec("e_zero_cancel", 2, 6, 5, e={4: ("0", "one")}),
    make_spec("e_zero_cancel_first", 2, 6, 5, e={2: ("0", "two")}),      # the first aux: j = ni
    make_spec("e_zero_cancel_last", 2, 6, 5, e={-1: ("0", "two")}),
]}
# ... and must accept these (the old predicate refused them as well)
CONSTRAINED_M1 = ("aux_e_m1", "aux_e_m1_twice")
# u = -1, v = -1 and an aux e = -1 together, with no zero reached by cancellation: a ceremony and
# bh_params_check evaluate the columns at other points than tau, where a cancellation does not vanish
CEREMONY = {s["name"]: s for s in [
    make_spec("cer8_uv", 2, 6, 5, u={1: ("-1", "one"), -1: ("-1", "two")}, v={0: ("-1", "two"), 4: ("-1", "one")}),
    make_spec("cer8", 2, 6, 5, u={0: ("-1", "one"), 3: ("-1", "two"), 6: ("0", "empty")},
              v={1: ("-1", "one"), 3: ("-1", "segments"), 2: ("0", "zero_coeff")}, e={4: ("-1", "one")}),
    make_spec("cer16", 3, 10, 12, u={2: ("-1", "two"), -1: ("-1", "long"), 5: ("0", "zero_coeff")},
              v={0: ("-1", "two"), -1: ("0", "empty"), 7: ("-1", "one")}, e={3: ("-1", "two"), -1: ("-1", "one")}),
]}
ALL = dict(SPECS, **UNCONSTRAINED, **CEREMONY)


def toxic_of(which):
    return {"full": FULL, "fork": FORK}[which] if isinstance(which, str) else which


@functools.lru_cache(maxsize=None)
def _expected(name, which):
    toxic = toxic_of(which) if isinstance(which, str) else dict(which)
    pre = prescribe(toxic["tau"], toxic, ALL[name])
    try:
        params = bm.generate_parameters(E, pre.circuit, toxic["alpha"], toxic["beta"], toxic["gamma"],
                                        toxic["delta"], toxic["tau"])
    except bm.UnconstrainedVariable:
        return pre, None, None
    lengths = dict(ic=len(params.vk["ic"]), l=len(params.l), a=len(params.a), b_g1=len(params.b_g1),
                   b_g2=len(params.b_g2))
    return pre, bm.params_to_bytes(params), lengths


def expected(name, which="full"):
    """(Prescribed, the oracle's Parameters bytes, the oracle's vector lengths) of a spec under the
    toxic waste "full", "fork" or a dict; the bytes and lengths are None where the oracle raises
    UnconstrainedVariable.  Computed once per process."""
    return _expected(name, which if isinstance(which, str) else tuple(sorted(which.items())))
