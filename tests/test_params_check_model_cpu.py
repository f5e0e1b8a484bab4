"""tests/params_check_model.py against the identity bh_params_check rests on, against the generator's
own output and against masks derived by hand from the equations.  Integers
mod r only."""
import os
import random
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mpc_structure_model as sm  # noqa: E402
import params_check_model as pm  # noqa: E402
from oracle import bellman as bm  # noqa: E402

R = pm.R
TOXIC = dict(alpha=0x6F0E1D2C3B4A59687786A5B4C3D2E1F00112233445566778899AABBCCDDEEFF1 % R,
             beta=0x1234567890ABCDEF1122334455667788,
             gamma=0x3C4D5E6F708192A3B4C5D6E7F8091A2B3C4D5E6F708192A3B4C5D6E7F8091A2B % R,
             delta=0x0F1E2D3C4B5A69788796A5B4C3D2E1F0FEDCBA98765432100123456789ABCDEF % R,
             tau=0x5AB3F1C2D4E6978877665544332211FFEEDDCCBBAA99887766554433221100FF % R)
RHO = 0x2B7E151628AED2A6ABF7158809CF4F3C762E7160F38B4DA56A784D9045190CFE % R
SIGMA = 0x243F6A8885A308D313198A2E03707344A4093822299F31D0082EFA98EC4E6C89 % R


def _circuit(seed=19):
    """6 constraints and 2 inputs (m = 8).  aux 0: a duplicate (variable, row) pair in A; aux 1: c and
    r - c on one row of A (a column that has terms and is absent); aux 2: an empty B column."""
    rng = random.Random(seed)
    k = lambda: rng.randrange(1, R)
    asm = bm.KeypairAssembly()
    asm.alloc_input("", None)
    asm.alloc_input("", None)
    for _ in range(5):
        asm.alloc("", None)
    asm.num_constraints = 6
    asm.at_aux[0] = [(k(), 0), (k(), 0), (k(), 3)]
    asm.bt_aux[0] = [(k(), 1)]
    c = k()
    asm.at_aux[1] = [(c, 2), (R - c, 2)]
    asm.bt_aux[1] = [(k(), 2), (k(), 5)]
    asm.at_aux[2] = [(k(), 4)]
    asm.ct_aux[2] = [(k(), 4)]
    asm.bt_aux[3] = [(k(), 0), (k(), 3)]
    asm.ct_aux[3] = [(k(), 1)]
    for t in (asm.at_aux, asm.bt_aux, asm.ct_aux):
        t[4] = [(k(), rng.randrange(6)) for _ in range(4)]
    asm.bt_inputs[0] = [(1, i) for i in range(6)]
    asm.ct_inputs[1] = [(k(), 0), (k(), 5)]
    return asm


ASM = _circuit()
M = pm.domain_size(ASM)
N = ASM.num_inputs + ASM.num_aux


def _storage(**kw):
    t = dict(TOXIC, **kw)
    return sm.well_formed(2 * M, t["tau"], t["alpha"], t["beta"])


def _params(**kw):
    return pm.generator_logs(ASM, **dict(TOXIC, **kw))


STORAGE = _storage()


def _mask(p, asm=ASM, rho=RHO, sigma=SIGMA, **kw):
    return pm.check_mask(asm, STORAGE, p, rho, sigma, **kw)


def test_sizes_of_the_circuit():
    assert M == 8 and N == 7
    p = _params()
    # inputs 0, 1 (the appended rows), aux 0, 2, 4 in A; input 0, aux 0, 1, 3, 4 in B
    assert (len(p["a"]), len(p["b_g1"]), len(p["b_g2"]), len(p["l"]), len(p["ic"]), len(p["h"])) == (5, 5, 5, 5, 2, 7)


# ------------------------------------------------------------------ 1. the identity behind the check
@pytest.mark.parametrize("which", [0, 1, 2])
def test_coefficients_evaluate_to_the_weighted_columns(which):
    """sum_k c_M(w)_k tau^k == sum_j w_j M_j(tau): the inverse NTT of M w is the polynomial
    sum_j w_j M_j(X), with duplicates, a cancelling and an empty column."""
    cols = pm.columns(ASM)[which]
    tau = TOXIC["tau"]
    w = [pow(RHO, j, R) for j in range(N)]
    coef = pm.coefficients(cols, w, M)
    lhs = sum(c * pow(tau, k, R) for k, c in enumerate(coef)) % R
    at_tau = pm.eval_columns(cols, pm.lagrange(M, tau))
    assert lhs == sum(wj * x for wj, x in zip(w, at_tau)) % R
    if which == 0:
        assert at_tau[ASM.num_inputs + 1] == 0 and len(cols[ASM.num_inputs + 1]) == 2  # the cancelling column
    if which == 1:
        assert at_tau[ASM.num_inputs + 2] == 0 and not cols[ASM.num_inputs + 2]  # the empty one


def test_presence_does_not_depend_on_sigma():
    """... except on the roots of a column's polynomial sum coeff X^row, fewer than m per column: input
    0's B column is 1 + X + ... + X^5, which sigma = -1 annuls (the m / r term of the soundness bound)."""
    a, b, _ = pm.columns(ASM)
    assert pm.eval_columns(b, [pow(R - 1, i, R) for i in range(M)])[0] == 0
    want = None
    for sigma in (SIGMA, RHO, 2, 3):
        x = [pow(sigma, i, R) for i in range(M)]
        got = ([u != 0 for u in pm.eval_columns(a, x)], [v != 0 for v in pm.eval_columns(b, x)])
        want = want or got
        assert got == want
    assert want[0] == [True, True, True, False, True, False, True]
    assert want[1] == [True, False, True, True, False, True, True]


# ------------------------------------------------------------------ 2. valid Parameters pass
@pytest.mark.parametrize("seed", range(4))
def test_generator_output_passes_for_any_gamma_delta(seed):
    rng = random.Random(seed)
    p = _params(gamma=rng.randrange(1, R), delta=rng.randrange(1, R))
    assert _mask(p, rho=rng.randrange(1, R), sigma=rng.randrange(1, R)) == 0


# ------------------------------------------------------------------ 3. each mutation, its mask
def _swapped(p, name, i, j):
    q = {k: (list(v) if isinstance(v, list) else v) for k, v in p.items()}
    q[name][i], q[name][j] = q[name][j], q[name][i]
    return q


def _with(p, **kw):
    return dict(p, **kw)


MUTATIONS = [
    ("a[0] <-> a[1]", lambda p: _swapped(p, "a", 0, 1), pm.A),
    ("a[last-1] <-> a[last]", lambda p: _swapped(p, "a", -2, -1), pm.A),
    ("b_g2 swapped, b_g1 left alone", lambda p: _swapped(p, "b_g2", 1, 3), pm.B_G2),
    ("b_g1 swapped, b_g2 left alone", lambda p: _swapped(p, "b_g1", 0, 4), pm.B_G1),
    ("two l elements swapped", lambda p: _swapped(p, "l", 0, 3), pm.L),
    ("two h elements swapped", lambda p: _swapped(p, "h", 2, 6), pm.H),
    ("two ic elements swapped", lambda p: _swapped(p, "ic", 0, 1), pm.IC),
    ("another tau", lambda p: _params(tau=TOXIC["tau"] + 1), pm.A | pm.B_G1 | pm.B_G2 | pm.H | pm.L | pm.IC),
    ("another alpha", lambda p: _params(alpha=TOXIC["alpha"] + 1), pm.ALPHA | pm.L | pm.IC),
    ("another beta", lambda p: _params(beta=TOXIC["beta"] + 1), pm.BETA | pm.L | pm.IC),
    ("delta_g1 of another delta", lambda p: _with(p, delta_g1=p["delta_g1"] + 1), pm.DELTA),
    ("gamma_g2 the identity", lambda p: _with(p, gamma_g2=0), pm.DELTA | pm.IC),
    ("l_0 + P, l_1 - P", lambda p: _with(p, l=[p["l"][0] + 5, p["l"][1] - 5] + p["l"][2:]), pm.L),
    ("one element dropped from l", lambda p: _with(p, l=p["l"][1:]), pm.SIZES),
    ("one element dropped from a", lambda p: _with(p, a=p["a"][:-1]), pm.SIZES),
    ("h one longer", lambda p: _with(p, h=p["h"] + [1]), pm.SIZES),
]


@pytest.mark.parametrize("name,mutate,want", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_mutation_masks(name, mutate, want):
    p = _params()
    assert _mask(p) == 0
    q = mutate(p)
    for k in pm.POINTS:
        q[k] %= R
    for k in pm.LISTS:
        q[k] = [x % R for x in q[k]]
    assert _mask(q) == want


def test_another_circuit_of_the_same_sizes():
    other = _circuit(seed=20)
    p = pm.generator_logs(other, **TOXIC)
    assert [len(p[k]) for k in pm.LISTS] == [len(_params()[k]) for k in pm.LISTS]
    mask = _mask(p)
    assert mask and not mask & pm.SIZES
    assert pm.check_mask(other, STORAGE, p, RHO, SIGMA) == 0


# ------------------------------------------------------------------ 4. why the weights are powers
def test_opposite_errors_cancel_under_equal_weights_only():
    p = _params()
    q = _with(p, l=[(p["l"][0] + 5) % R, (p["l"][1] - 5) % R] + p["l"][2:])
    assert _mask(q, weights=[1] * N) == 0
    assert _mask(q) == pm.L
    for rho in (2, RHO + 1, R - 1):
        assert _mask(q, rho=rho) == pm.L
