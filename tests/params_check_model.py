"""The mask of bh_params_check computed in Fr, with no curve arithmetic.  A
helper, not a test: test_params_check_model_cpu.py pins it against masks derived by hand and against
the generator, test_gpu_params_check.py compares the device with it.

Points are given by their discrete logs mod r, as in mpc_structure_model.py: e(a G1, b G2) ==
e(c G1, d G2) iff a b == c d mod r, so every equation of the device check is an equation between
logs and the model's mask is exactly the device's.

A circuit is a KeypairAssembly-shaped object (num_inputs, num_aux, num_constraints and the six
column lists at_inputs .. ct_aux of (coeff, row) terms; oracle/bellman.py's or bellman_hip's).  A
storage is mpc_structure_model's dict of logs.  Parameters are a dict of logs: the points alpha_g1,
beta_g1, beta_g2, gamma_g2, delta_g1, delta_g2 and the lists ic, h, l, a, b_g1, b_g2.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import bellman as bm  # noqa: E402

R = bm.BLS12_381.Fr.q

(SIZES, ALPHA, BETA, DELTA, A, B_G1, B_G2, L, IC, H) = (1 << k for k in range(10))

POINTS = ("alpha_g1", "beta_g1", "beta_g2", "gamma_g2", "delta_g1", "delta_g2")
LISTS = ("ic", "h", "l", "a", "b_g1", "b_g2")


def domain_size(asm):
    m = 1
    while m < asm.num_constraints + asm.num_inputs:
        m *= 2
    return m


def columns(asm):
    """A, B, C over the variables [inputs, aux] as lists of (coeff, row); A with the appended rows
    input_i * 0 = 0 (generator.rs:276-282), row num_constraints + i."""
    a = [list(c) for c in asm.at_inputs] + [list(c) for c in asm.at_aux]
    for i in range(asm.num_inputs):
        a[i].append((1, asm.num_constraints + i))
    b = [list(c) for c in asm.bt_inputs] + [list(c) for c in asm.bt_aux]
    c = [list(c) for c in asm.ct_inputs] + [list(c) for c in asm.ct_aux]
    return a, b, c


def eval_columns(cols, x):
    """bh_r1cs_eval of one matrix: sum over a column's terms of coeff * x[row]."""
    return [sum(c * x[row] for c, row in col) % R for col in cols]


def ifft(values):
    dom = bm.EvaluationDomain(bm.BLS12_381, list(values))
    assert len(dom.coeffs) == len(values)
    dom.ifft()
    return dom.coeffs


def lagrange(m, tau):
    """L_k(tau), k < m: the inverse transform of the powers (generator.rs:400-401)."""
    return ifft([pow(tau, i, R) for i in range(m)])


def coefficients(cols, z, m):
    """c_M(z): the inverse NTT of the row vector M z (bh_r1cs_witness's a, b or c for z)."""
    rows = [0] * m
    for zj, col in zip(z, cols):
        for c, row in col:
            rows[row] = (rows[row] + c * zj) % R
    return ifft(rows)


def generator_logs(asm, alpha, beta, gamma, delta, tau):
    """The logs of bh_generate_parameters' output (generator.rs:349-397, 411-572, 614-633)."""
    m = domain_size(asm)
    ni = asm.num_inputs
    a, b, c = columns(asm)
    lag = lagrange(m, tau)
    u, v, w = (eval_columns(x, lag) for x in (a, b, c))
    gi, di = pow(gamma, -1, R), pow(delta, -1, R)
    ext = [(beta * uj + alpha * vj + wj) % R for uj, vj, wj in zip(u, v, w)]
    zt = (pow(tau, m, R) - 1) * di % R
    return {"alpha_g1": alpha % R, "beta_g1": beta % R, "beta_g2": beta % R, "gamma_g2": gamma % R,
            "delta_g1": delta % R, "delta_g2": delta % R,
            "ic": [e * gi % R for e in ext[:ni]], "l": [e * di % R for e in ext[ni:]],
            "h": [pow(tau, i, R) * zt % R for i in range(m - 1)],
            "a": [x for x in u if x], "b_g1": [x for x in v if x], "b_g2": [x for x in v if x]}


def _dot(xs, ys):
    assert len(xs) == len(ys)
    return sum(x * y for x, y in zip(xs, ys)) % R


def check_mask(asm, s, p, rho, sigma, weights=None):
    """bh_params_check's mask of the Parameters logs p against the circuit asm and the storage logs
    s.  weights: the n variable weights instead of rho^j (to show what other weights would miss)."""
    assert 0 < rho < R and 0 < sigma < R
    m = domain_size(asm)
    ni, n = asm.num_inputs, asm.num_inputs + asm.num_aux
    assert m >= 2 and len(s["tau_g1"]) >= 2 * m
    a, b, c = columns(asm)
    x = [pow(sigma, i, R) for i in range(m)]
    fu = [uj != 0 for uj in eval_columns(a, x)]
    fv = [vj != 0 for vj in eval_columns(b, x)]
    if (len(p["ic"]) != ni or len(p["l"]) != n - ni or len(p["h"]) != m - 1 or len(p["a"]) != sum(fu)
            or len(p["b_g1"]) != sum(fv) or len(p["b_g2"]) != sum(fv)):
        return SIZES
    w = [pow(rho, j, R) for j in range(n)] if weights is None else [x % R for x in weights]
    w_in = w[:ni] + [0] * (n - ni)
    w_aux = [0] * ni + w[ni:]
    w_a = [wj for wj, f in zip(w, fu) if f]
    w_b = [wj for wj, f in zip(w, fv) if f]
    t, t2 = s["tau_g1"][:m], s["tau_g2"][:m]
    at, bt = s["alpha_mul_tau_g1"][:m], s["beta_mul_tau_g1"][:m]

    def k_of(z):
        return (_dot(bt, coefficients(a, z, m)) + _dot(at, coefficients(b, z, m)) + _dot(t, coefficients(c, z, m))) % R

    mask = 0
    if p["alpha_g1"] != s["alpha_g1"]:
        mask |= ALPHA
    if p["beta_g1"] != s["beta_g1"] or p["beta_g2"] != s["beta_g2"]:
        mask |= BETA
    if p["delta_g1"] != p["delta_g2"] or p["gamma_g2"] == 0 or p["delta_g2"] == 0:
        mask |= DELTA
    c_a, c_b = coefficients(a, w, m), coefficients(b, w, m)
    if _dot(p["a"], w_a) != _dot(t, c_a):
        mask |= A
    if _dot(p["b_g1"], w_b) != _dot(t, c_b):
        mask |= B_G1
    if _dot(p["b_g2"], w_b) != _dot(t2, c_b):
        mask |= B_G2
    if _dot(p["l"], w[ni:]) * p["delta_g2"] % R != k_of(w_aux):
        mask |= L
    if _dot(p["ic"], w[:ni]) * p["gamma_g2"] % R != k_of(w_in):
        mask |= IC
    pw = [pow(rho, i, R) for i in range(m - 1)]
    full = s["tau_g1"]
    if _dot(p["h"], pw) * p["delta_g2"] % R != _dot([(full[i + m] - full[i]) % R for i in range(m - 1)], pw):
        mask |= H
    return mask
