"""The mask of bh_mpc_common_check / bh_mpc_common_verify_structure computed in Fr, with no curve
arithmetic.  A helper, not a test: test_mpc_structure_model_cpu.py pins it against masks derived by
hand, test_gpu_mpc_structure.py compares the device with it.

A storage is given by its discrete logs: a dict with the four points ("alpha_g1" ... "beta_g2") as
ints mod r and the six vectors ("tau_g1" ... "beta_mul_tau_g2") as lists of ints mod r, the point
being log * G1 or log * G2.  The pairing is non-degenerate, so e(a G1, b G2) == e(c G1, d G2) iff
a b == c d mod r: every equation of the device check is an equation between these logs, and the
model's mask is exactly the device's, not an approximation of it.

A contribution is (new, mine): `new` the logs of its results (its to_storage_format()), `mine` the
logs of the player's lists -- "alpha_g1", "alpha_g2", "beta_g1", "beta_g2" and six lists under the
vectors' names.
"""
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001

POINTS = ("alpha_g1", "alpha_g2", "beta_g1", "beta_g2")
VECTORS = ("tau_g1", "tau_g2", "alpha_mul_tau_g1", "alpha_mul_tau_g2", "beta_mul_tau_g1", "beta_mul_tau_g2")

(FIRST, ALPHA, BETA, POWERS, TAU_G2, ALPHA_TAU, ALPHA_TAU_G2, BETA_TAU, BETA_TAU_G2, LENGTHS, ALPHA_RATIO,
 BETA_RATIO, TAU_RATIO) = (1 << k for k in range(13))


def well_formed(n, tau=1, alpha=1, beta=1):
    """The logs of the well-formed storage of length n with these scalars (1, 1, 1: the initial one)."""
    p = [pow(tau, i, R) for i in range(n)]
    return {"alpha_g1": alpha % R, "alpha_g2": alpha % R, "beta_g1": beta % R, "beta_g2": beta % R,
            "tau_g1": list(p), "tau_g2": list(p),
            "alpha_mul_tau_g1": [alpha * x % R for x in p], "alpha_mul_tau_g2": [alpha * x % R for x in p],
            "beta_mul_tau_g1": [beta * x % R for x in p], "beta_mul_tau_g2": [beta * x % R for x in p]}


def contribute(old, alpha, beta, tau, factors=None):
    """(new, mine) of mpc_common_paramters_generator (mpc.rs:730-785) on the logs `old`.  factors: the
    per-element multipliers of the tau pair instead of tau^i (a player who does not use powers)."""
    n = len(old["tau_g1"])
    p = [pow(tau, i, R) for i in range(n)]
    k = {"tau": list(p) if factors is None else [f % R for f in factors],
         "alpha_mul_tau": [alpha * x % R for x in p], "beta_mul_tau": [beta * x % R for x in p]}
    new, mine = {}, {}
    for name, s in (("alpha", alpha), ("beta", beta)):
        for g in ("g1", "g2"):
            new[f"{name}_{g}"] = old[f"{name}_{g}"] * s % R
            mine[f"{name}_{g}"] = s % R
    for v in VECTORS:
        ks = k[v[:-3]]
        new[v] = [a * b % R for a, b in zip(old[v], ks)]
        mine[v] = list(ks)
    return new, mine


def _weighted(v, rho, n=None):
    n = len(v) if n is None else n
    acc, w = 0, 1
    for i in range(n):
        acc = (acc + w * v[i]) % R
        w = w * rho % R
    return acc


def check_mask(s, rho):
    """bh_mpc_common_check's mask of the storage with logs s under the weights rho^i."""
    assert 0 < rho < R
    n = len(s["tau_g1"])
    assert all(len(s[v]) == n for v in VECTORS)
    mask = 0
    if s["alpha_g1"] != s["alpha_g2"]:
        mask |= ALPHA
    if s["beta_g1"] != s["beta_g2"]:
        mask |= BETA
    if n == 0:
        return mask
    t1, t2 = s["tau_g1"], s["tau_g2"]
    if t1[0] != 1 or t2[0] != 1:
        mask |= FIRST
    if n >= 2 and _weighted([(t1[i + 1] - t2[1] * t1[i]) % R for i in range(n - 1)], rho):
        mask |= POWERS
    s_t1 = _weighted(t1, rho)
    if s_t1 != _weighted(t2, rho):
        mask |= TAU_G2
    for name, bit_tau, bit_g2 in (("alpha", ALPHA_TAU, ALPHA_TAU_G2), ("beta", BETA_TAU, BETA_TAU_G2)):
        s1 = _weighted(s[f"{name}_mul_tau_g1"], rho)
        if s1 != s_t1 * s[f"{name}_g2"] % R:
            mask |= bit_tau
        if s1 != _weighted(s[f"{name}_mul_tau_g2"], rho):
            mask |= bit_g2
    return mask


def verify_mask(old, new, mine, rho):
    """bh_mpc_common_verify_structure's mask of the contribution (new, mine) to the storage old."""
    n = len(old["tau_g1"])
    if any(len(new[v]) != n or len(mine[v]) != n for v in VECTORS):
        return LENGTHS
    mask = check_mask(new, rho)
    if new["alpha_g1"] != old["alpha_g1"] * mine["alpha_g2"] % R:
        mask |= ALPHA_RATIO
    if new["beta_g1"] != old["beta_g1"] * mine["beta_g2"] % R:
        mask |= BETA_RATIO
    if n >= 2 and new["tau_g1"][1] != old["tau_g1"][1] * mine["tau_g2"][1] % R:
        mask |= TAU_RATIO
    return mask
