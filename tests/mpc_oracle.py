"""Python restatement of the ceremony functions of the reference's groth16/mpc.rs that the device
rounds replace, over oracle.bls12_381 and oracle.pairing.  A helper, not a test: test_mpc_oracle_cpu.py
pins it against the constants the reference asserts, test_gpu_mpc.py compares the device with it.

Points are affine tuples as in oracle.bls12_381 (None = identity); scalars are ints, multiplied mod r
where the reference multiplies in u64 (the two agree while the reference's product does not overflow).
"""
from oracle import bls12_381 as bls
from oracle import pairing as pr

G1, G2, R = bls.G1, bls.G2, bls.R
GEN1, GEN2 = G1.gen_affine, G2.gen_affine


def mul(C, a, k):
    return C.to_affine(C.mul(C.from_affine(a), k % R))


def sub(C, a, b):
    return C.to_affine(C.add(C.from_affine(a), C.neg(C.from_affine(b))))


def g1(k):
    return mul(G1, GEN1, k)


def g2(k):
    return mul(G2, GEN2, k)


def g1_bytes(a):
    return bls.g1_to_uncompressed(a)


def g2_bytes(a):
    return bls.g2_to_uncompressed(a)


class ParameterPair:  # mpc.rs:16-29
    def __init__(self, g1_result, g2_result, g1_mine, g2_mine):
        self.g1_result, self.g2_result, self.g1_mine, self.g2_mine = g1_result, g2_result, g1_mine, g2_mine

    def bytes(self):
        return g1_bytes(self.g1_result) + g2_bytes(self.g2_result) + g1_bytes(self.g1_mine) + g2_bytes(self.g2_mine)


def make_new_paramter(x, pointg1, pointg2, inverse=False):  # mpc.rs:647-675
    k = pow(x, -1, R) if inverse else x % R
    return ParameterPair(mul(G1, pointg1, k), mul(G2, pointg2, k), g1(k), g2(k))


def make_new_tau_paramter(a, x, list_g1, list_g2, invert=False):  # mpc.rs:677-706
    assert len(list_g1) == len(list_g2)
    return [make_new_paramter(pow(x, i, R) * a % R, list_g1[i], list_g2[i], invert) for i in range(len(list_g1))]


class Storage:
    """CommonParamterInStorage (mpc.rs:398-414) / UnCommonParamterInStorage (mpc.rs:926-942): `points`
    and `vectors` in declaration order, by name."""

    def __init__(self, points, vectors):
        self.points, self.vectors = dict(points), dict(vectors)

    def __getattr__(self, name):
        for d in (self.__dict__["points"], self.__dict__["vectors"]):
            if name in d:
                return d[name]
        raise AttributeError(name)


COMMON_POINTS = ("alpha_g1", "alpha_g2", "beta_g1", "beta_g2")
COMMON_VECTORS = ("tau_g1", "tau_g2", "alpha_mul_tau_g1", "alpha_mul_tau_g2", "beta_mul_tau_g1", "beta_mul_tau_g2")
UNCOMMON_POINTS = ("gamma_g1", "gamma_g2", "delta_g1", "delta_g2")
UNCOMMON_VECTORS = ("kin_g1", "kin_g2", "kout_g1", "kout_g2", "h_g1", "h_g2")


def _u32(n):
    return int(n).to_bytes(4, "big")


def _pt_bytes(name, a):
    return g1_bytes(a) if name.endswith("g1") else g2_bytes(a)


def common_storage_bytes(s):
    """The library's bytes of a CommonParamterInStorage: u32-BE len, the fields in order."""
    out = _u32(len(s.tau_g1))
    out += b"".join(_pt_bytes(n, s.points[n]) for n in COMMON_POINTS)
    out += b"".join(_pt_bytes(n, a) for n in COMMON_VECTORS for a in s.vectors[n])
    return out


def uncommon_storage_bytes(s):
    out = b"".join(_pt_bytes(n, s.points[n]) for n in UNCOMMON_POINTS)
    for n in UNCOMMON_VECTORS:
        out += _u32(len(s.vectors[n])) + b"".join(_pt_bytes(n, a) for a in s.vectors[n])
    return out


class CommonParamter:  # mpc.rs:362-373
    def __init__(self, alpha, beta, tau, alpha_mul_tau, beta_mul_tau):
        self.alpha, self.beta, self.tau, self.alpha_mul_tau, self.beta_mul_tau = alpha, beta, tau, alpha_mul_tau, beta_mul_tau

    def to_storage_format(self):  # mpc.rs:381-394
        return Storage(
            {"alpha_g1": self.alpha.g1_result, "alpha_g2": self.alpha.g2_result,
             "beta_g1": self.beta.g1_result, "beta_g2": self.beta.g2_result},
            {"tau_g1": [p.g1_result for p in self.tau], "tau_g2": [p.g2_result for p in self.tau],
             "alpha_mul_tau_g1": [p.g1_result for p in self.alpha_mul_tau],
             "alpha_mul_tau_g2": [p.g2_result for p in self.alpha_mul_tau],
             "beta_mul_tau_g1": [p.g1_result for p in self.beta_mul_tau],
             "beta_mul_tau_g2": [p.g2_result for p in self.beta_mul_tau]})

    def bytes(self):
        out = self.alpha.bytes() + self.beta.bytes()
        for lst in (self.tau, self.alpha_mul_tau, self.beta_mul_tau):
            out += _u32(len(lst)) + b"".join(p.bytes() for p in lst)
        return out


def initial_common_paramters(length):  # mpc.rs:708-728
    return Storage({n: (GEN1 if n.endswith("g1") else GEN2) for n in COMMON_POINTS},
                   {n: [GEN1 if n.endswith("g1") else GEN2] * length for n in COMMON_VECTORS})


def mpc_common_paramters_generator(storage, alpha_beta_tau):  # mpc.rs:730-785
    alpha, beta, tau = alpha_beta_tau
    return CommonParamter(
        make_new_paramter(alpha, storage.alpha_g1, storage.alpha_g2),
        make_new_paramter(beta, storage.beta_g1, storage.beta_g2),
        make_new_tau_paramter(1, tau, storage.tau_g1, storage.tau_g2),
        make_new_tau_paramter(alpha, tau, storage.alpha_mul_tau_g1, storage.alpha_mul_tau_g2),
        make_new_tau_paramter(beta, tau, storage.beta_mul_tau_g1, storage.beta_mul_tau_g2))


def _pairing_eq(p1, q1, p2, q2):
    """e(p1, q1) == e(p2, q2), as one product with one final exponentiation."""
    return pr.pairing_product_is_one([(p1, q1), (G1.to_affine(G1.neg(G1.from_affine(p2))), q2)])


def verify_new_paramter(paramter, baseg1, baseg2=None):  # mpc.rs:787-804
    return (_pairing_eq(paramter.g1_result, GEN2, baseg1, paramter.g2_mine)
            and _pairing_eq(paramter.g1_result, GEN2, GEN1, paramter.g2_result))


def verify_common_paramter(storage, new_paramter, pairings=True):
    """mpc.rs:806-862: the next storage, or None where the reference's assert fails.  pairings=False
    keeps only the length check (each pairing takes most of a second here)."""
    n = len(new_paramter.tau)
    ok = n == len(new_paramter.alpha_mul_tau) == len(new_paramter.beta_mul_tau)
    if ok and pairings:
        ok = (verify_new_paramter(new_paramter.alpha, storage.alpha_g1)
              and verify_new_paramter(new_paramter.beta, storage.beta_g1))
        for i in range(n):  # the tau list itself is not checked (commented out, mpc.rs:831-840)
            ok = ok and verify_new_paramter(new_paramter.alpha_mul_tau[i], storage.alpha_mul_tau_g1[i])
            ok = ok and verify_new_paramter(new_paramter.beta_mul_tau[i], storage.beta_mul_tau_g1[i])
    return new_paramter.to_storage_format() if ok else None


def h_basis(storage, n):  # the matrixed_h part of matrix, mpc.rs:631-635
    assert 2 * n <= len(storage.tau_g1)
    return ([sub(G1, storage.tau_g1[n + i], storage.tau_g1[i]) for i in range(n)],
            [sub(G2, storage.tau_g2[n + i], storage.tau_g2[i]) for i in range(n)])


class UnCommonParamter:  # mpc.rs:891-902
    def __init__(self, delta, gamma, ic, l, h):
        self.delta, self.gamma, self.ic, self.l, self.h = delta, gamma, ic, l, h

    def to_storage_format(self):  # mpc.rs:910-923
        return Storage(
            {"gamma_g1": self.gamma.g1_result, "gamma_g2": self.gamma.g2_result,
             "delta_g1": self.delta.g1_result, "delta_g2": self.delta.g2_result},
            {"kin_g1": [p.g1_result for p in self.ic], "kin_g2": [p.g2_result for p in self.ic],
             "kout_g1": [p.g1_result for p in self.l], "kout_g2": [p.g2_result for p in self.l],
             "h_g1": [p.g1_result for p in self.h], "h_g2": [p.g2_result for p in self.h]})

    def bytes(self):
        out = self.delta.bytes() + self.gamma.bytes()
        for lst in (self.ic, self.l, self.h):
            out += _u32(len(lst)) + b"".join(p.bytes() for p in lst)
        return out


def initial_uncommon_paramters(matrix):
    """mpc.rs:993-1015; matrix: CommonParamterMatrix as a dict front_g1, front_g2, back_g1, back_g2,
    h_g1, h_g2."""
    return Storage({n: (GEN1 if n.endswith("g1") else GEN2) for n in UNCOMMON_POINTS},
                   {"kin_g1": list(matrix["front_g1"]), "kin_g2": list(matrix["front_g2"]),
                    "kout_g1": list(matrix["back_g1"]), "kout_g2": list(matrix["back_g2"]),
                    "h_g1": list(matrix["h_g1"]), "h_g2": list(matrix["h_g2"])})


def mpc_uncommon_paramters_generator(storage, gamma_delta):  # mpc.rs:1017-1063
    gamma, delta = gamma_delta
    return UnCommonParamter(
        make_new_paramter(delta, storage.delta_g1, storage.delta_g2),
        make_new_paramter(gamma, storage.gamma_g1, storage.gamma_g2),
        make_new_tau_paramter(gamma, 1, storage.kin_g1, storage.kin_g2, True),
        make_new_tau_paramter(delta, 1, storage.kout_g1, storage.kout_g2, True),
        make_new_tau_paramter(delta, 1, storage.h_g1, storage.h_g2, True))


def verify_uncommon_paramter(matrix, storage, new_paramter, pairings=True):  # mpc.rs:1065-1131
    ok = (len(new_paramter.ic) >= len(storage.kin_g1) and len(new_paramter.l) >= len(storage.kout_g1)
          and len(new_paramter.h) >= len(storage.h_g1))  # where the reference's indexing would panic
    if ok and pairings:
        ok = (verify_new_paramter(new_paramter.delta, storage.delta_g1)
              and verify_new_paramter(new_paramter.gamma, storage.gamma_g1))
        for lst, key, pair, old in ((new_paramter.ic, "front_g1", new_paramter.gamma, storage.kin_g1),
                                    (new_paramter.l, "back_g1", new_paramter.delta, storage.kout_g1),
                                    (new_paramter.h, "h_g1", new_paramter.delta, storage.h_g1)):
            for i in range(len(old)):
                ok = ok and _pairing_eq(lst[i].g1_result, pair.g2_result, matrix[key][i], GEN2)
    return new_paramter.to_storage_format() if ok else None
