"""Plain Python model of csrc/dist_h.hip: the distributed H block in integers mod r, with the
device's buffer layouts and its c' shortcut (c leaves the pipeline after the first exchange).  It
takes nothing from the library; tests/test_dist_h_model_cpu.py checks it against oracle/bellman.py.

m = 2^L = N M, C = M / N, omega of order m, w_N = omega^M, g = 7.  Rank `rank` owns the residue
class {N j + rank} before a transform and the chunks {t M + q : q = rank C + u, u < C} after it.
Buffers are flat lists indexed as the device indexes them:

  work / recv   [vec M + s C + u]   vector vec, chunk s (the peer rank), lane u
  cprime, hbuf  [t C + u]           the value for k = t M + rank C + u
  hidx          [t C + u]           k, or -1 for k = m - 1 (the coefficient create_proof drops)

stage0 is k_dist_mid and stage1 is k_dist_final; both are linear in their inputs, so feeding them
the raw device words (Montgomery residues, any representative) gives the residue of the device's
output words.  pipeline() chains phase1, the exchanges, stage0, phase3 and stage1 for every rank.
"""

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
G = 7                                   # the coset's multiplicative generator
ROOT_OF_UNITY = pow(G, (R - 1) >> 32, R)  # of order 2^32


def eligible(N, L):
    """dist_h_eligible: 2, 4, 8 or 16 ranks and a chunk of at least two elements"""
    return N in (2, 4, 8, 16) and L >= 2 * (N.bit_length() - 1) + 1


class Shape:
    def __init__(self, N, L):
        assert eligible(N, L), (N, L)
        self.N, self.L = N, L
        self.m = 1 << L
        self.M = self.m // N
        self.C = self.M // N
        self.w = pow(ROOT_OF_UNITY, 1 << (32 - L), R)
        self.wi = pow(self.w, R - 2, R)
        self.wN, self.wNi = pow(self.w, self.M, R), pow(self.wi, self.M, R)
        self.gi = pow(G, R - 2, R)
        self.minv = pow(self.m, R - 2, R)
        self.zinv = pow(pow(G, self.m, R) - 1, R - 2, R)   # 1 / Z(g), Z(x) = x^m - 1


def dft(x, root):
    """X[k] = sum_j x[j] root^(j k), root of order len(x)"""
    n = len(x)
    pw = [1] * n
    for i in range(1, n):
        pw[i] = pw[i - 1] * root % R
    return [sum(x[j] * pw[j * k % n] for j in range(n)) % R for k in range(n)]


def index_of(sh, rank, slot):
    """the global index k of slot t C + u of rank's cprime / hbuf / hidx"""
    t, u = divmod(slot, sh.C)
    return t * sh.M + rank * sh.C + u


def phase1(sh, rank, a, b, c):
    """dist_h_phase1 -> work (3 M): the inverse M-point transform (root omega^-N, no 1/M) of this
    rank's residue class of a, b and c, natural order"""
    root = pow(sh.wi, sh.N, R)
    work = []
    for v in (a, b, c):
        work += dft([v[sh.N * j + rank] for j in range(sh.M)], root)
    return work


def exchange(sh, send, nvec):
    """the all-to-all: chunk r of rank p's send buffer -> chunk p of rank r's receive buffer.
    send: one flat buffer per rank; returns one 3 M buffer per rank (vectors past nvec: None)"""
    N, M, C = sh.N, sh.M, sh.C
    recv = [[None] * (3 * M) for _ in range(N)]
    for r in range(N):
        for p in range(N):
            for v in range(nvec):
                recv[r][v * M + p * C:v * M + (p + 1) * C] = send[p][v * M + r * C:v * M + (r + 1) * C]
    return recv


def _inverse_n_dft(sh, q, col):
    """X[t] = sum_s w_N^(-s t) omega^(-q s) col[s]"""
    return dft([col[s] * pow(sh.wi, q * s, R) % R for s in range(sh.N)], sh.wNi)


def stage0(sh, rank, recv):
    """k_dist_mid: recv (3 M, [vec][source rank][C]) -> (out, cprime): the 2 M values of a's and b's
    rows in work (row d bound for rank d) and the M values of c' = ifft(c) / Z(g)"""
    N, M, C = sh.N, sh.M, sh.C
    out, cprime = [None] * (2 * M), [None] * M
    ck = sh.minv * sh.zinv % R
    for u in range(C):
        q = rank * C + u
        for vec in range(3):
            X = _inverse_n_dft(sh, q, [recv[vec * M + s * C + u] for s in range(N)])
            if vec == 2:
                for t in range(N):
                    cprime[t * C + u] = X[t] * ck % R
                continue
            S = [X[t] * pow(G, t * M + q, R) * sh.minv % R for t in range(N)]
            W = dft(S, sh.wN)
            for d in range(N):
                out[vec * M + d * C + u] = W[d] * pow(sh.w, q * d, R) % R
    return out, cprime


def phase3(sh, recv):
    """dist_h_phase3: recv's a and b rows (natural q) -> the M values of its row 0: forward M-point
    transforms (root omega^N), a b / Z(g), inverse transform (no 1/M)"""
    M = sh.M
    fa, fb = (dft(recv[v * M:(v + 1) * M], pow(sh.w, sh.N, R)) for v in (0, 1))
    return dft([x * y % R * sh.zinv % R for x, y in zip(fa, fb)], pow(sh.wi, sh.N, R))


def stage1(sh, rank, recv, cprime):
    """k_dist_final: recv (M, [source rank][C]) and cprime (M) -> (hbuf, hidx)"""
    N, M, C = sh.N, sh.M, sh.C
    hbuf, hidx = [None] * M, [None] * M
    for u in range(C):
        q = rank * C + u
        X = _inverse_n_dft(sh, q, [recv[s * C + u] for s in range(N)])
        for t in range(N):
            k = t * M + q
            hbuf[t * C + u] = (X[t] * pow(sh.gi, k, R) * sh.minv - cprime[t * C + u]) % R
            hidx[t * C + u] = -1 if k == sh.m - 1 else k
    return hbuf, hidx


def pipeline(sh, a, b, c, trace=None):
    """dist_h_run on every rank -> [(hbuf, hidx)] by rank.  trace (a dict) receives every rank's
    stage inputs and outputs: recv1, out, cprime, recv3"""
    N, M = sh.N, sh.M
    assert len(a) == len(b) == len(c) == sh.m
    recv1 = exchange(sh, [phase1(sh, r, a, b, c) for r in range(N)], 3)
    mid = [stage0(sh, r, recv1[r]) for r in range(N)]
    recv2 = exchange(sh, [o for o, _ in mid], 2)
    recv3 = exchange(sh, [phase3(sh, recv2[r]) for r in range(N)], 1)
    recv3 = [x[:M] for x in recv3]
    if trace is not None:
        trace.update(recv1=recv1, out=[o for o, _ in mid], cprime=[cp for _, cp in mid], recv3=recv3)
    return [stage1(sh, r, recv3[r], mid[r][1]) for r in range(N)]


def assemble(sh, shares):
    """[(hbuf, hidx)] by rank -> the m coefficients by global index (the -1 slot is k = m - 1)"""
    h = [None] * sh.m
    for hbuf, hidx in shares:
        for v, k in zip(hbuf, hidx):
            k = sh.m - 1 if k < 0 else k
            assert h[k] is None, k
            h[k] = v
    assert None not in h
    return h


INPUT_KINDS = ("random", "satisfied", "all_r_minus_1", "zero", "c_only", "c_zero")


def make_inputs(kind, m, rng):
    """(a, b, c), m canonical values each, of one of INPUT_KINDS (rng: a random.Random)"""
    rnd = lambda: [rng.randrange(R) for _ in range(m)]
    if kind == "random":                 # a o b != c: every coefficient of h depends on c'
        return rnd(), rnd(), rnd()
    if kind == "satisfied":
        a, b = rnd(), rnd()
        return a, b, [x * y % R for x, y in zip(a, b)]
    if kind == "all_r_minus_1":
        return [R - 1] * m, [R - 1] * m, [R - 1] * m
    if kind == "zero":
        return [0] * m, [0] * m, [0] * m
    if kind == "c_only":                 # h = -c'
        return [0] * m, [0] * m, rnd()
    if kind == "c_zero":
        return rnd(), rnd(), [0] * m
    raise ValueError(kind)


def one_hot_inputs(m, i, j, rng):
    """a one-hot at i, b random, c one-hot at j (the hot values random and non-zero)"""
    a, c = [0] * m, [0] * m
    a[i], c[j] = rng.randrange(1, R), rng.randrange(1, R)
    return a, [rng.randrange(R) for _ in range(m)], c


def ifft(x):
    """the coefficients of the polynomial with values x on the domain of size len(x) (radix 2)"""
    n = len(x)
    L = n.bit_length() - 1
    assert n == 1 << L
    wi = pow(pow(ROOT_OF_UNITY, 1 << (32 - L), R), R - 2, R) if L else 1
    a = [x[int(format(i, "0%db" % L)[::-1], 2)] if L else x[i] for i in range(n)]
    tw = [1] * max(n // 2, 1)
    for i in range(1, n // 2):
        tw[i] = tw[i - 1] * wi % R
    h = 1
    while h < n:
        step = n // (2 * h)
        for s in range(0, n, 2 * h):
            for j in range(h):
                u, t = a[s + j], a[s + j + h] * tw[j * step] % R
                a[s + j], a[s + j + h] = (u + t) % R, (u - t) % R
        h *= 2
    ninv = pow(n, R - 2, R)
    return [v * ninv % R for v in a]


def top_coefficient(a, b, c):
    """The coefficient at k = m - 1 that the pipeline leaves in the -1 slot, directly: with A, B, Cc
    the coefficient vectors of a, b, c, the coset round trip returns A B mod (x^m - g^m), whose
    coefficient m - 1 is sum_i A[i] B[m - 1 - i] (A B has no coefficient 2 m - 1), so
    h[m - 1] = (sum_i A[i] B[m - 1 - i] - Cc[m - 1]) / Z(g).  Zero when a o b = c (degree m - 2)."""
    m = len(a)
    zinv = pow(pow(G, m, R) - 1, R - 2, R)
    A, B = (None, None) if not (any(a) and any(b)) else (ifft(a), ifft(b))
    conv = sum(x * y for x, y in zip(A, reversed(B))) % R if A else 0
    # Cc[m - 1] = (1 / m) sum_j c[j] omega^(-j (m - 1)) = (1 / m) sum_j c[j] omega^j
    w = pow(ROOT_OF_UNITY, 1 << (32 - (m.bit_length() - 1)), R)
    top, p = 0, 1
    for v in c:
        top += v * p
        p = p * w % R
    return (conv - top * pow(m, R - 2, R)) * zinv % R
