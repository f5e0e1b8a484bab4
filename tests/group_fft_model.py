"""Plain Python model of csrc/group_fft.hip's index algebra, run over exponents in Z_r: a scalar
stands for the point it multiplies G by, so u + w v is (u + w * v) % r.  It takes nothing from the
library; tests/test_group_fft_model_cpu.py checks it against oracle/bellman.py.

The transform (fft_model) follows the host loop of fft_t step by step: the gather
physical q <- in[bitrev(rotl(q))], the L constant-geometry stages over the split (even | odd) array,
the twiddle index b & ~mask, which butterflies with w = 1 skip their multiplication (the first
stage's by default, every stage's prefix or none in the measurement modes), the chunks with their
four (last stage: two) output runs, and the 1/n as a last pass.  The column sum (column_sums) follows
bh_r1cs_create's segment scheme and the three summing kernels, the long columns' strided lanes and
tree included.
"""

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
R1CS_S = 32


def bitrev(i, L):
    r = 0
    for _ in range(L):
        r = (r << 1) | (i & 1)
        i >>= 1
    return r


def rotl(q, L):
    return ((q << 1) | (q >> (L - 1))) & ((1 << L) - 1)


def rotr(i, L):
    return (i >> 1) | ((i & 1) << (L - 1))


def gather_source(q, L):
    """k_gfft_gather: the input index physical slot q is loaded from"""
    return bitrev(rotl(q, L), L)


def twiddle_index(stage, b, L):
    """k_gfft_twiddles: the exponent e of w = omega^e for butterfly b of a stage"""
    mask = (1 << (L - 1 - stage)) - 1
    return b & ~mask


def stage_ranges(stage, L, chunk, w1="first"):
    """(mul, b0, k) for every butterfly launch of a stage, in the host's order.  w1: "first" (the
    default), "prefix" or "none" (BH_GROUP_FFT_W1)"""
    half = 1 << (L - 1)
    n1 = (1 << (L - 1 - stage)) if w1 == "prefix" else half if (w1 == "first" and stage == 0) else 0
    out = []
    for mul, lo, hi in ((0, 0, n1), (1, n1, half)):
        b0 = lo
        while b0 < hi:
            k = min(chunk, hi - b0)
            out.append((mul, b0, k))
            b0 += k
    return out


def fft_model(x, omega, inverse=False, scale=True, chunk=1 << 18, w1="first", stats=None):
    """The transform of x (len 2^L >= 2) over exponents.  stats (a dict) receives the number of
    multiplications by a twiddle, of butterflies that skipped theirs, and of multiplications by one."""
    n = len(x)
    L = n.bit_length() - 1
    assert n == 1 << L and L >= 1
    half = n // 2
    chunk = min(half, chunk)
    w0 = pow(omega, R - 2, R) if inverse else omega
    tw = [pow(w0, e, R) for e in range(half)]
    cur = [x[gather_source(q, L)] for q in range(n)]
    muls = skipped = ones = 0
    for stage in range(L):
        last = stage == L - 1
        nxt = [None] * n
        for mul, b0, k in stage_ranges(stage, L, chunk, w1):
            assert last or (k % 2 == 0 and b0 % 2 == 0)
            slots = [None] * (2 * k)
            for l in range(k):
                b = b0 + l
                u, v = cur[b], cur[half + b]
                e = twiddle_index(stage, b, L)
                if mul:
                    t = tw[e] * v % R
                    muls += 1
                    ones += e == 0
                else:
                    assert e == 0
                    t = v
                    skipped += 1
                lo = l if last else (l & 1) * k + (l >> 1)
                slots[lo] = (u + t) % R
                slots[lo + (k if last else k // 2)] = (u - t) % R
            if last:
                nxt[b0:b0 + k] = slots[:k]
                nxt[half + b0:half + b0 + k] = slots[k:]
            else:
                for q in range(4):
                    d = (q >> 1) * half + (q & 1) * (half // 2) + b0 // 2
                    nxt[d:d + k // 2] = slots[q * (k // 2):(q + 1) * (k // 2)]
        assert None not in nxt
        cur = nxt
    if inverse and scale:
        ninv = pow(n, R - 2, R)
        cur = [v * ninv % R for v in cur]
    if stats is not None:
        stats["muls"], stats["skipped"], stats["muls_by_one"] = muls, skipped, ones
    return cur


# ------------------------------------------------------------------ the column sum
def segment_scheme(columns):
    """bh_r1cs_create's layout of a list of columns (each a list of (coeff, row)): coeff, row, seg,
    colseg, longcols"""
    coeff, row, seg, colseg, longcols = [], [], [], [], []
    for j, col in enumerate(columns):
        t0 = len(coeff)
        for c, i in col:
            coeff.append(c % R)
            row.append(i)
        colseg.append(len(seg))
        seg.extend(range(t0, len(coeff), R1CS_S))
        if len(seg) - colseg[j] > R1CS_S:
            longcols.append(j)
    colseg.append(len(seg))
    seg.append(len(coeff))
    return coeff, row, seg, colseg, longcols


def column_sums(columns, lag, m, chunk=1 << 18):
    """sum over column j of (coeff / m) * (m * lag)[row]: the unscaled transform's Lagrange values
    times coefficients that carry the 1/m, summed by segments (in chunks of whole segments), columns
    and long columns as k_gfft_seg_sum / _col_sum / _col_long do"""
    coeff, row, seg, colseg, longcols = segment_scheme(columns)
    minv = pow(m, R - 2, R)
    sc = [c * minv % R for c in coeff]
    unscaled = [v * m % R for v in lag]
    nseg = len(seg) - 1
    part = [None] * nseg
    k0 = 0
    while k0 < nseg:
        k1, tbase = k0, seg[k0]
        while k1 < nseg and seg[k1 + 1] - tbase <= chunk:
            k1 += 1
        assert k1 > k0
        prod = [sc[t] * unscaled[row[t]] % R for t in range(tbase, seg[k1])]
        for k in range(k0, k1):
            part[k] = sum(prod[t - tbase] for t in range(seg[k], seg[k + 1])) % R
        k0 = k1
    y = [None] * len(columns)
    for j in range(len(columns)):
        p0, p1 = colseg[j], colseg[j + 1]
        if p1 - p0 > R1CS_S:
            continue
        y[j] = sum(part[p0:p1]) % R
    for j in longcols:
        p0, p1 = colseg[j], colseg[j + 1]
        acc = [sum(part[p] for p in range(p0 + lane, p1, 64)) % R for lane in range(64)]
        off = 32
        while off:
            for lane in range(off):
                acc[lane] = (acc[lane] + acc[lane + off]) % R
            off >>= 1
        y[j] = acc[0]
    assert None not in y
    return y
