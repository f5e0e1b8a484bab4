#!/usr/bin/env python3
"""Timings of the Gt vectors: pairings per second and exponentiations per
second on the device, against what the library offered per value before bh_gt_*.

For each 2^log_len, on the vectors a x^i G1 and a x^i G2 (bh_srs_mul_powers of the generators), in
one process, medians of --reps runs after one warm-up:

  * bh_gt_pairing                       pairings per second
  * bh_gt_mul_each, one scalar each     exponentiations per second (seeded random scalars below r)
  * bh_gt_mul_each, one shared scalar   the same with every branch wave-uniform
  * bh_gt_upload(checked=1)             membership tests per second (a shared-exponent power each)

and, on --baseline-len pairs, the per-value path without them: bh_miller_product on one pair, then
bh_final_exponentiation on the host (the value in the library's own convention, not the crate's).

Every call ends in a synchronise, so host wall time is the device time plus the call's host work,
copies and allocations.
usage: time_gt.py [--log-len 10 14 16] [--baseline-len 16] [--reps 5]"""
import argparse
import ctypes
import json
import os
import random
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bellman-mpc_amd"))
sys.path.insert(0, ROOT)


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, (time.perf_counter() - t0) * 1e3


def measure(reps, fn):
    """one warm-up, then reps runs: [ms]"""
    return [timed(fn)[1] for _ in range(reps + 1)][1:]


def summary(runs, n):
    med = statistics.median(runs)
    return {"ms": [round(v, 2) for v in runs], "median_ms": round(med, 2),
            "spread_ms": round(max(runs) - min(runs), 2), "per_second": round(n / med * 1e3, 1)}


def ptr(arr):
    return arr.ctypes.data_as(ctypes.c_void_p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-len", type=int, nargs="+", default=[10, 14, 16])
    ap.add_argument("--baseline-len", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import bellman_hip as bh
    lib = bh.lib()
    ctx = bh.Context(0)
    a, x = 0x1F2E3D4C5B6A79881122334455667788, 0x0123456789ABCDEFFEDCBA9876543210AABBCCDD
    rng = random.Random(18)

    def vectors(n):
        gens = bh.initial_common_paramters(ctx, n)
        return gens.vector(0).mul_powers(a, x), gens.vector(1).mul_powers(a, x)

    for log_len in args.log_len:
        n = 1 << log_len
        g1, g2 = vectors(n)
        rec = {"len": n}
        made = []

        def pairing():
            h = ctypes.c_void_p()
            code = lib.bh_gt_pairing(ctx.h, g1.h, 0, g2.h, 0, n, ctypes.byref(h))
            assert code == 0, code
            made.append(h)

        rec["pairing"] = summary(measure(args.reps, pairing), n)
        gt = made[-1]
        for h in made[:-1]:
            lib.bh_gt_free(h)
        del made[:]
        words = np.ascontiguousarray(np.stack([bh.fr_canonical_words(rng.randrange(bh.R_MODULUS)) for _ in range(n)]))

        def mul_each(count):
            h = ctypes.c_void_p()
            code = lib.bh_gt_mul_each(ctx.h, gt, ptr(words), count, ctypes.byref(h))
            assert code == 0, code
            lib.bh_gt_free(h)

        rec["mul_each"] = summary(measure(args.reps, lambda: mul_each(n)), n)
        rec["mul_each_shared_scalar"] = summary(measure(args.reps, lambda: mul_each(1)), n)
        enc = np.zeros(576 * n, dtype=np.uint8)
        assert lib.bh_gt_read(gt, 0, n, ptr(enc)) == 0

        def upload_checked():
            h = ctypes.c_void_p()
            code = lib.bh_gt_upload(ctx.h, ptr(enc), n, 1, ctypes.byref(h))
            assert code == 0, code
            lib.bh_gt_free(h)

        rec["upload_checked"] = summary(measure(args.reps, upload_checked), n)
        lib.bh_gt_free(gt)
        print(json.dumps(rec), flush=True)
        del g1, g2

    n = args.baseline_len
    g1, g2 = vectors(n)

    def per_value():
        return [bh.final_exponentiation(bh.multi_miller_loop(ctx, g1, g2, i, i, 1)) for i in range(n)]

    rec = {"len": n, "what": "bh_miller_product on one pair + bh_final_exponentiation on the host, per value"}
    rec["per_value"] = summary(measure(args.reps, per_value), n)
    # the two paths agree: conj(e0)^3 of the per-value result is the Gt vector's element
    want = bh.pairing(ctx, g1, g2).to_bytes()
    from oracle import pairing as pr
    for i, e0 in enumerate(per_value()):
        c = [v if k % 2 == 0 else pr.F2.neg(v) for k, v in enumerate(e0)]
        assert bh.gt_format(pr.f12_mul(pr.f12_sqr(c), c)) == want[576 * i:576 * i + 576]
    print(json.dumps(rec), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
