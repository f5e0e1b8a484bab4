#!/usr/bin/env python3
"""Timings of the ceremony's structure check.

For each 2^log_len: one round-one contribution to the initial storage, then, on that contribution in
the same run, medians of --reps runs after one warm-up of

  * bh_mpc_common_check of the contribution's storage, with bh_mpc_last_check_ms's split into the
    weights plus the eight multiexps and the pairing equations;
  * bh_mpc_common_verify_structure of the contribution (the same check plus three ratio proofs and
    the copy of the six vectors into the next storage), with the same split;
  * bh_mpc_common_verify of the contribution (2 len Miller loops on the device), with the Miller share.

Every call synchronises, so host wall time is the device time plus the call's allocations.  The z of
bh_mpc_common_verify are drawn before its clock starts; the rho of the other two is one scalar.
usage: time_mpc_check.py [--log-len 12 16 20] [--reps 5]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bellman-mpc_amd"))
sys.path.insert(0, ROOT)


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, (time.perf_counter() - t0) * 1e3


def summary(runs):
    return {"ms": [round(v, 1) for v in runs], "median_ms": round(statistics.median(runs), 1),
            "spread_ms": round(max(runs) - min(runs), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-len", type=int, nargs="+", default=[12, 16, 20])
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import bellman_hip as bh
    ctx = bh.Context(0)
    a, x = 0x1F2E3D4C5B6A79881122334455667788, 0x0123456789ABCDEFFEDCBA9876543210AABBCCDD
    rho = 0x2B7E151628AED2A6ABF7158809CF4F3C762E7160F38B4DA56A784D9045190CFE % bh.R_MODULUS
    for log_len in args.log_len:
        n = 1 << log_len
        st = bh.initial_common_paramters(ctx, n)
        c = bh.mpc_common_paramters_generator(ctx, st, (a, x, a ^ x))
        z = bh.random_z(n)
        z_words = bh._z_words(z)
        rec = {"len": n}

        nxt = bh.verify_common_paramter_structure(ctx, st, c, rho)
        assert nxt is not None
        total, split = [], []
        for _ in range(args.reps + 1):
            mask, ms = timed(lambda: nxt.check(rho))
            assert mask == 0
            total.append(ms)
            split.append(bh.last_check_ms())
        rec["check"] = dict(summary(total[1:]), median_multiexp_ms=round(statistics.median(s[0] for s in split[1:]), 1),
                            median_pairing_ms=round(statistics.median(s[1] for s in split[1:]), 1))
        del nxt

        total, split = [], []
        for _ in range(args.reps + 1):
            got, ms = timed(lambda: bh.verify_common_paramter_structure(ctx, st, c, rho))
            assert got is not None
            total.append(ms)
            split.append(bh.last_check_ms())
            del got
        rec["verify_structure"] = dict(summary(total[1:]),
                                       median_multiexp_ms=round(statistics.median(s[0] for s in split[1:]), 1),
                                       median_pairing_ms=round(statistics.median(s[1] for s in split[1:]), 1))

        total, miller = [], []
        import ctypes
        for _ in range(args.reps + 1):
            valid, h = ctypes.c_int(), ctypes.c_void_p()

            def run():
                return bh.lib().bh_mpc_common_verify(ctx.h, st.h, c.h, z_words.ctypes.data_as(ctypes.c_void_p),
                                                     ctypes.byref(valid), ctypes.byref(h))
            code, ms = timed(run)
            assert code == 0 and valid.value == 1
            assert bh.lib().bh_mpc_last_miller_device() == 2
            bh.lib().bh_mpc_common_free(h)
            total.append(ms)
            miller.append(bh.lib().bh_mpc_last_miller_ms())
        rec["verify"] = dict(summary(total[1:]), median_miller_ms=round(statistics.median(miller[1:]), 1))
        rec["verify_over_verify_structure"] = round(rec["verify"]["median_ms"] / rec["verify_structure"]["median_ms"], 2)
        print(json.dumps(rec), flush=True)
        del st, c
    ctx.close()


if __name__ == "__main__":
    main()
