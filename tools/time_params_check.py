#!/usr/bin/env python3
"""Timings of bh_params_check beside the rebuild it replaces.

For each 2^log_m: the MiMC chain whose domain size is m = 2^log_m (rounds = m / 2 - 1), the round-one
storage of length 2 m after one contribution with known scalars, and the generator's Parameters for
those scalars.  Then, in the same process, medians of --reps runs after one warm-up of

  * bh_params_check of those Parameters, with bh_params_last_check_ms's split into the scalar side
    (powers, evaluation, row products, inverse NTTs), the sixteen multiexps and the pairings;
  * bh_mpc_common_matrix on the same storage and circuit: what a receiver had to run before this
    check existed (and every round-two contribution after it), with bh_mpc_last_matrix_ms's split.

Every call synchronises, so host wall time is the device time plus the call's allocations.
usage: time_params_check.py [--log-m 16 20] [--reps 5] [--matrix-reps 5]"""
import argparse
import ctypes
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
    ap.add_argument("--log-m", type=int, nargs="+", default=[16, 20])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--matrix-reps", type=int, default=5)
    args = ap.parse_args()
    import bellman_hip as bh
    ctx = bh.Context(0)
    q = bh.R_MODULUS
    toxic = dict(alpha=0x1F2E3D4C5B6A79881122334455667788AABBCCDDEEFF00112233445566778899 % q,
                 beta=0x0123456789ABCDEFFEDCBA9876543210AABBCCDD00112233445566778899AABB % q,
                 gamma=0x3C4D5E6F708192A3B4C5D6E7F8091A2B3C4D5E6F708192A3B4C5D6E7F8091A2B % q,
                 delta=0x0F1E2D3C4B5A69788796A5B4C3D2E1F0FEDCBA98765432100123456789ABCDEF % q,
                 tau=0x5AB3F1C2D4E6978877665544332211FFEEDDCCBBAA99887766554433221100FF % q)
    rho = 0x2B7E151628AED2A6ABF7158809CF4F3C762E7160F38B4DA56A784D9045190CFE % q
    sigma = 0x243F6A8885A308D313198A2E03707344A4093822299F31D0082EFA98EC4E6C89 % q
    for log_m in args.log_m:
        m = 1 << log_m
        r1cs = bh.R1CS.chain(ctx, m // 2 - 1)
        sz = r1cs.sizes()
        assert m // 2 < sz["constraints"] <= m
        st = bh.initial_common_paramters(ctx, 2 * m)
        c = bh.mpc_common_paramters_generator(ctx, st, (toxic["alpha"], toxic["beta"], toxic["tau"]))
        st = bh.verify_common_paramter_structure(ctx, st, c, rho)
        assert st is not None
        del c
        params, gen_ms = timed(lambda: bh.Parameters.generate(ctx, r1cs, **toxic))
        rec = {"m": m, "sizes": sz, "params": params.sizes(), "generate_ms": round(gen_ms, 1)}

        total, split = [], []
        for _ in range(args.reps + 1):
            mask, ms = timed(lambda: params.check(r1cs, st, rho, sigma))
            assert mask == 0
            total.append(ms)
            split.append(bh.last_params_check_ms())
        rec["check"] = dict(summary(total[1:]), first_ms=round(total[0], 1),
                            median_scalar_ms=round(statistics.median(s[0] for s in split[1:]), 1),
                            median_multiexp_ms=round(statistics.median(s[1] for s in split[1:]), 1),
                            median_pairing_ms=round(statistics.median(s[2] for s in split[1:]), 1))

        total, split = [], []
        for _ in range(args.matrix_reps + 1):
            mx, ms = timed(lambda: st.matrix(r1cs))
            out = (ctypes.c_double * 3)()
            bh.lib().bh_mpc_last_matrix_ms(out)
            total.append(ms)
            split.append(tuple(out))
            del mx
        rec["matrix"] = dict(summary(total[1:]), first_ms=round(total[0], 1),
                             median_fft_ms=round(statistics.median(s[0] for s in split[1:]), 1),
                             median_product_ms=round(statistics.median(s[1] for s in split[1:]), 1),
                             median_h_ms=round(statistics.median(s[2] for s in split[1:]), 1))
        rec["matrix_over_check"] = round(rec["matrix"]["median_ms"] / rec["check"]["median_ms"], 1)
        print(json.dumps(rec), flush=True)
        del params, st, r1cs
    ctx.close()


if __name__ == "__main__":
    main()
