#!/usr/bin/env python3
"""Timings of the ceremony rounds on the device.

  * bh_srs_mul_powers for G1 and G2 at 2^log_len points, --reps runs after one warm-up: median,
    spread, points/s (the one-time A/B of the signed-window kernel against the plain
    double-and-add it replaced is profiles/mpc_ab_varbase_window_2p20.txt);
  * the same length through k_fixed_base (the "mine" lists of a contribution; read it from the
    kernel statistics of a profiler run of this tool, it has no API of its own);
  * one full round-one contribution at that length;
  * one verification at each 2^log_verify, --reps runs after one warm-up, on both paths of its
    len Miller loops per vector pair: the device product (the default) and the host's pool threads
    (BH_MPC_HOST_MILLER=1, which the library reads at every verification), with the Miller share
    shown separately.  Sizes above --host-max-log time the device path only (the host path is
    minutes per run there).

Every call synchronises, so host wall time is the device time plus the call's allocations.
usage: time_mpc.py [--log-len 20] [--log-verify 10 [16 20 ...]] [--host-max-log 10] [--reps 3]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-len", type=int, default=20)
    ap.add_argument("--log-verify", type=int, nargs="+", default=[10])
    ap.add_argument("--host-max-log", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    import bellman_hip as bh
    ctx = bh.Context(0)
    n = 1 << args.log_len
    a, x = 0x1F2E3D4C5B6A79881122334455667788, 0x0123456789ABCDEFFEDCBA9876543210AABBCCDD
    out = {"len": n}

    st0, ms = timed(lambda: bh.initial_common_paramters(ctx, n))
    out["initial_ms"] = round(ms, 1)
    # distinct points: one contribution's worth of powers on the generators
    vec = {1: st0.tau_g1.mul_powers(3, 5), 2: st0.tau_g2.mul_powers(3, 5)}

    for group in (1, 2):
        runs = [timed(lambda: vec[group].mul_powers(a, x))[1] for _ in range(args.reps + 1)][1:]
        med = statistics.median(runs)
        out[f"mul_powers_g{group}"] = {"ms": [round(v, 2) for v in runs], "median_ms": round(med, 2),
                                       "spread_ms": round(max(runs) - min(runs), 2),
                                       "points_per_s": round(n / med * 1e3)}

    c, ms = timed(lambda: bh.mpc_common_paramters_generator(ctx, st0, (a, x, a ^ x)))
    out["contribution_ms"] = round(ms, 1)
    del c, vec, st0

    out["verify"] = []
    for log_verify in args.log_verify:
        nv = 1 << log_verify
        st = bh.initial_common_paramters(ctx, nv)
        c = bh.mpc_common_paramters_generator(ctx, st, (a, x, a ^ x))
        z = bh.random_z(nv)
        rec = {"len": nv, "miller_loops": 2 * nv}
        for path in ("device", "host"):
            if path == "host" and log_verify > args.host_max_log:
                continue
            os.environ["BH_MPC_HOST_MILLER"] = "1" if path == "host" else "0"
            total, miller = [], []
            for _ in range(args.reps + 1):
                nxt, ms = timed(lambda: bh.verify_common_paramter(ctx, st, c, z=z))
                assert nxt is not None
                assert bh.lib().bh_mpc_last_miller_device() == (2 if path == "device" else 0)
                total.append(ms)
                miller.append(bh.lib().bh_mpc_last_miller_ms())
            total, miller = total[1:], miller[1:]
            rec[path] = {"total_ms": [round(v, 1) for v in total], "miller_ms": [round(v, 1) for v in miller],
                         "median_total_ms": round(statistics.median(total), 1),
                         "median_miller_ms": round(statistics.median(miller), 1),
                         "spread_total_ms": round(max(total) - min(total), 1),
                         "pairs_per_s": round(2 * nv / statistics.median(miller) * 1e3)}
        os.environ.pop("BH_MPC_HOST_MILLER", None)
        out["verify"].append(rec)
        del st, c
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
