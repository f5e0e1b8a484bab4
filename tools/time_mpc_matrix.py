#!/usr/bin/env python3
"""Timings of the step between the ceremony's rounds.

At each 2^log_len (default 16 and 20), --reps runs after one warm-up, medians and spreads:
  * bh_srs_fft forward and inverse, in G1 and G2, of tau^i G;
  * the inverse transform with BH_GROUP_FFT_W1=none (every butterfly multiplies) and =prefix (every
    stage's w = 1 prefix skips its multiplication, where the default skips the first stage's only:
    the A/B of that shortcut), and the share of the inverse's last 1/n pass (inverse minus forward:
    the two differ in nothing else);
  * bh_mpc_common_matrix on the MiMC chain whose domain has that size, from a storage of twice the
    length after one contribution, split by bh_mpc_last_matrix_ms into the six transforms, the
    matrix product and the h basis.
Beside each figure stands the prediction from the measured bh_srs_mul_powers rates (section 11):
a transform as (n / 2) log2 n multiplications, the product as one per term and use.

Every call synchronises, so host wall time is the device time plus the call's allocations.
usage: time_mpc_matrix.py [--log-len 16 20] [--reps 3] [--skip-matrix]"""
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

RATE = {1: 19.5e6, 2: 6.1e6}  # bh_srs_mul_powers, points/s at 2^20


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, (time.perf_counter() - t0) * 1e3


def summary(runs):
    return {"ms": [round(v, 1) for v in runs], "median_ms": round(statistics.median(runs), 1),
            "spread_ms": round(max(runs) - min(runs), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-len", type=int, nargs="+", default=[16, 20])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip-matrix", action="store_true")
    args = ap.parse_args()
    import bellman_hip as bh
    ctx = bh.Context(0)
    a, b, tau = 0x1F2E3D4C5B6A79881122334455667788, 0x0123456789ABCDEFFEDCBA9876543210AABBCCDD, \
        0x5AB3F1C2D4E6978877665544332211FFEEDDCCBBAA99887766554433221100FF % bh.R_MODULUS
    out = {"sizes": []}
    for L in args.log_len:
        n = 1 << L
        rec = {"len": n}
        for group in (1, 2):
            vec = _powers(bh, ctx, group, n, tau)
            pred = (n / 2) * L / RATE[group] * 1e3
            g = {"predicted_ms": round(pred, 1)}
            for name, inverse, env in (("fft", False, None), ("ifft", True, None), ("ifft_w1_none", True, "none"),
                                       ("ifft_w1_prefix", True, "prefix")):
                if env:
                    os.environ["BH_GROUP_FFT_W1"] = env
                runs = [timed(lambda: vec.fft(inverse))[1] for _ in range(args.reps + 1)][1:]
                os.environ.pop("BH_GROUP_FFT_W1", None)
                g[name] = summary(runs)
            g["scale_pass_ms"] = round(g["ifft"]["median_ms"] - g["fft"]["median_ms"], 1)
            g["ifft_over_prediction"] = round(g["ifft"]["median_ms"] / pred, 2)
            rec[f"g{group}"] = g
            del vec
        if not args.skip_matrix:
            rounds = n // 2 - 1  # 2 * rounds + 2 constraints with the input rows
            r1cs = bh.R1CS.chain(ctx, rounds)
            sz = r1cs.sizes()
            storage = _contributed(bh, ctx, 2 * n, (a, b, tau))
            parts = []
            total = []
            for _ in range(args.reps + 1):
                mx, ms = timed(lambda: storage.matrix(r1cs))
                p = (ctypes.c_double * 3)()
                bh.lib().bh_mpc_last_matrix_ms(p)
                parts.append(list(p))
                total.append(ms)
                del mx
            parts, total = parts[1:], total[1:]
            na, nb_, nc = sz["nnz_a"], sz["nnz_b"], sz["nnz_c"]
            pred_t = 3 * (n / 2) * L * (1 / RATE[1] + 1 / RATE[2]) * 1e3
            pred_p = ((2 * na + 2 * nb_ + nc) / RATE[1] + (na + 2 * nb_ + nc) / RATE[2]) * 1e3
            rec["matrix"] = {
                "constraints": sz["constraints"], "terms": [na, nb_, nc], "total": summary(total),
                "transforms": summary([p[0] for p in parts]), "product": summary([p[1] for p in parts]),
                "h_basis": summary([p[2] for p in parts]),
                "predicted_transforms_ms": round(pred_t, 1), "predicted_product_ms": round(pred_p, 1)}
            del storage, r1cs
        out["sizes"].append(rec)
    out["kernels_checked"] = ctx.scratch_report()["kernels_checked"]
    print(json.dumps(out))
    ctx.close()


def _powers(bh, ctx, group, n, tau):
    st = bh.initial_common_paramters(ctx, n)
    return (st.tau_g1 if group == 1 else st.tau_g2).mul_powers(1, tau)


def _contributed(bh, ctx, length, player):
    """A storage of that length after one player: verified, as a ceremony would hold it."""
    st = bh.initial_common_paramters(ctx, length)
    nxt = bh.verify_common_paramter(ctx, st, bh.mpc_common_paramters_generator(ctx, st, player))
    assert nxt is not None
    return nxt


if __name__ == "__main__":
    main()
