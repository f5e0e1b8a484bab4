#!/usr/bin/env python3
"""Timings of the batch verifier on its two paths: bh_verify_batch (one host
thread) and bh_verify_batch_device (the per-proof work on the device).

Four proofs are made once with prove_batch (a MiMC chain of --rounds rounds, four distinct
witnesses) and tiled to k; the work per proof does not depend on the proofs being distinct, and the
z values are distinct (random, full width).  For each k: one warm-up of every path that runs there,
then --reps timed runs, host and device alternating where both run; the host clock around the call.
Every run's verdict is asserted.  Prints one line per run, the medians and spreads, the comparison
per k where both paths ran, and one JSON line.

usage: time_verify.py [--host-k 256 1024] [--device-k 1024 16384 65536] [--reps 3] [--rounds 255]
       (--host-k with no value: device runs only, e.g. under a profiler)"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--host-k", type=int, nargs="*", default=[256, 1024])
    ap.add_argument("--device-k", type=int, nargs="*", default=[1024, 1 << 14, 1 << 16])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=255)
    args = ap.parse_args()
    import bellman_hip as bh
    ctx = bh.Context(0)
    params = bh.Parameters.chain(ctx, args.rounds)
    ws = [bh.Witness.chain(ctx, args.rounds, seed=7, preimage_seed=20 + i) for i in range(4)]
    base_proofs = bh.prove_batch(ctx, params, ws, 27134, 17146)
    vkb = np.frombuffer(bytes(params.vk_bytes()), dtype=np.uint8)
    base_publics = [bh.fr_from_mont(bh.chain_assignment(args.rounds, seed=7, preimage_seed=20 + i)["inputs"])[1:]
                    for i in range(4)]
    rng = random.Random(2025)
    out = {"rounds": args.rounds, "reps": args.reps, "k": []}
    for k in sorted(set(args.host_k) | set(args.device_k)):
        # the C calls on arrays built beforehand: the Python layer's marshalling is not the verifier's time
        pf = np.frombuffer(b"".join(base_proofs[i % 4] for i in range(k)), dtype=np.uint8)
        ins = bh.fr_to_canonical_limbs([x for i in range(k) for x in base_publics[i % 4]])
        z = bh.fr_to_canonical_limbs([rng.randrange(1, bh.R_MODULUS) for _ in range(k)])
        ni = len(base_publics[0])
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731

        def call(fn, *head):
            ok = ctypes.c_int()
            st = fn(*head, p(vkb), vkb.size, p(pf), p(ins), ni, k, p(z), ctypes.byref(ok))
            return st == 0 and ok.value == 1

        paths = [(name, fn) for name, fn, ks in (
            ("host", lambda: call(bh.lib().bh_verify_batch), args.host_k),
            ("device", lambda: call(bh.lib().bh_verify_batch_device, ctx.h), args.device_k)) if k in ks]
        runs = {name: [] for name, _ in paths}
        for rep in range(args.reps + 1):  # rep 0: the warm-up
            for name, fn in paths:
                ok, ms = timed(fn)
                assert ok is True, (name, k)
                print(f"k={k} {name} {'warm-up' if rep == 0 else 'run ' + str(rep)}: {ms:.1f} ms", flush=True)
                if rep:
                    runs[name].append(ms)
        rec = {"k": k}
        for name, v in runs.items():
            med = statistics.median(v)
            rec[name] = {"ms": [round(x, 1) for x in v], "median_ms": round(med, 1),
                         "spread_ms": round(max(v) - min(v), 1), "per_proof_us": round(med / k * 1e3, 1)}
            print(f"k={k} {name}: median {med:.1f} ms, spread {max(v) - min(v):.1f} ms, "
                  f"{med / k * 1e3:.1f} us per proof", flush=True)
        if len(runs) == 2:
            gap = rec["host"]["median_ms"] - rec["device"]["median_ms"]
            spread = max(rec["host"]["spread_ms"], rec["device"]["spread_ms"])
            verdict = "device faster" if gap > spread else "host faster" if -gap > spread else "no difference shown"
            rec["gap_ms"], rec["verdict"] = round(gap, 1), verdict
            print(f"k={k}: host - device = {gap:.1f} ms against the larger spread {spread:.1f} ms: {verdict}",
                  flush=True)
        out["k"].append(rec)
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
