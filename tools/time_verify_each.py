#!/usr/bin/env python3
"""Timings of per-proof verdicts: bh_verify_each_device against the batch
verifier on the same proofs (bh_verify_batch_device, one verdict for all) and against a loop over
bh_verify_proof on the host, and bh_final_exponentiation_batch alone.

Four proofs are made once with prove_batch (a MiMC chain of --rounds rounds, four distinct
witnesses) and tiled to k: the work per proof does not depend on the proofs being distinct.  For
each k one warm-up of both device paths, then --reps timed runs, the two alternating; the host
clock around calls that return synchronised.  Every run's answers are asserted.  The host loop runs
over --host-proofs proofs once and is SCALED to k (labelled so): it is one thread's time per proof
times k.  The final exponentiation runs on seeded random values.  Prints one line per run, medians
and spreads, and one JSON line.

usage: time_verify_each.py [--k 64 1024 16384] [--fexp-n 1024 65536] [--reps 5] [--host-proofs 16]
       time_verify_each.py --trace-k 16384     one warm-up and one bh_verify_each_device call and
                                               nothing else: the run to put under a kernel trace
       time_verify_each.py --stats FILE.csv    a kernel trace's per-kernel statistics
                                               (Name, Calls, TotalDurationNs columns) by stage"""
import argparse
import csv
import ctypes
import json
import os
import random
import re
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bellman-mpc_amd"))
sys.path.insert(0, ROOT)

# kernel name prefix -> stage of bh_verify_each_device
# (the table's k_varbase_multiples, k_normalize and k_points_to_dev launches, microseconds for a handful of
# bases, also serve whatever made the proofs and stay under "other")
STAGES = [("k_proof_", "1 decode (Proof::read)"), ("k_each_", "2 accumulated inputs"), ("k_miller_", "3 Miller loops"),
          ("k_fexp_scale", "4 constant pair"), ("k_fexp_steps", "5 final exponentiation"),
          ("k_fexp_is_one", "6 verdicts")]


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, (time.perf_counter() - t0) * 1e3


def summary(v, k):
    med = statistics.median(v)
    return {"ms": [round(x, 1) for x in v], "median_ms": round(med, 1), "spread_ms": round(max(v) - min(v), 1),
            "per_item_us": round(med / k * 1e3, 1)}


def stage_shares(path):
    """a kernel-stats CSV -> printed shares per stage"""
    by_stage, total = {}, 0.0
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            ns = float(row.get("TotalDurationNs") or row.get("TotalDuration(ns)") or 0)
            m = re.search(r"\bk_[A-Za-z0-9_]+", name)  # the kernel's own name inside the demangled signature
            short = m.group(0) if m else name
            stage = next((s for pre, s in STAGES if short.startswith(pre)), "other: " + short[:40])
            by_stage[stage] = by_stage.get(stage, 0.0) + ns
            total += ns
    for stage, ns in sorted(by_stage.items()):
        print(f"{stage:32s} {ns / 1e6:10.2f} ms  {100 * ns / total:5.1f} %")
    print(f"{'all kernels':32s} {total / 1e6:10.2f} ms")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, nargs="*", default=[64, 1 << 10, 1 << 14])
    ap.add_argument("--fexp-n", type=int, nargs="*", default=[1 << 10, 1 << 16])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-proofs", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=255)
    ap.add_argument("--trace-k", type=int, default=0)
    ap.add_argument("--stats", default=None)
    args = ap.parse_args()
    if args.stats:
        return stage_shares(args.stats)
    import bellman_hip as bh
    lib = bh.lib()
    ctx = bh.Context(0)
    params = bh.Parameters.chain(ctx, args.rounds)
    ws = [bh.Witness.chain(ctx, args.rounds, seed=7, preimage_seed=20 + i) for i in range(4)]
    base_proofs = bh.prove_batch(ctx, params, ws, 27134, 17146)
    vkb = np.frombuffer(bytes(params.vk_bytes()), dtype=np.uint8)
    base_publics = [bh.fr_from_mont(bh.chain_assignment(args.rounds, seed=7, preimage_seed=20 + i)["inputs"])[1:]
                    for i in range(4)]
    ni = len(base_publics[0])
    rng = random.Random(2025)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731

    def arrays(k):
        pf = np.frombuffer(b"".join(base_proofs[i % 4] for i in range(k)), dtype=np.uint8)
        ins = bh.fr_to_canonical_limbs([x for i in range(k) for x in base_publics[i % 4]])
        return pf, ins

    def each(k, pf, ins):
        st, ok = np.full(k, 7, dtype=np.uint32), np.zeros(k, dtype=np.uint8)
        ret = lib.bh_verify_each_device(ctx.h, p(vkb), vkb.size, p(pf), p(ins), ni, k, p(st), p(ok))
        return ret == 0 and not st.any() and ok.all()

    if args.trace_k:
        pf, ins = arrays(args.trace_k)
        for _ in range(2):
            assert each(args.trace_k, pf, ins)
        ctx.close()
        return

    out = {"rounds": args.rounds, "reps": args.reps, "num_inputs": ni, "k": [], "fexp": []}
    # the host loop, once: one thread's time per proof
    pf, ins = arrays(args.host_proofs)
    ok = ctypes.c_int()
    host_ms = []
    for j in range(args.host_proofs):
        st, ms = timed(lambda: lib.bh_verify_proof(p(vkb), vkb.size, p(pf[192 * j:]), p(ins[ni * j:]), ni,
                                                   ctypes.byref(ok)))
        assert st == 0 and ok.value == 1
        host_ms.append(ms)
    host_per_proof = statistics.median(host_ms)
    out["host_per_proof_ms"] = round(host_per_proof, 2)
    print(f"host bh_verify_proof: median {host_per_proof:.2f} ms per proof over {args.host_proofs} proofs "
          f"(min {min(host_ms):.2f}, max {max(host_ms):.2f})", flush=True)

    for k in args.k:
        pf, ins = arrays(k)
        z = bh.fr_to_canonical_limbs([rng.randrange(1, bh.R_MODULUS) for _ in range(k)])

        def batch():
            v = ctypes.c_int()
            st = lib.bh_verify_batch_device(ctx.h, p(vkb), vkb.size, p(pf), p(ins), ni, k, p(z), ctypes.byref(v))
            return st == 0 and v.value == 1

        paths = [("each", lambda: each(k, pf, ins)), ("batch", batch)]
        runs = {name: [] for name, _ in paths}
        for rep in range(args.reps + 1):  # rep 0: the warm-up
            for name, fn in paths:
                good, ms = timed(fn)
                assert good, (name, k)
                print(f"k={k} {name} {'warm-up' if rep == 0 else 'run ' + str(rep)}: {ms:.1f} ms", flush=True)
                if rep:
                    runs[name].append(ms)
        rec = {"k": k, "each": summary(runs["each"], k), "batch": summary(runs["batch"], k),
               "host_loop_scaled_ms": round(host_per_proof * k, 1)}
        for name in ("each", "batch"):
            r = rec[name]
            print(f"k={k} {name}: median {r['median_ms']} ms, spread {r['spread_ms']} ms, {r['per_item_us']} us per proof",
                  flush=True)
        print(f"k={k} host loop (SCALED from {args.host_proofs} proofs): {rec['host_loop_scaled_ms']} ms", flush=True)
        out["k"].append(rec)

    for n in args.fexp_n:
        # 256 distinct values tiled to n; coefficients below 2^380 < p
        vals = np.frombuffer(b"".join(rng.getrandbits(380).to_bytes(48, "big") for _ in range(12 * min(n, 256))),
                             dtype=np.uint8)
        src = np.tile(vals, (n + 255) // 256)[:576 * n].copy()
        dst = np.zeros(576 * n, dtype=np.uint8)
        runs = []
        for rep in range(args.reps + 1):
            st, ms = timed(lambda: lib.bh_final_exponentiation_batch(ctx.h, p(src), n, p(dst)))
            assert st == 0
            print(f"fexp n={n} {'warm-up' if rep == 0 else 'run ' + str(rep)}: {ms:.1f} ms", flush=True)
            if rep:
                runs.append(ms)
        one = np.zeros(576, dtype=np.uint8)
        assert lib.bh_final_exponentiation(p(src), p(one)) == 0 and one.tobytes() == dst[:576].tobytes()
        rec = {"n": n, **summary(runs, n)}
        print(f"fexp n={n}: median {rec['median_ms']} ms, spread {rec['spread_ms']} ms, {rec['per_item_us']} us per value",
              flush=True)
        out["fexp"].append(rec)
    print(json.dumps(out))
    ctx.close()


if __name__ == "__main__":
    main()
