#!/usr/bin/env python3
"""Times CRS generation for the MiMC chain two ways, in one process on one context:
Parameters.chain (bh_chain_params: the QAP evaluation on the host) and
Parameters.generate(R1CS.chain(...)) (bh_generate_parameters: the general device generator).

After one warm-up of each, three repetitions of each are timed (host clock around calls that end
in a device synchronise), bh_r1cs_create (synthesis + flattening + upload, bh_chain_r1cs) is
timed separately, and the two Parameters::write outputs are compared byte for byte.  Prints one
JSON line.

  python tools/time_generate.py [--rounds 524287]      # 2^20 constraints by default
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bellman-mpc_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=(1 << 19) - 1)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    import bellman_hip as bh

    ctx = bh.Context(0)

    def timed(f):
        ctx.synchronize()
        t0 = time.perf_counter()
        out = f()
        ctx.synchronize()
        return out, time.perf_counter() - t0

    chain = lambda: bh.Parameters.chain(ctx, args.rounds)
    # warm-up of each: code objects, the domain's tables, allocations
    ref_bytes = chain().write()
    r1cs, _ = timed(lambda: bh.R1CS.chain(ctx, args.rounds))
    general = lambda: bh.Parameters.generate(ctx, r1cs)
    assert general().write() == ref_bytes, "bh_generate_parameters differs from bh_chain_params"
    t_create = [timed(lambda: bh.R1CS.chain(ctx, args.rounds))[1] for _ in range(args.reps)]
    t_chain, t_general = [], []
    for _ in range(args.reps):  # alternating, so that drift hits both alike
        t_chain.append(timed(chain)[1])
        t_general.append(timed(general)[1])
    sz = r1cs.sizes()
    spread = max(t_chain) - min(t_chain)
    res = {
        "rounds": args.rounds, "constraints": sz["constraints"], "segment": sz["segment"],
        "chain_params_s": [round(t, 4) for t in t_chain],
        "generate_parameters_s": [round(t, 4) for t in t_general],
        "r1cs_create_s": [round(t, 4) for t in t_create],
        "chain_params_median_s": round(statistics.median(t_chain), 4),
        "generate_parameters_median_s": round(statistics.median(t_general), 4),
        "chain_params_spread_s": round(spread, 4),
        "bytes_equal": True,
        "not_slower": statistics.median(t_general) <= statistics.median(t_chain) + spread,
    }
    print(json.dumps(res))
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
