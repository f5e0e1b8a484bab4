#!/usr/bin/env python3
"""Times the two ways to a resident witness of the MiMC chain, in one process on one context:
bh_witness_upload of the host-evaluated a, b, c (the evaluation itself is NOT timed: it is
bh_chain_assignment's, natively on the host) and bh_r1cs_witness, which takes only the
assignment and computes a, b, c and the density maps on the device from R1CS.chain's matrices.

Timed, with a host clock around calls that end in a device synchronise, after a warm-up of each:
  upload       bh_witness_upload
  cold         bh_r1cs_witness, first call on a fresh handle: the row view is built
  warm         bh_r1cs_witness on a handle that has its row view
  warm_check   the same with the satisfaction pass
The upload and the warm call alternate.  The two witnesses are read back and compared word for word
before anything is timed.  Prints one JSON line with every sample, the medians, the bytes each path
moves over PCIe and the --box label of the machine.

  python tools/time_witness.py [--rounds 524287] [--reps 5] [--box NAME]      # 2^20 constraints by default
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "bellman-mpc_amd"))

VECS = ("a", "b", "c", "inputs", "aux")
DENS = ("a_aux_density", "b_input_density", "b_aux_density")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=(1 << 19) - 1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--box", default="MI355X", help="label of the machine measured, copied into the result")
    args = ap.parse_args()
    import bellman_hip as bh

    ctx = bh.Context(0)
    lib = bh.lib()
    asg = bh.chain_assignment(args.rounds)
    nc, ni, na = asg["a"].shape[0], asg["inputs"].shape[0], asg["aux"].shape[0]
    ptr = {k: asg[k].ctypes.data_as(ctypes.c_void_p) for k in VECS + DENS}

    def timed(f):
        ctx.synchronize()
        t0 = time.perf_counter()
        out = f()
        ctx.synchronize()
        return out, time.perf_counter() - t0

    def upload():
        h = ctypes.c_void_p()
        code = lib.bh_witness_upload(ctx.h, ptr["a"], ptr["b"], ptr["c"], nc, ptr["inputs"], ni, ptr["aux"], na,
                                     ptr["a_aux_density"], ptr["b_input_density"], ptr["b_aux_density"],
                                     ctypes.byref(h))
        assert code == 0, code
        return bh.Witness(ctx, h, nc)

    def product(r1cs, check=False):
        return bh.Witness.from_r1cs(ctx, r1cs, asg["inputs"], asg["aux"], check=check)

    # warm-up of each (code objects, staging ring, allocations) and the comparison
    r1cs = bh.R1CS.chain(ctx, args.rounds)
    w_up, w_dev = upload(), product(r1cs, check=True)
    assert w_dev[1] is None, "the chain's own assignment must satisfy it"
    got_up, got_dev = w_up.read(raw=True), w_dev[0].read(raw=True)
    for k in VECS + DENS:
        assert np.array_equal(got_up[k], got_dev[k]), k
    del w_up, w_dev, got_up, got_dev

    t_cold = []
    for _ in range(args.reps):
        fresh = bh.R1CS.chain(ctx, args.rounds)
        t_cold.append(timed(lambda: product(fresh))[1])
        del fresh
    t_up, t_warm, t_check = [], [], []
    for _ in range(args.reps):  # alternating, so that drift hits all alike
        t_up.append(timed(upload)[1])
        t_warm.append(timed(lambda: product(r1cs))[1])
        t_check.append(timed(lambda: product(r1cs, check=True))[1])
    sz = r1cs.sizes()
    dens_bytes = 8 * sum(asg[k].shape[0] for k in DENS)
    med = lambda t: round(statistics.median(t), 5)
    res = {
        "box": args.box, "rounds": args.rounds, "constraints": nc, "inputs": ni, "aux": na,
        "terms": sz["nnz_a"] + sz["nnz_b"] + sz["nnz_c"], "reps": args.reps,
        "upload_s": [round(t, 5) for t in t_up], "cold_s": [round(t, 5) for t in t_cold],
        "warm_s": [round(t, 5) for t in t_warm], "warm_check_s": [round(t, 5) for t in t_check],
        "upload_median_s": med(t_up), "cold_median_s": med(t_cold), "warm_median_s": med(t_warm),
        "warm_check_median_s": med(t_check),
        "upload_spread_s": round(max(t_up) - min(t_up), 5), "warm_spread_s": round(max(t_warm) - min(t_warm), 5),
        "upload_pcie_bytes": 32 * (3 * nc + ni + na) + dens_bytes,
        "r1cs_witness_pcie_bytes": 32 * (ni + na),
        "r1cs_witness_check_pcie_bytes": 32 * (ni + na) + 4,
        "read_back_equal": True,
    }
    print(json.dumps(res))
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
