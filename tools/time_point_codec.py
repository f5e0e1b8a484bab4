#!/usr/bin/env python3
"""Timings of the point codecs: the compressed one against the uncompressed paths (DESIGN.md section
17), and, run once on this tree and once on a build of the parent commit (--package), the
uncompressed paths on the device codec against the parent's host loops (section 20).

For each 2^log_len and each group, on the vector a x^i G (bh_srs_mul_powers of the generators), the
two variants alternating in one process, medians of --reps runs after one warm-up of each:

  * bh_srs_upload(checked=0)  against  bh_srs_upload_compressed(checked=0)
  * bh_srs_read               against  bh_srs_read_compressed

and, at 2^--mpc-log-len, on the storage after one contribution,

  * bh_mpc_common_write / bh_mpc_common_read(checked=0)  against the compressed pair.

and, on the Parameters of the MiMC chain with 2^--params-log-len constraints (bh_chain_params),

  * bh_params_load(checked=0), bh_params_write, and where the library has them
    bh_params_load_compressed(checked=0), bh_params_write_compressed.

Every call synchronises, so host wall time is the device time plus the call's host work, copies and
allocations.  The bytes each call moves between host and device are reported alongside.
--package DIR imports bellman_hip from DIR (another build's bellman-mpc_amd directory) instead of
this tree's.
usage: time_point_codec.py [--log-len 16 20] [--mpc-log-len 16] [--params-log-len 16 20] [--reps 5]
                           [--package DIR]"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return r, (time.perf_counter() - t0) * 1e3


def summary(runs, nbytes):
    return {"ms": [round(v, 2) for v in runs], "median_ms": round(statistics.median(runs), 2),
            "spread_ms": round(max(runs) - min(runs), 2), "bytes": nbytes}


def alternate(reps, plain, comp):
    """One warm-up of each, then reps alternating runs of each: ([plain ms], [compressed ms])."""
    a, b = [], []
    for _ in range(reps + 1):
        a.append(timed(plain)[1])
        b.append(timed(comp)[1])
    return a[1:], b[1:]


def ptr(arr):
    return arr.ctypes.data_as(ctypes.c_void_p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-len", type=int, nargs="+", default=[16, 20])
    ap.add_argument("--mpc-log-len", type=int, default=16)
    ap.add_argument("--params-log-len", type=int, nargs="*", default=[16, 20])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--package", default=os.path.join(ROOT, "bellman-mpc_amd"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.package))
    import bellman_hip as bh
    lib = bh.lib()
    ctx = bh.Context(0)
    a, x = 0x1F2E3D4C5B6A79881122334455667788, 0x0123456789ABCDEFFEDCBA9876543210AABBCCDD

    for log_len in args.log_len:
        n = 1 << log_len
        gens = bh.initial_common_paramters(ctx, n)
        for group, name in ((bh.BH_G1, "G1"), (bh.BH_G2, "G2")):
            vec = gens.vector(group - 1).mul_powers(a, x)
            unc = np.frombuffer(vec.read(0, n), dtype=np.uint8)
            comp = np.frombuffer(vec.to_compressed(), dtype=np.uint8)
            rec = {"len": n, "group": name}

            def upload(fn, buf):
                h = ctypes.c_void_p()
                code = fn(ctx.h, group, ptr(buf), n, 0, ctypes.byref(h))
                assert code == 0, code
                return h

            handles = []
            t_unc, t_comp = alternate(args.reps, lambda: handles.append(upload(lib.bh_srs_upload, unc)),
                                      lambda: handles.append(upload(lib.bh_srs_upload_compressed, comp)))
            # the two uploads hold the same points
            back = np.zeros(unc.size, dtype=np.uint8)
            assert lib.bh_srs_read(handles[-1], 0, n, ptr(back)) == 0 and bytes(back) == bytes(unc)
            for h in handles:
                lib.bh_srs_free(h)
            rec["upload"] = summary(t_unc, int(unc.size))
            rec["upload_compressed"] = summary(t_comp, int(comp.size))
            rec["upload_compressed_over_upload"] = round(rec["upload_compressed"]["median_ms"] /
                                                         rec["upload"]["median_ms"], 3)

            out_u, out_c = np.zeros(unc.size, dtype=np.uint8), np.zeros(comp.size, dtype=np.uint8)

            def read(fn, out):
                code = fn(vec.h, 0, n, ptr(out))
                assert code == 0, code

            t_unc, t_comp = alternate(args.reps, lambda: read(lib.bh_srs_read, out_u),
                                      lambda: read(lib.bh_srs_read_compressed, out_c))
            assert bytes(out_u) == bytes(unc) and bytes(out_c) == bytes(comp)
            rec["read"] = summary(t_unc, int(unc.size))
            rec["read_compressed"] = summary(t_comp, int(comp.size))
            rec["read_compressed_over_read"] = round(rec["read_compressed"]["median_ms"] / rec["read"]["median_ms"], 3)
            print(json.dumps(rec), flush=True)
            del vec
        del gens

    n = 1 << args.mpc_log_len
    st = bh.initial_common_paramters(ctx, n)
    st = bh.verify_common_paramter_structure(ctx, st, bh.mpc_common_paramters_generator(ctx, st, (a, x, a ^ x)))
    assert st is not None
    sizes = {False: 4 + 576 + 864 * n, True: 4 + 288 + 432 * n}
    bufs = {c: np.zeros(sizes[c], dtype=np.uint8) for c in sizes}

    def write(compressed):
        fn = lib.bh_mpc_common_write_compressed if compressed else lib.bh_mpc_common_write
        got = ctypes.c_size_t()
        code = fn(st.h, ptr(bufs[compressed]), sizes[compressed], ctypes.byref(got))
        assert code == 0 and got.value == sizes[compressed], (code, got.value)

    def read(compressed):
        fn = lib.bh_mpc_common_read_compressed if compressed else lib.bh_mpc_common_read
        h = ctypes.c_void_p()
        code = fn(ctx.h, ptr(bufs[compressed]), sizes[compressed], 0, ctypes.byref(h))
        assert code == 0, code
        lib.bh_mpc_common_free(h)

    rec = {"len": n, "what": "bh_mpc_common"}
    t_unc, t_comp = alternate(args.reps, lambda: write(False), lambda: write(True))
    rec["write"] = summary(t_unc, sizes[False])
    rec["write_compressed"] = summary(t_comp, sizes[True])
    rec["write_compressed_over_write"] = round(rec["write_compressed"]["median_ms"] / rec["write"]["median_ms"], 3)
    t_unc, t_comp = alternate(args.reps, lambda: read(False), lambda: read(True))
    rec["read"] = summary(t_unc, sizes[False])
    rec["read_compressed"] = summary(t_comp, sizes[True])
    rec["read_compressed_over_read"] = round(rec["read_compressed"]["median_ms"] / rec["read"]["median_ms"], 3)
    # the compressed file holds the same storage
    assert bh.CommonParamterInStorage.read(ctx, bytes(bufs[True]), checked=False, compressed=True).write() == \
        bytes(bufs[False])
    print(json.dumps(rec), flush=True)
    del st

    for log_len in args.params_log_len:
        params = bh.Parameters.chain(ctx, (1 << (log_len - 1)) - 1)
        rec = {"constraints": 1 << log_len, "what": "bh_params", "sizes": params.sizes()}
        forms = [("", lib.bh_params_load, lib.bh_params_write)]
        if hasattr(lib, "bh_params_write_compressed"):
            forms.append(("_compressed", lib.bh_params_load_compressed, lib.bh_params_write_compressed))
        for suffix, load, write in forms:
            got = ctypes.c_size_t()
            assert write(params.h, None, 0, ctypes.byref(got)) == 0
            buf = np.zeros(got.value, dtype=np.uint8)

            def do_write():
                code = write(params.h, ptr(buf), buf.size, ctypes.byref(got))
                assert code == 0 and got.value == buf.size, (code, got.value)

            loaded = []

            def do_load():
                h = ctypes.c_void_p()
                code = load(ctx.h, ptr(buf), buf.size, 0, ctypes.byref(h))
                assert code == 0, code
                loaded.append(h)

            t_write, t_load = [], []
            for _ in range(args.reps + 1):  # one warm-up of each
                t_write.append(timed(do_write)[1])
                t_load.append(timed(do_load)[1])
                while len(loaded) > 1:
                    lib.bh_params_free(loaded.pop(0))
            rec["write" + suffix] = summary(t_write[1:], int(buf.size))
            rec["load" + suffix] = summary(t_load[1:], int(buf.size))
            # what was loaded writes the file it came from
            back = np.zeros(buf.size, dtype=np.uint8)
            assert write(loaded[0], ptr(back), back.size, ctypes.byref(got)) == 0 and bytes(back) == bytes(buf)
            lib.bh_params_free(loaded.pop())
        print(json.dumps(rec), flush=True)
        del params
    ctx.close()


if __name__ == "__main__":
    main()
