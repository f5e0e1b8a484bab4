"""The proof scheduler's policy on the host (csrc/proof_schedule.h): which multiexps are large,
the stream of every sort, accumulation and reduction tail, what each sort takes its entries from,
where H is enqueued, and the order of the host's enqueues -- computed by the library's own
proof_schedule() (bh_selftest_proof_schedule), the function compute_msms' executor walks.  The
cases pin the schedule of every entry point (resident witness, serial, batch lane, bh_prove,
distributed H, device public inputs); the properties hold for random inputs too.  No GPU."""
import ctypes
import os
import random

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL_JOB = 4096
MAIN, SMALL, SORT, H, LANE3, TAIL0 = 0, 1, 2, 3, 4, 5
OP_H, OP_SORT, OP_ACC, OP_TAIL, MARK_ACC0, MARK_SORTS, HANDOFF = range(7)
REAL, COPY, DERIVE = 0, 1, 2
REL_NONE, REL_SAME, REL_DERIVABLE = 0, 1, 2
FLAGS = ["serial", "borrowed_streams", "cu_masked", "host_in", "uploading", "distributed"]


@pytest.fixture(scope="module")
def lib():
    lib = ctypes.CDLL(os.path.join(ROOT, "bellman-mpc_amd", "bellman_hip", "libbellman_hip.so"))
    f = lib.bh_selftest_proof_schedule
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint8), ctypes.c_uint,
                  ctypes.POINTER(ctypes.c_int64), ctypes.c_size_t]
    return lib


def schedule(lib, jobs, rel, **flags):
    """jobs: 8 dicts (len, used, W, is_h, g2); rel: {(i, j): REL_*}, what j's sort can take from i's."""
    assert set(flags) <= set(FLAGS)
    jw = (ctypes.c_uint64 * 40)(*[int(j[k]) for j in jobs for k in ("len", "used", "W", "is_h", "g2")])
    rw = (ctypes.c_uint8 * 64)()
    for (i, j), r in rel.items():
        rw[8 * i + j] = r
    bits = sum(1 << b for b, name in enumerate(FLAGS) if flags.get(name))
    out = (ctypes.c_int64 * 512)()
    n = lib.bh_selftest_proof_schedule(jw, rw, bits, out, 512)
    assert n >= 23
    w = list(out[:n])
    s = {"big": w[1:1 + w[0]], "small": w[10:10 + w[9]], "h_first": bool(w[18]), "first_own": bool(w[19]),
         "multi_lane": bool(w[20]), "wait_j": w[21]}
    assert n == 23 + 9 * w[22]
    names = ["op", "job", "stream", "kind", "src", "pre", "wait_h", "wait_sorted", "slot"]
    s["steps"] = [dict(zip(names, w[23 + 9 * i:32 + 9 * i])) for i in range(w[22])]
    return s


def proof_jobs(n=1 << 20, aux=None, h=None, inputs=0, W=13):
    """Job numbering: 0 b_g2_aux, 1 b_g1_aux, 2 l, 3 a_aux, 4 h, 5-7 the public-input multiexps;
    used = (1/2, 1/2, 1, 1/2, 1) n for jobs 0 to 4."""
    aux = n if aux is None else aux
    h = n if h is None else h
    mk = lambda ln, used, is_h=False, g2=False: dict(len=ln, used=used, W=W, is_h=is_h, g2=g2)
    return [mk(aux, n // 2, g2=True), mk(aux, n // 2), mk(aux, n), mk(aux, n // 2), mk(h, n, is_h=True),
            mk(inputs, inputs), mk(inputs, inputs), mk(inputs, inputs, g2=True)]


# job 1 has the same digits as job 0, job 3 is derivable from job 2 -- and, as the prover finds them,
# the b_aux ones from l too, and among the public-input ones b_g1's = b_g2's, derivable from a's
REL = {(0, 1): REL_SAME, (1, 0): REL_SAME, (2, 3): REL_DERIVABLE, (2, 0): REL_DERIVABLE, (2, 1): REL_DERIVABLE,
       (6, 7): REL_SAME, (7, 6): REL_SAME, (5, 6): REL_DERIVABLE, (5, 7): REL_DERIVABLE}


def brief(s):
    """The enqueue steps as short tuples: ("H",), ("sort", j, stream, kind, src), ("acc", j, stream),
    ("tail", j, stream); the host's marks left out."""
    out = []
    for t in s["steps"]:
        if t["op"] == OP_H:
            out.append(("H", t["stream"]))
        elif t["op"] == OP_SORT:
            out.append(("sort", t["job"], t["stream"], t["kind"], t["src"]))
        elif t["op"] == OP_ACC:
            out.append(("acc", t["job"], t["stream"]))
        elif t["op"] == OP_TAIL:
            out.append(("tail", t["job"], t["stream"]))
    return out


def check_properties(s, jobs, rel, flags):
    steps = s["steps"]
    on_device = [j for j in range(8) if jobs[j]["len"] and not (flags.get("host_in") and j >= 5)]
    assert sorted(s["big"] + s["small"]) == on_device
    pos = {}
    for i, t in enumerate(steps):
        if t["op"] in (OP_SORT, OP_ACC, OP_TAIL):
            assert (t["op"], t["job"]) not in pos, "a multiexp's stage enqueued twice"
            pos[(t["op"], t["job"])] = i
    # every non-empty multiexp that is not on the host: exactly once in each of sort, acc and tail
    assert sorted(pos) == sorted((op, j) for op in (OP_SORT, OP_ACC, OP_TAIL) for j in on_device)
    h_steps = [i for i, t in enumerate(steps) if t["op"] == OP_H]
    assert len(h_steps) == 1
    for j in on_device:
        srt = steps[pos[(OP_SORT, j)]]
        assert pos[(OP_SORT, j)] < pos[(OP_ACC, j)] < pos[(OP_TAIL, j)]
        if srt["kind"] == REAL:
            assert srt["src"] == -1
        else:
            # a copy's or derivation's source has its own (real or derived) sort earlier
            src = srt["src"]
            assert rel.get((src, j)) == (REL_SAME if srt["kind"] == COPY else REL_DERIVABLE)
            assert pos[(OP_SORT, src)] < pos[(OP_SORT, j)]
            assert steps[pos[(OP_SORT, src)]]["kind"] != COPY
        if jobs[j]["is_h"]:
            assert h_steps[0] < pos[(OP_SORT, j)]
            assert srt["wait_h"] == int(bool(flags.get("distributed")))
    if flags.get("serial"):
        assert all(t["stream"] == MAIN for t in steps)
    # the large tails come last, in accumulation order, each with its own done event
    tails = [t for t in steps if t["op"] == OP_TAIL and t["slot"] >= 0]
    assert [t["job"] for t in tails] == s["big"] and [t["slot"] for t in tails] == list(range(len(tails)))
    assert [t["op"] for t in steps[len(steps) - len(tails) - 1:]] == [HANDOFF] + [OP_TAIL] * len(tails)
    if s["big"]:
        first = steps[pos[(OP_ACC, s["big"][0])]]
        assert first["wait_sorted"] == s["wait_j"] and pos[(OP_SORT, s["wait_j"])] < pos[(OP_ACC, s["big"][0])]


CASE1 = dict(host_in=True, cu_masked=True)
CASE1_STEPS = [
    ("H", H),
    ("sort", 0, SORT, REAL, -1), ("sort", 1, SORT, COPY, 0),
    ("acc", 0, SMALL), ("acc", 1, MAIN),
    ("sort", 2, SORT, REAL, -1), ("sort", 3, SORT, DERIVE, 2), ("sort", 4, H, REAL, -1),
    # lane loads in units of n W: (1.375, 0.5, 0) -> l on lane 3 -> (1.375, 0.5, 1) -> a_aux on main
    # -> (1.375, 1, 1) -> h: ties go to the lower index (strict <), main
    ("acc", 2, LANE3), ("acc", 3, MAIN), ("acc", 4, MAIN),
    # the G2 tail behind its accumulation (nothing later is queued there), the last tail on its
    # accumulation's lane, the others on the tail streams
    ("tail", 0, SMALL), ("tail", 1, TAIL0 + 1), ("tail", 2, TAIL0 + 2), ("tail", 3, TAIL0 + 3), ("tail", 4, MAIN),
]


def test_case1_resident_witness_one_gpu(lib):
    jobs = proof_jobs()
    s = schedule(lib, jobs, REL, **CASE1)
    assert s["big"] == [0, 1, 2, 3, 4] and s["small"] == []
    assert s["h_first"] and s["first_own"] and s["multi_lane"]
    assert s["wait_j"] == 0  # the trailing copy (sort 1) is not waited for
    assert brief(s) == CASE1_STEPS
    assert [t["pre"] for t in s["steps"] if t["op"] == OP_SORT] == [1, 1, 0, 0, 0]
    # the host's marks: after the two early accumulations, after the sorts
    ops = [t["op"] for t in s["steps"]]
    assert ops.index(MARK_ACC0) == 5 and ops.index(MARK_SORTS) == 9
    check_properties(s, jobs, REL, CASE1)


def test_case2_serial(lib):
    jobs = proof_jobs()
    flags = dict(CASE1, serial=True)
    s = schedule(lib, jobs, REL, **flags)
    assert not s["first_own"] and not s["multi_lane"] and s["h_first"]
    assert brief(s) == [
        ("H", MAIN), ("sort", 0, MAIN, REAL, -1), ("sort", 1, MAIN, COPY, 0),
        ("acc", 0, MAIN),  # not followed early by acc 1
        ("sort", 2, MAIN, REAL, -1), ("sort", 3, MAIN, DERIVE, 2), ("sort", 4, MAIN, REAL, -1),
        ("acc", 1, MAIN), ("acc", 2, MAIN), ("acc", 3, MAIN), ("acc", 4, MAIN),
    ] + [("tail", q, MAIN) for q in range(5)]
    check_properties(s, jobs, REL, flags)


def test_case3_batch_lane(lib):
    jobs = proof_jobs()
    flags = dict(CASE1, borrowed_streams=True)
    s = schedule(lib, jobs, REL, **flags)
    assert s["first_own"] and not s["multi_lane"]
    want = list(CASE1_STEPS)
    want[8:11] = [("acc", 2, MAIN), ("acc", 3, MAIN), ("acc", 4, MAIN)]
    # neither the G2 override nor the last-tail override applies
    want[11:] = [("tail", q, TAIL0 + q % 5) for q in range(5)]
    assert brief(s) == want
    check_properties(s, jobs, REL, flags)


def test_case4_uploading(lib):
    jobs = proof_jobs()
    flags = dict(CASE1, uploading=True)
    s = schedule(lib, jobs, REL, **flags)
    assert not s["h_first"] and s["multi_lane"]
    want = [x for x in CASE1_STEPS if x != ("H", H) and x[:2] != ("sort", 4)]
    k = want.index(("acc", 4, MAIN))
    want[k:k] = [("H", H), ("sort", 4, H, REAL, -1)]
    assert brief(s) == want
    check_properties(s, jobs, REL, flags)


def test_case5_distributed(lib):
    jobs = proof_jobs()
    flags = dict(CASE1, distributed=True)
    s = schedule(lib, jobs, REL, **flags)
    assert s["h_first"]
    want = [("sort", 4, SORT, REAL, -1) if x[:2] == ("sort", 4) else x for x in CASE1_STEPS]
    assert brief(s) == want
    h_sort = [t for t in s["steps"] if t["op"] == OP_SORT and t["job"] == 4][0]
    assert h_sort["wait_h"] == 1  # behind a wait on the H-done event
    assert [t["wait_h"] for t in s["steps"] if t["op"] == OP_SORT and t["job"] != 4] == [0] * 4
    check_properties(s, jobs, REL, flags)


def test_case6_public_inputs_on_the_device(lib):
    jobs = proof_jobs(inputs=3)
    flags = dict(cu_masked=True)
    s = schedule(lib, jobs, REL, **flags)
    assert s["big"] == [0, 1, 2, 3, 4] and s["small"] == [5, 6, 7]
    assert not s["first_own"] and not s["multi_lane"] and s["h_first"]
    small = []
    # (a derived sort is one of its own: b_g2_inputs copies b_g1_inputs')
    for j, kind, src in ((5, REAL, -1), (6, DERIVE, 5), (7, COPY, 6)):
        small += [("sort", j, SMALL, kind, src), ("acc", j, SMALL), ("tail", j, SMALL)]
    assert brief(s) == [
        ("H", H), ("sort", 0, SORT, REAL, -1), ("sort", 1, SORT, COPY, 0), ("acc", 0, MAIN),
        ("sort", 2, SORT, REAL, -1), ("sort", 3, SORT, DERIVE, 2), ("sort", 4, H, REAL, -1),
        ("acc", 1, MAIN), ("acc", 2, MAIN), ("acc", 3, MAIN), ("acc", 4, MAIN),
    ] + small + [("tail", q, TAIL0 + q % 5) for q in range(5)]
    check_properties(s, jobs, REL, flags)


def test_case7_uploading_h_is_the_only_large_multiexp(lib):
    jobs = proof_jobs(n=1 << 5, aux=31, h=31)
    flags = dict(CASE1, uploading=True)
    s = schedule(lib, jobs, REL, **flags)
    assert s["big"] == [4] and s["small"] == [0, 1, 2, 3]
    assert s["h_first"]  # h's sort is among the pre-sorts, despite uploading
    assert brief(s)[:3] == [("H", H), ("sort", 4, H, REAL, -1), ("acc", 4, MAIN)]
    assert s["steps"][1]["pre"] == 1
    check_properties(s, jobs, REL, flags)


def test_h_still_runs_without_a_large_h_job(lib):
    jobs = proof_jobs(h=0)
    for up in (False, True):
        flags = dict(CASE1, uploading=up)
        s = schedule(lib, jobs, REL, **flags)
        assert s["big"] == [0, 1, 2, 3]
        assert [t["op"] for t in s["steps"]].count(OP_H) == 1
        check_properties(s, jobs, REL, flags)


def test_properties_on_random_inputs(lib):
    rng = random.Random(20260219)
    lens = [0, 1, 63, SMALL_JOB - 1, SMALL_JOB, SMALL_JOB + 1, 1 << 19]
    for _ in range(400):
        jobs = proof_jobs(n=rng.choice([1 << 12, 1 << 20]))
        for j in jobs:
            j["len"] = rng.choice(lens)
            j["W"] = rng.choice([0, 13, 16, 22])
            j["used"] = rng.choice([0, j["len"], 1 << 20])
        # a random relation (only between non-empty multiexps, as the prover evaluates it)
        live = [j for j in range(8) if jobs[j]["len"]]
        rel = {}
        for i in live:
            for j in live:
                if i != j and rng.random() < 0.3:
                    rel[(i, j)] = rng.choice([REL_SAME, REL_DERIVABLE])
        flags = {name: rng.random() < 0.5 for name in FLAGS}
        s = schedule(lib, jobs, rel, **flags)
        assert s["big"] == [j for j in live if not (flags["host_in"] and j >= 5)
                            and (jobs[j]["len"] >= SMALL_JOB or jobs[j]["is_h"])]
        check_properties(s, jobs, rel, flags)
