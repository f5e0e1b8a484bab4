"""Crafted proof encodings for the verifiers' Proof::read (groth16/mod.rs:50-103): each case replaces
one point (A, B or C) of a valid 192-byte proof by an encoding that the decoder must reject with a
given status, or that is well-formed but makes the proof invalid.  Built from the golden proofs and
tests/golden/subgroup.json; shared by tests/test_proof_cases_cpu.py (the host verifier, the
yardstick) and tests/test_gpu_verify_device.py (the device decoder against it).  Not a test module."""
import json
import os

from oracle import bls12_381 as bls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, R = bls.P, bls.R
F2 = bls.Fp2Ops

OK, INVALID_ARGUMENT, INVALID_ENCODING, NOT_IN_SUBGROUP = 0, 10, 11, 14
SLOTS = {"A": (0, 48), "B": (48, 144), "C": (144, 192)}


def golden_batches():
    """{params bytes: [(proof bytes, public inputs without ONE), ...]} of tests/golden/golden.json"""
    with open(os.path.join(ROOT, "tests", "golden", "golden.json")) as f:
        proofs = json.load(f)["proofs"]
    by_vk = {}
    for fx in proofs:
        public = [int(x, 16) for x in fx["inputs"]][1:]  # input 0 is ONE (prover.rs:202-204)
        by_vk.setdefault(bytes.fromhex(fx["params"]), []).append((bytes.fromhex(fx["proof"]), public))
    return by_vk


def _is_square_fp(a):
    return a % P == 0 or pow(a, (P - 1) // 2, P) == 1


def _is_square_fp2(a):
    return _is_square_fp((a[0] * a[0] + a[1] * a[1]) % P)  # a square iff its norm is one in Fp


def _compressed_x(slot, x, sign):
    """the compressed encoding of abscissa x (an int, or (c0, c1) for B) with the given sign flag"""
    body = bytearray(x.to_bytes(48, "big") if slot != "B" else x[1].to_bytes(48, "big") + x[0].to_bytes(48, "big"))
    body[0] |= 0x80 | (0x20 if sign else 0)
    return bytes(body)


def non_residue_x(slot):
    """the first x = 1, 2, ... (x = (x0, 1) over Fp2, as tests/golden/make_subgroup.py scans) with
    x^3 + b not a square"""
    x0 = 1
    while True:
        if slot != "B":
            if not _is_square_fp((x0 ** 3 + 4) % P):
                return x0
        else:
            x = (x0, 1)
            if not _is_square_fp2(F2.add(F2.mul(F2.sqr(x), x), (4, 4))):
                return x
        x0 += 1


def off_subgroup(slot):
    """the on-curve point outside the order-r subgroup of tests/golden/subgroup.json"""
    with open(os.path.join(ROOT, "tests", "golden", "subgroup.json")) as f:
        fx = json.load(f)
    if slot != "B":
        ok, pt = bls.g1_from_uncompressed(bytes.fromhex(fx["g1_off_subgroup"]), checked=False)
    else:
        ok, pt = bls.g2_from_uncompressed(bytes.fromhex(fx["g2_off_subgroup"]), checked=False)
    assert ok
    return pt


def point_cases(slot, original):
    """[(name, encoding of the slot's length, status)]: the replacements for one point; status 0
    means well-formed (the proof then fails to verify)."""
    n = len(original)
    assert n == SLOTS[slot][1] - SLOTS[slot][0]
    out = []

    def put(name, enc, status):
        assert len(enc) == n
        out.append((f"{slot}:{name}", bytes(enc), status))

    e = bytearray(original)
    e[0] &= 0x7F
    put("compression_flag_cleared", e, INVALID_ENCODING)
    put("infinity_zero_payload", bytes([0xC0]) + bytes(n - 1), INVALID_ENCODING)
    e = bytearray(original)
    e[0] |= 0x40
    put("infinity_nonzero_payload", e, INVALID_ENCODING)
    tail = bytes(n - 48) if slot != "B" else original[48:]
    e = bytearray(P.to_bytes(48, "big") + tail)
    e[0] |= 0x80
    put("x_equals_p", e, INVALID_ENCODING)
    e = bytearray(((1 << 381) - 1).to_bytes(48, "big") + tail)
    e[0] |= 0x80
    put("x_all_ones", e, INVALID_ENCODING)
    if slot == "B":
        put("c0_equals_p", original[:48] + P.to_bytes(48, "big"), INVALID_ENCODING)
        e = bytearray(original)
        e[48] |= 0x80
        put("c0_top_bit_set", e, INVALID_ENCODING)
    put("non_residue", _compressed_x(slot, non_residue_x(slot), False), INVALID_ENCODING)
    pt = off_subgroup(slot)
    for sign in (False, True):
        put(f"off_subgroup_sign{int(sign)}", _compressed_x(slot, pt[0], sign), NOT_IN_SUBGROUP)
    e = bytearray(original)
    e[0] ^= 0x20
    put("sign_flag_flipped", e, OK)
    return out


def with_point(proof, slot, enc):
    lo, hi = SLOTS[slot]
    return proof[:lo] + enc + proof[hi:]


def proof_cases(proof):
    """[(name, 192-byte proof, status)] over A, B and C of one valid proof"""
    out = []
    for slot, (lo, hi) in SLOTS.items():
        for name, enc, status in point_cases(slot, proof[lo:hi]):
            out.append((name, with_point(proof, slot, enc), status))
    return out


def words(values):
    """ints -> flat list of 4 little-endian u64 words each, NOT reduced (values below 2^256)"""
    return [(int(v) >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for v in values for k in range(4)]


def call_batch(fn, vk_bytes, proofs, inputs, zs, num_inputs=None, ctx=None):
    """bh_verify_batch / bh_verify_batch_device on raw words -> (status, valid).  zs and inputs are
    passed as given (a value >= r reaches the library); num_inputs defaults to len(inputs[0])."""
    import ctypes

    import numpy as np
    k = len(proofs)
    vk = np.frombuffer(bytes(vk_bytes), dtype=np.uint8)
    pf = np.frombuffer(b"".join(proofs) or b"\0", dtype=np.uint8)
    if num_inputs is None:
        num_inputs = len(inputs[0]) if k else 0
    ins = np.array(words([x for row in inputs for x in row]) or [0] * 4, dtype=np.uint64)
    z = np.array(words(zs) or [0] * 4, dtype=np.uint64)
    ok = ctypes.c_int(-1)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    args = [p(vk), vk.size, p(pf), p(ins), num_inputs, k, p(z), ctypes.byref(ok)]
    if ctx is not None:
        args.insert(0, ctx.h)
    return int(fn(*args)), ok.value
