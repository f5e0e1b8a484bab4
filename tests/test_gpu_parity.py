"""GPU parity: the HIP path (through the C ABI) against the oracle's committed
golden vectors and live oracle runs on the same seeded inputs.  Bit-exact for
every integer/group result."""
import hashlib
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


def _bh():
    import bellman_hip as bh
    return bh


def _bases(ctx, group, hexes):
    bh = _bh()
    return bh.Bases(ctx, group, b"".join(bytes.fromhex(h) for h in hexes))


def _run_cases(ctx, group, data):
    bh = _bh()
    bases = _bases(ctx, group, data["bases"])
    assert len(bases) == len(data["bases"])
    for case in data["cases"]:
        exps = [int(x, 16) for x in case["exps"]]
        dens = None if case["density"] is None else [c == "1" for c in case["density"]]
        for mont in (False, True):
            try:
                got = bh.multiexp(ctx, bases, case["offset"], dens, exps, montgomery=mont)
                assert "point" in case, f"{case['note']}: expected error {case.get('error')}"
                assert got.hex() == case["point"], case["note"]
            except bh.SynthesisError as e:
                assert case.get("error") == e.code, (case["note"], e)


def test_srs_roundtrip(ctx, golden):
    bh = _bh()
    b = _bases(ctx, bh.BH_G1, golden["msm_g1"]["bases"][:8])
    for i in range(8):
        assert b.get(i).hex() == golden["msm_g1"]["bases"][i]
    b2 = _bases(ctx, bh.BH_G2, golden["msm_g2"]["bases"][:4])
    for i in range(4):
        assert b2.get(i).hex() == golden["msm_g2"]["bases"][i]


def test_srs_rejects_bad_points(ctx, golden):
    bh = _bh()
    raw = bytearray(bytes.fromhex(golden["msm_g1"]["bases"][0]))
    raw[-1] ^= 1  # off the curve
    with pytest.raises(bh.SynthesisError) as e:
        bh.Bases(ctx, bh.BH_G1, bytes(raw), checked=True)
    assert e.value.code == 12
    bh.Bases(ctx, bh.BH_G1, bytes(raw), checked=False)  # unchecked read accepts it
    big = bytearray(96)
    big[0] = 0x1F
    big[1:48] = b"\xff" * 47  # x >= p
    with pytest.raises(bh.SynthesisError):
        bh.Bases(ctx, bh.BH_G1, bytes(big), checked=False)
    # G2: the same off-curve rule over Fp2 ...
    from oracle import bls12_381 as bls
    good2 = bytes.fromhex(golden["msm_g2"]["bases"][0])
    raw2 = _off_curve(bh.BH_G2, good2)
    with pytest.raises(bh.SynthesisError) as e:
        bh.Bases(ctx, bh.BH_G2, raw2, checked=True)
    assert e.value.code == 12
    bh.Bases(ctx, bh.BH_G2, raw2, checked=False)
    # ... and a component >= p in any of the four 48-byte slots (x.c1, x.c0, y.c1, y.c0) is an
    # invalid encoding even unchecked (p's top byte 0x1a leaves slot 0's flag bits clear)
    for slot in range(4):
        big2 = bytearray(good2)
        big2[48 * slot:48 * slot + 48] = bls.P.to_bytes(48, "big")
        with pytest.raises(bh.SynthesisError) as e:
            bh.Bases(ctx, bh.BH_G2, bytes(big2), checked=False)
        assert e.value.code == 11, slot


def _group_bases(golden, group):
    """(wire bytes per point, the golden bases' encodings, the oracle's unchecked decoder and curve)"""
    from oracle import bls12_381 as bls
    if group == _bh().BH_G1:
        return 96, [bytes.fromhex(h) for h in golden["msm_g1"]["bases"]], bls.g1_from_uncompressed, bls.G1
    return 192, [bytes.fromhex(h) for h in golden["msm_g2"]["bases"]], bls.g2_from_uncompressed, bls.G2


def _off_curve(group, enc):
    """enc with the low bit of its last byte (y, or y.c0) flipped: still a valid encoding, every
    component < p, no longer on the curve (checked here on the CPU)"""
    from oracle import bls12_381 as bls
    dec, curve = (bls.g1_from_uncompressed, bls.G1) if group == _bh().BH_G1 else (bls.g2_from_uncompressed, bls.G2)
    ok, good = dec(enc, checked=False)
    assert ok and curve.on_curve_affine(good)
    raw = bytearray(enc)
    raw[-1] ^= 1
    ok, pt = dec(bytes(raw), checked=False)  # ok: flags clear, every component < p
    assert ok and pt is not None and not curve.on_curve_affine(pt)
    return bytes(raw)


@pytest.mark.parametrize("g2", [False, True])
def test_srs_checks_at_a_block_edge_and_skip_identities(ctx, golden, g2):
    """257 points: the conversion and check kernels run 256 threads per block, so index 255 is a
    block's last thread and 256 the only live thread of the next.  An off-curve point at either is
    found; identity encodings (0x40, then zeros) at 0 and 256 pass the checked read, are skipped by
    the curve check and come back as the identity; their neighbours round-trip."""
    bh = _bh()
    group = bh.BH_G2 if g2 else bh.BH_G1
    width, encs, dec, curve = _group_bases(golden, group)
    pts = [encs[i % len(encs)] for i in range(257)]
    for i in (1, 255, 256):
        ok, pt = dec(pts[i], checked=False)
        assert ok and curve.on_curve_affine(pt)
    for at in (255, 256):
        bad = list(pts)
        bad[at] = _off_curve(group, pts[at])
        with pytest.raises(bh.SynthesisError) as e:
            bh.Bases(ctx, group, b"".join(bad), checked=True)
        assert e.value.code == 12, at
    identity = bytes([0x40]) + bytes(width - 1)
    withid = list(pts)
    withid[0] = withid[256] = identity
    b = bh.Bases(ctx, group, b"".join(withid), checked=True)
    assert len(b) == 257
    for i in (0, 256):
        assert b.get(i) == identity
    for i in (1, 255):
        assert b.get(i) == pts[i]


@pytest.mark.parametrize("g2", [False, True])
def test_srs_of_one_identity(ctx, g2):
    bh = _bh()
    group = bh.BH_G2 if g2 else bh.BH_G1
    identity = bytes([0x40]) + bytes((192 if g2 else 96) - 1)
    for checked in (True, False):
        b = bh.Bases(ctx, group, identity, checked=checked)
        assert len(b) == 1 and b.get(0) == identity


def test_msm_g1_golden(ctx, golden):
    _run_cases(ctx, _bh().BH_G1, golden["msm_g1"])


def test_msm_g2_golden(ctx, golden):
    _run_cases(ctx, _bh().BH_G2, golden["msm_g2"])


@pytest.mark.parametrize("c", [4, 7, 11, 16])
def test_msm_window_independent(ctx, golden, c):
    """Device window size never changes the result (forced c)."""
    bh = _bh()
    data = golden["msm_g1"]
    bases = _bases(ctx, bh.BH_G1, data["bases"])
    case = [k for k in data["cases"] if k["note"].startswith("random n=160")][0]
    exps = [int(x, 16) for x in case["exps"]]
    ctx.set_window(c)
    try:
        assert bh.multiexp(ctx, bases, 0, None, exps).hex() == case["point"]
    finally:
        ctx.set_window(0)


def test_msm_identity_base_semantics(ctx, golden):
    """Source::next rejects an identity base (multiexp.rs:63-65) only when consumed
    with a non-zero exponent; compare with the oracle restatement."""
    bh = _bh()
    from oracle import bellman as bm
    from oracle import bls12_381 as bls
    hexes = list(golden["msm_g1"]["bases"][:40])
    ident = "40" + "00" * 95
    hexes[5] = ident
    bases = _bases(ctx, bh.BH_G1, hexes)
    pts = []
    for h in hexes:
        ok, p = bls.g1_from_uncompressed(bytes.fromhex(h), checked=False)
        pts.append(p)
    rng = random.Random(9)
    E = bm.BLS12_381
    for exps in ([rng.randrange(R) for _ in range(40)],
                 [0 if i == 5 else rng.randrange(R) for i in range(40)],
                 [1 if i == 5 else rng.randrange(R) for i in range(40)]):
        try:
            want = ("point", bls.g1_to_uncompressed(E.G1.to_affine(bm.multiexp(E, E.G1, pts, 0, None, exps))).hex())
        except bm.SynthesisError as e:
            want = ("error", e.code)
        try:
            got = ("point", bh.multiexp(ctx, bases, 0, None, exps).hex())
        except bh.SynthesisError as e:
            got = ("error", e.code)
        assert got == want


@pytest.mark.parametrize("g2", [False, True])
def test_msm_exceptional_additions_in_one_bucket(ctx, g2):
    """Equal and opposite bases under equal exponents land in one bucket per window.  Their order
    inside the bucket is decided by the sort's LDS atomics, not by this test, so which doublings
    and identities the accumulation meets is not chosen here (test_gpu_accumulate.py drives the
    accumulation kernels on an ordered entry list for that); the reductions add equal partial
    sums, the case curve.cuh folds into the full addition's own instruction stream.  Compared
    with the oracle's multiexp (multiexp.rs:159-281)."""
    bh = _bh()
    from oracle import bellman as bm
    from oracle import bls12_381 as bls
    E = bm.BLS12_381
    G = E.G2 if g2 else E.G1
    gen = bls.G2.generator() if g2 else bls.G1.generator()
    enc = bls.g2_to_uncompressed if g2 else bls.g1_to_uncompressed
    aff = lambda k: G.to_affine(G.mul(gen, k % R))
    P, N, Q = aff(11), aff(R - 11), aff(29)
    rng = random.Random(21)
    others = [aff(rng.randrange(1, R)) for _ in range(8)]
    pts = [P] * 24 + [N] * 24 + [Q] * 16 + others
    bases = bh.Bases(ctx, bh.BH_G2 if g2 else bh.BH_G1, b"".join(enc(p) for p in pts))
    e1, e2 = rng.randrange(R), rng.randrange(R)
    cases = [
        [e1] * 48 + [e2] * 16 + [rng.randrange(R) for _ in range(8)],     # 24P - 24P + 16 e2 Q + ...
        [e1] * 24 + [e2] * 24 + [e1] * 16 + [rng.randrange(R) for _ in range(8)],
        [e1] * 48 + [0] * 24,                                             # the exact identity
        [1] * 24 + [R - 1] * 24 + [2] * 16 + [0] * 8,                      # small digits, one bucket
    ]
    for exps in cases:
        want = enc(G.to_affine(bm.multiexp(E, G, pts, 0, None, exps)))
        assert bh.multiexp(ctx, bases, 0, None, exps) == want


def test_msm_density_mismatch(ctx, golden):
    bh = _bh()
    bases = _bases(ctx, bh.BH_G1, golden["msm_g1"]["bases"][:10])
    with pytest.raises(bh.DensitySizeMismatch):
        bh.multiexp(ctx, bases, 0, [True] * 5, [1] * 10)


def test_msm_medium_vs_oracle_naive(ctx):
    """n = 2^12 random bases / scalars (dense 255-bit) vs the oracle's naive sum."""
    bh = _bh()
    from oracle import bls12_381 as bls
    rng = random.Random(12)
    G = bls.G1
    n = 4096
    # bases P_i = [k_i] G built incrementally to keep the oracle fast
    step = G.mul(G.generator(), rng.randrange(1, R))
    acc = G.mul(G.generator(), rng.randrange(1, R))
    pts, enc = [], []
    for i in range(n):
        acc = G.add(acc, step)
        a = G.to_affine(acc)
        pts.append(a)
        enc.append(bls.g1_to_uncompressed(a))
    bases = bh.Bases(ctx, bh.BH_G1, b"".join(enc))
    exps = [rng.randrange(R) for _ in range(n)]
    got = bh.multiexp(ctx, bases, 0, None, exps)
    # exact oracle value by linearity: P_i = B + (i+1) S with B = acc - n*S
    B = G.add(acc, G.neg(G.mul(step, n)))
    se = sum(exps) % R
    sie = sum((i + 1) * e for i, e in enumerate(exps)) % R
    want = G.to_affine(G.add(G.mul(B, se), G.mul(step, sie)))
    assert got.hex() == bls.g1_to_uncompressed(want).hex()


def test_domain_ops_golden(ctx, golden):
    bh = _bh()
    for case in golden["domain"]:
        coeffs = [int(x, 16) for x in case["coeffs"]]
        other = [int(x, 16) for x in case["other"]]
        for op, want in case["results"].items():
            d = bh.EvaluationDomain(ctx, coeffs)
            if op == "distribute_powers_12345":
                d.distribute_powers(12345)
            elif op in ("mul_assign", "sub_assign"):
                getattr(d, op)(bh.EvaluationDomain(ctx, other))
            else:
                getattr(d, op)()
            assert [format(v, "x") for v in d.into_coeffs()] == want, (case["log_m"], op)


@pytest.mark.parametrize("logm", [10, 12, 14])
def test_fft_roundtrip_and_linearity(ctx, logm):
    """Size-independent properties at larger sizes: ifft(fft(x)) = x, icoset(coset(x)) = x,
    fft linear, and fft of a delta is all-ones."""
    bh = _bh()
    rng = np.random.default_rng(logm)
    m = 1 << logm
    vals = [int(x) for x in rng.integers(0, 2**62, size=m)]
    d = bh.EvaluationDomain(ctx, vals)
    orig = d.coeffs.copy()
    d.fft(); d.ifft()
    assert np.array_equal(d.coeffs, orig)
    d.coset_fft(); d.icoset_fft()
    assert np.array_equal(d.coeffs, orig)
    delta = bh.EvaluationDomain(ctx, [1] + [0] * (m - 1))
    delta.fft()
    assert delta.into_coeffs() == [1] * m


@pytest.mark.parametrize("logm", [9, 11, 16])
def test_fft_full_range_and_extreme_values_equal_oracle(ctx, logm):
    """The NTT butterflies keep sums and differences limb-wise (carry-free) where they only feed
    a product, under limb and value bounds argued in csrc/ntt.hip: checked against the oracle's
    serial_fft (domain.rs:261-303) on full-range values and on the extremes that maximise limbs
    and values (r-1 everywhere, r-1 / 0 alternating, 2^255-ish patterns reduced mod r), over one
    pass (2^9: odd stage count, radix-2 first stage) and two passes (2^11, 2^16)."""
    bh = _bh()
    from oracle import bellman as bm
    E = bm.BLS12_381
    m = 1 << logm
    rng = np.random.default_rng(100 + logm)
    cases = {
        "random": [int.from_bytes(rng.bytes(32), "little") % R for _ in range(m)],
        "r-1": [R - 1] * m,
        "alternating": [(R - 1) if i % 2 == 0 else 0 for i in range(m)],
        "high": [((1 << 255) - 1 - i) % R for i in range(m)],
    }
    for name, vals in cases.items():
        for op in ("fft", "ifft", "coset_fft", "icoset_fft"):
            d = bh.EvaluationDomain(ctx, vals)
            getattr(d, op)()
            o = bm.EvaluationDomain(E, list(vals))
            getattr(o, op)()
            assert d.into_coeffs() == [int(x) for x in o.coeffs], (name, op, logm)


_ALL_FFTS = ("fft", "ifft", "coset_fft", "icoset_fft")


@pytest.mark.parametrize("logm,ops,names", [(13, _ALL_FFTS, ("random", "r-1")), (15, _ALL_FFTS, ("random", "r-1")),
                                            (17, ("fft", "ifft"), ("random",))])
def test_fft_pass_splits_equal_oracle(ctx, logm, ops, names):
    """The pass splits no other direct transform test visits (launch_ntt: 2^13 = [6, 7], 2^15 =
    [8, 7], 2^17 = [8, 9]; the odd pass runs a radix-2 stage first), element for element against
    the oracle's serial_fft, so that a wrong element there names the transform and not a proof."""
    bh = _bh()
    from oracle import bellman as bm
    E = bm.BLS12_381
    m = 1 << logm
    rng = np.random.default_rng(100 + logm)
    cases = {
        "random": [int.from_bytes(rng.bytes(32), "little") % R for _ in range(m)],
        "r-1": [R - 1] * m,
    }
    for name in names:
        for op in ops:
            d = bh.EvaluationDomain(ctx, cases[name])
            getattr(d, op)()
            o = bm.EvaluationDomain(E, list(cases[name]))
            getattr(o, op)()
            assert d.into_coeffs() == [int(x) for x in o.coeffs], (name, op, logm)


def test_compute_h_golden(ctx, golden):
    bh = _bh()
    g = golden["h_random"]
    a, b, c = ([int(x, 16) for x in g[k]] for k in "abc")
    assert [format(v, "x") for v in bh.compute_h(ctx, a, b, c)] == g["h"]


def _proof_from_fixture(ctx, fx):
    bh = _bh()
    params = bh.Parameters.read(ctx, bytes.fromhex(fx["params"]))

    class P:  # a completed ProvingAssignment
        pass
    p = P()
    p.a, p.b, p.c = ([int(x, 16) for x in fx[k]] for k in "abc")
    p.input_assignment = [int(x, 16) for x in fx["inputs"]]
    p.aux_assignment = [int(x, 16) for x in fx["aux"]]
    for k in ("a_aux_density", "b_input_density", "b_aux_density"):
        t = bh.DensityTracker()
        t.bv = [ch == "1" for ch in fx[k]]
        setattr(p, k, t)
    w = bh.Witness.from_assignment(ctx, p)
    return params, w


def test_proofs_golden(ctx, golden):
    bh = _bh()
    for fx in golden["proofs"]:
        params, w = _proof_from_fixture(ctx, fx)
        proof = bh.prove_witness(ctx, params, w, fx["r"], fx["s"])
        assert proof.hex() == fx["proof"], fx["name"]
        assert params.write().hex() == fx["params"], fx["name"]


def test_create_proof_host_synthesis(ctx, golden):
    """create_random_proof through the product's own host synthesis (prover.rs:158-204)."""
    bh = _bh()
    from oracle import circuits as cc
    fx = [f for f in golden["proofs"] if f["name"] == "mimc_chain_r15"][0]
    params = bh.Parameters.read(ctx, bytes.fromhex(fx["params"]))
    proof = bh.create_random_proof(ctx, cc.chain_circuit(R, 15), params)
    assert proof.hex() == fx["proof"]


@pytest.mark.parametrize("name,rounds", [("mimc_chain_r7", 7), ("mimc_chain_r15", 15)])
def test_native_chain_params_and_witness(ctx, golden, name, rounds):
    """Native C++ synthesis + device CRS generation reproduce the oracle's
    Parameters bytes and proof bytes exactly."""
    bh = _bh()
    fx = [f for f in golden["proofs"] if f["name"] == name][0]
    params = bh.Parameters.chain(ctx, rounds)
    assert params.write().hex() == fx["params"]
    w = bh.Witness.chain(ctx, rounds)
    assert bh.prove_witness(ctx, params, w, 27134, 17146).hex() == fx["proof"]


@pytest.mark.parametrize("nshards", [2, 3, 8])
def test_sharded_partials_combine(ctx, golden, nshards):
    """The multi-GPU decomposition on one device: per-shard partial multiexps
    (bh_prove_witness_partial) summed by bh_proof_from_partials give the proof."""
    bh = _bh()
    fx = [f for f in golden["proofs"] if f["name"] == "mimc_chain_r15"][0]
    params = bh.Parameters.chain(ctx, 15)
    w = bh.Witness.chain(ctx, 15)
    parts = b"".join(bh.prove_witness_partial(ctx, params, w, k, nshards) for k in range(nshards))
    assert bh.proof_from_partials(params.vk_bytes(), parts, nshards, 27134, 17146).hex() == fx["proof"]


@pytest.mark.parametrize("logc", [17, 20, 22])
def test_window_tables_match_plain_windows(ctx, logc):
    """SRS window tables (every digit window sharing one bucket set, larger c) give
    byte-identical proofs to plain per-window buckets, on one device and sharded over
    two (whose smaller shards pick a different c, so the tables are rebuilt).  At 2^22
    (BASELINE.json configs[2]) this is the benchmark's own proof."""
    bh = _bh()
    rounds = (1 << (logc - 1)) - 1
    params = bh.Parameters.chain(ctx, rounds)
    w = bh.Witness.chain(ctx, rounds)
    ctx.set_tables(False)
    try:
        plain = bh.prove_witness(ctx, params, w, 27134, 17146)
    finally:
        ctx.set_tables(True)
    params.prepare(w)
    assert bh.prove_witness(ctx, params, w, 27134, 17146) == plain
    parts = b"".join(bh.prove_witness_partial(ctx, params, w, k, 2) for k in range(2))
    assert bh.proof_from_partials(params.vk_bytes(), parts, 2, 27134, 17146) == plain
    if logc == 22:
        # the benchmark's own proof (C3) equals the oracle port's proof of the same CRS and
        # witness, recorded in tests/golden/port_proofs.json by tools/cpu_baseline_full.py
        # --fixture (prover.rs:315-349 output)
        fx = _port_proof(22)
        assert hashlib.sha256(params.write()).hexdigest() == fx["params_sha256"]
        assert plain.hex() == fx["proof_port"]
        # the drop-in entry point at the headline size: bh_prove from host buffers (the
        # ProvingAssignment in bls12_381's layouts) gives the same bytes
        asg = bh.chain_assignment(rounds)
        assert bh.prove(ctx, params, asg, 27134, 17146).hex() == fx["proof_port"]


def test_checked_load_rejects_points_outside_subgroup(ctx):
    """Parameters::read(checked) / from_uncompressed reject on-curve points that are not
    torsion-free (groth16/mod.rs:292-400); the unchecked read accepts them.  Fixture:
    tests/golden/make_subgroup.py."""
    import json
    import os
    bh = _bh()
    fx = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "subgroup.json")))
    for group, key in ((bh.BH_G1, "g1_off_subgroup"), (bh.BH_G2, "g2_off_subgroup")):
        raw = bytes.fromhex(fx[key])
        with pytest.raises(bh.SynthesisError) as e:
            bh.Bases(ctx, group, raw, checked=True)
        assert e.value.code == 14
        bh.Bases(ctx, group, raw, checked=False)
    # a valid subgroup point passes the checked path
    g = bytes.fromhex(_golden_first_g1())
    bh.Bases(ctx, bh.BH_G1, g, checked=True)


def _port_proof(logc, required=True):
    """tests/golden/port_proofs.json: the oracle C++ port's full-size proofs (MiMC chain, seed 7,
    preimage seed 8, r = 27134, s = 17146) with the SHA-256 of the Parameters they were proved
    with; written by tools/cpu_baseline_full.py --fixture on the GPU box."""
    import json
    import os
    path = os.path.join(os.path.dirname(__file__), "golden", "port_proofs.json")
    fx = json.load(open(path)) if os.path.exists(path) else {}
    if f"2^{logc}" not in fx:
        assert not required, f"{path} has no 2^{logc} entry"
        return None
    return fx[f"2^{logc}"]


def _golden_first_g1():
    import json
    import os
    return json.load(open(os.path.join(os.path.dirname(__file__), "golden", "golden.json")))["msm_g1"]["bases"][0]


def _params_vectors(raw):
    """Split Parameters::write bytes (groth16/mod.rs:260-290) -> dict of raw vectors."""
    import struct
    off = 96 + 96 + 192 + 192 + 96 + 192
    (n_ic,) = struct.unpack(">I", raw[off:off + 4])
    off += 4 + 96 * n_ic
    out = {}
    for name, size in (("h", 96), ("l", 96), ("a", 96), ("b_g1", 96), ("b_g2", 192)):
        (n,) = struct.unpack(">I", raw[off:off + 4])
        out[name] = raw[off + 4:off + 4 + n * size]
        off += 4 + n * size
    return out


def test_c2_msm_2p20_matches_bellman_port(ctx):
    """BASELINE.json configs[1] (C2): a 2^20-point G1 multiexp with dense uniform scalars,
    bit-exact against bellman's multiexp algorithm (the C++ port, oracle/cpu) at full size.
    Bases: the h query of a device-generated 2^21-constraint CRS ([tau^i Z(tau)/delta] G1)."""
    import sys
    import os
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import cpu_port
    bh = _bh()
    n = 1 << 20
    params = bh.Parameters.chain(ctx, (1 << 20) - 1)
    h = _params_vectors(params.write())["h"][:96 * n]
    rng = np.random.default_rng(20)
    ex = rng.integers(0, 1 << 63, size=(n, 4), dtype=np.uint64) * 2 + rng.integers(0, 2, size=(n, 4), dtype=np.uint64)
    ex[:, 3] %= np.uint64(0x73EDA753299D7D48)  # below r
    bases = bh.Bases(ctx, bh.BH_G1, h, checked=False)
    got = bh.multiexp(ctx, bases, 0, None, ex)
    want, _ = cpu_port.multiexp_g1(h, ex)
    assert got == want


def test_c5_distinct_witnesses_shared_params(ctx):
    """BASELINE.json configs[4] (C5) semantics: independent proofs of one circuit (shared
    Parameters) with distinct witnesses, each bit-exact with the oracle."""
    from oracle import bellman as bm
    from oracle import bls12_381 as bls
    from oracle import circuits as cc
    bh = _bh()
    E = bm.BLS12_381
    for rounds in (3, 15):
        oparams = bm.generate_random_parameters(E, cc.chain_circuit(bls.R, rounds, witness=False))
        params = bh.Parameters.chain(ctx, rounds)
        assert params.write() == bm.params_to_bytes(oparams)
        for ps in (100, 101, 102, 103):
            prover = bm.synthesize_for_proving(E, cc.chain_circuit(bls.R, rounds, preimage_seed=ps))
            want = bm.proof_to_bytes(bm.prove_from_assignment(E, prover, oparams, 27134, 17146))
            w = bh.Witness.chain(ctx, rounds, preimage_seed=ps)
            assert bh.prove_witness(ctx, params, w, 27134, 17146) == want, (rounds, ps)


def test_concurrent_contexts_in_threads(golden):
    """Throughput mode (C5): several contexts on one device proving at once from host
    threads (the ABI is thread-safe per context; ctypes releases the GIL) give the same
    bytes as the committed proof."""
    import threading
    bh = _bh()
    fx = [f for f in golden["proofs"] if f["name"] == "mimc_chain_r15"][0]
    results, errors = [], []

    def worker():
        try:
            c = bh.Context(0)
            p = bh.Parameters.chain(c, 15)
            w = bh.Witness.chain(c, 15)
            for _ in range(3):
                results.append(bh.prove_witness(c, p, w, 27134, 17146).hex())
            del p, w
            c.close()
        except Exception as e:  # pragma: no cover - reported below
            errors.append(repr(e))

    threads = [threading.Thread(target=worker) for _ in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert len(results) == 12 and set(results) == {fx["proof"]}


@pytest.mark.slow
def test_c4_2p24_sharded_8_ways_equals_single_device_proof():
    """BASELINE.json configs[3] (C4): a 2^24-constraint proof whose multiexps are split 8 ways
    by scalar range (bh_prove_witness_partial, the per-rank work of the multi-GPU path, run
    here shard after shard on one device) and recombined by bh_proof_from_partials equals
    the unsharded proof.  Both use SRS window tables sized for their shard (c differs)."""
    bh = _bh()
    c = bh.Context(0)
    try:
        rounds = (1 << 23) - 1
        params = bh.Parameters.chain(c, rounds)
        w = bh.Witness.chain(c, rounds)
        single = bh.prove_witness(c, params, w, 27134, 17146)
        # the proof is valid (verify_proof, verifier.rs:23-62, natively) for the chain's image ...
        public = bh.fr_from_mont(bh.chain_assignment(rounds)["inputs"])[1:]
        vk = params.vk_bytes()
        assert bh.verify_proof(vk, single, public)
        assert not bh.verify_proof(vk, single, [(public[0] + 1) % R])
        # ... and, where the oracle port has proved C4 (tests/golden/port_proofs.json), its proof
        fx = _port_proof(24, required=False)
        if fx is not None:
            assert single.hex() == fx["proof_port"]
        params.prepare(w, 8)
        parts = b"".join(bh.prove_witness_partial(c, params, w, k, 8) for k in range(8))
        assert bh.proof_from_partials(params.vk_bytes(), parts, 8, 27134, 17146) == single
        # the same split with the H block distributed over the 8 (virtual) ranks
        parts = bh.prove_witness_partials_local(c, params, w, 8)
        assert bh.proof_from_partials(params.vk_bytes(), parts, 8, 27134, 17146) == single
        del params, w
    finally:
        c.close()


@pytest.mark.parametrize("logc", [10, 22])
def test_device_proof_verifies_with_pairing(ctx, logc):
    """The device proof of a MiMC chain -- at 2^22 constraints the benchmark's own proof
    (BASELINE.json configs[2]) -- is accepted by the oracle's restatement of verify_proof
    (verifier.rs:23-62, oracle/pairing.py) for the device-generated verifying key and the
    chain's public image, and rejected for a wrong image."""
    from oracle import bls12_381 as bls
    from oracle import circuits as cc
    from oracle import pairing as pr
    bh = _bh()
    rounds = (1 << (logc - 1)) - 1
    params = bh.Parameters.chain(ctx, rounds)
    w = bh.Witness.chain(ctx, rounds)
    params.prepare(w)
    proof = pr.proof_from_bytes(bh.prove_witness(ctx, params, w, 27134, 17146))
    vk_bytes = params.vk_bytes()
    vk = pr.vk_from_params_bytes(vk_bytes)
    xl, xr = cc.fr_stream(8, 2, bls.R)
    image = cc.mimc(xl, xr, cc.fr_stream(7, rounds, bls.R), bls.R)
    assert pr.verify_proof(vk, proof, [image])
    assert not pr.verify_proof(vk, proof, [(image + 1) % bls.R])


@pytest.mark.parametrize("logc,nshards", [(10, 2), (10, 4), (12, 8), (14, 16), (14, 4), (16, 8)])
def test_distributed_h_partials_equal_single_proof(ctx, logc, nshards):
    """The multi-GPU algorithm with the H block distributed (dist_h.h: per NTT a local
    m/N-point NTT + one all-to-all + N-point DFTs; each rank's h multiexp over the strided
    coefficient set it ends with), run with N virtual ranks on one device: the recombined
    proof equals the single-device proof byte for byte."""
    bh = _bh()
    rounds = (1 << (logc - 1)) - 1
    params = bh.Parameters.chain(ctx, rounds)
    w = bh.Witness.chain(ctx, rounds)
    single = bh.prove_witness(ctx, params, w, 27134, 17146)
    parts = bh.prove_witness_partials_local(ctx, params, w, nshards)
    assert bh.proof_from_partials(params.vk_bytes(), parts, nshards, 27134, 17146) == single


def test_polynomial_arith_fft_product_equals_naive(ctx):
    """domain.rs:378-420 (polynomial_arith): fft(a) * fft(b), then ifft, equals the naive
    product; lengths sampled from the reference's 0..70 x 0..70 sweep, incl. empty."""
    bh = _bh()
    rng = random.Random(378)
    lens = [0, 1, 2, 3, 5, 8, 13, 31, 32, 33, 64, 69]
    for la in lens:
        for lb in lens:
            a = [rng.randrange(R) for _ in range(la)]
            b = [rng.randrange(R) for _ in range(lb)]
            naive = [0] * (la + lb)
            for i, x in enumerate(a):
                for j, y in enumerate(b):
                    naive[i + j] = (naive[i + j] + x * y) % R
            da = bh.EvaluationDomain(ctx, a + [0] * lb)
            db = bh.EvaluationDomain(ctx, b + [0] * la)
            da.fft()
            db.fft()
            da.mul_assign(db)
            da.ifft()
            got = list(da.into_coeffs())
            assert got[: la + lb] == naive, (la, lb)
            assert all(v == 0 for v in got[la + lb:]), (la, lb)


@pytest.mark.parametrize("logm", range(0, 10))
def test_fft_composition(ctx, logm):
    """domain.rs:429-463 (fft_composition): ifft/fft, fft/ifft, icoset/coset and coset/icoset
    are identities on random full-width Fr vectors of length 2^0 .. 2^9."""
    bh = _bh()
    rng = random.Random(429 + logm)
    v = [rng.randrange(R) for _ in range(1 << logm)]
    d = bh.EvaluationDomain(ctx, v)
    for first, second in (("ifft", "fft"), ("fft", "ifft"), ("icoset_fft", "coset_fft"), ("coset_fft", "icoset_fft")):
        getattr(d, first)()
        getattr(d, second)()
        assert list(d.into_coeffs()) == v, (first, second)


@pytest.mark.parametrize("rounds", [15, 100, 5000, (1 << 15) - 1])
def test_bh_prove_from_host_buffers(ctx, golden, rounds):
    """bh_prove, the drop-in entry point: the ProvingAssignment as
    host buffers in bls12_381's layouts (a/b/c/assignments as 4-limb Montgomery Fr, densities
    as bitvec words) straight to the 192-byte proof.  Equals the golden proof (r15) and the
    device-resident-witness proof (2^16 constraints).  100 and 5000 rounds give 202 and 10002
    constraints, so the H block's domain (256, 16384) is zero-padded past the constraints (the
    raw upload's padding branch); those proofs also verify natively."""
    bh = _bh()
    params = bh.Parameters.chain(ctx, rounds)
    asg = bh.chain_assignment(rounds)
    proof = bh.prove(ctx, params, asg, 27134, 17146)
    if rounds == 15:
        fx = [f for f in golden["proofs"] if f["name"] == "mimc_chain_r15"][0]
        assert proof.hex() == fx["proof"]
    assert proof == bh.prove_witness(ctx, params, bh.Witness.chain(ctx, rounds), 27134, 17146)
    assert bh.prove(ctx, params, asg, 27134, 17146) == proof  # buffers reused
    if rounds in (100, 5000):
        nc = asg["a"].shape[0]
        assert nc & (nc - 1), "a constraint count that is not a power of two"
        public = bh.fr_from_mont(asg["inputs"])[1:]
        assert bh.verify_proof(params.vk_bytes(), proof, public)


def test_async_multiexp_waiters_equal_sequential(ctx, golden):
    """bh_multiexp_submit / bh_multiexp_wait (the Waiter seam, multiexp.rs:252-281 and
    multicore.rs:94-110): eight multiexps in flight at once from one thread, as create_proof
    keeps them (prover.rs:233-307), waited in reverse order, equal the sequential results;
    EOF / identity errors surface from wait() like the reference's."""
    bh = _bh()
    rng = random.Random(99)
    g1 = _bases(ctx, bh.BH_G1, golden["msm_g1"]["bases"])
    g2 = _bases(ctx, bh.BH_G2, golden["msm_g2"]["bases"])
    n1, n2 = len(golden["msm_g1"]["bases"]), len(golden["msm_g2"]["bases"])
    jobs = []
    for k in range(8):
        G, bases, nb = (bh.BH_G1, g1, n1) if k % 3 else (bh.BH_G2, g2, n2)
        n = rng.randrange(1, nb)
        dens = [rng.random() < 0.7 for _ in range(n)] if k % 2 else None
        exps = [rng.randrange(R) for _ in range(n)]
        jobs.append((bases, 0, dens, exps))
    waiters = [bh.multiexp_async(ctx, *j) for j in jobs]
    got = [w.wait() for w in reversed(waiters)][::-1]
    assert got == [bh.multiexp(ctx, *j) for j in jobs]
    # error semantics from the golden cases, deferred to wait()
    for case in golden["msm_g1"]["cases"]:
        if "error" not in case:
            continue
        exps = [int(x, 16) for x in case["exps"]]
        dens = None if case["density"] is None else [c == "1" for c in case["density"]]
        w = bh.multiexp_async(ctx, g1, case["offset"], dens, exps)
        with pytest.raises(bh.SynthesisError) as e:
            w.wait()
        assert e.value.code == case["error"]


def test_async_multiexp_outlives_destroyed_context(golden):
    """A Waiter whose context is destroyed before wait() is detached: wait() raises and touches
    nothing of the context (bh_ctx_destroy used to free the slots outstanding jobs
    pointed to).  A Waiter that goes out of scope unwaited is harmless too."""
    bh = _bh()
    c2 = bh.Context(0)
    g1 = _bases(c2, bh.BH_G1, golden["msm_g1"]["bases"])
    n = len(golden["msm_g1"]["bases"])
    exps = [(7 ** (i + 3)) % R for i in range(n)]
    want = bh.multiexp(c2, g1, 0, None, exps)
    done = bh.multiexp_async(c2, g1, 0, None, exps)
    assert done.wait() == want
    pending = [bh.multiexp_async(c2, g1, 0, None, exps) for _ in range(3)]
    dropped = bh.multiexp_async(c2, g1, 0, None, exps)
    del dropped  # never waited: __del__ waits it (after which the context's slots stay intact)
    c2.close()
    for w in pending:
        with pytest.raises(bh.SynthesisError):
            w.wait()


@pytest.mark.parametrize("logc,k,lanes", [(12, 5, 1), (12, 5, 2), (16, 6, 3), (20, 4, 2)])
def test_prove_batch_equals_single_proofs(ctx, logc, k, lanes):
    """Throughput mode (BASELINE.json configs[4], C5): independent proofs of distinct
    witnesses (preimage seeds 8 + i) sharing one Parameters, pipelined on `lanes` contexts of
    one device by bh_prove_batch, are each byte-equal to that witness's single proof (at
    2^20 constraints, the C5 proof size, too)."""
    bh = _bh()
    rounds = (1 << (logc - 1)) - 1
    params = bh.Parameters.chain(ctx, rounds)
    ws = [bh.Witness.chain(ctx, rounds, seed=7, preimage_seed=8 + i) for i in range(k)]
    got = bh.prove_batch(ctx, params, ws, 27134, 17146, lanes)
    want = [bh.prove_witness(ctx, params, w, 27134, 17146) for w in ws]
    assert got == want
    assert len(set(got)) == k


def test_msm_canonical_exponents_at_or_above_r(ctx, golden):
    """Exponent words >= r (k < 2^256) in the canonical format give k*P like the
    reference's 256-bit window walk does (multiexp.rs:159-250): (k mod r)*P."""
    bh = _bh()
    g1 = _bases(ctx, bh.BH_G1, golden["msm_g1"]["bases"][:40])
    rng = random.Random(5)
    ks = [rng.randrange(R) for _ in range(40)]
    big = [k + R if k + R < 1 << 256 else k for k in ks]
    big[0], ks[0] = R, 0
    big[1], ks[1] = (1 << 256) - 1, ((1 << 256) - 1) % R
    raw = np.array([[(k >> (64 * i)) & (2**64 - 1) for i in range(4)] for k in big], dtype=np.uint64)
    assert bh.multiexp(ctx, g1, 0, None, raw) == bh.multiexp(ctx, g1, 0, None, ks)


def test_c1_mimc322_device_params_and_proof(ctx):
    """C1 (BASELINE.json configs[0], mimc_mod.rs:6 MIMC_ROUNDS = 322, 646 constraints): the
    device CRS generator reproduces the oracle's Parameters bytes, and both the resident-
    witness prover and the drop-in bh_prove reproduce the oracle's proof; the proof verifies
    under the oracle's pairing restatement."""
    import hashlib
    import json
    import os
    from oracle import pairing as pr
    bh = _bh()
    here = os.path.dirname(os.path.abspath(__file__))
    with open(os.path.join(here, "golden", "mimc322.json")) as f:
        fx = json.load(f)
    params = bh.Parameters.chain(ctx, fx["rounds"])
    pbytes = params.write()
    assert hashlib.sha256(pbytes).hexdigest() == fx["params_sha256"]
    proof = bh.prove_witness(ctx, params, bh.Witness.chain(ctx, fx["rounds"]), fx["r"], fx["s"])
    assert proof.hex() == fx["proof"]
    assert bh.prove(ctx, params, bh.chain_assignment(fx["rounds"]), fx["r"], fx["s"]).hex() == fx["proof"]
    vk = pr.vk_from_params_bytes(params.vk_bytes())
    assert pr.verify_proof(vk, pr.proof_from_bytes(proof), [int(fx["image"], 16)])


@pytest.mark.parametrize("logc,tables", [(16, True), (16, False), (18, True), (18, False)])
def test_c3_family_proof_equals_cpu_port(ctx, logc, tables):
    """Oracle-backed parity at size: the device proof of a 2^16 / 2^18-constraint MiMC chain,
    with and without the SRS window tables, equals the proof of the C++ restatement of
    bellman's multicore prover (oracle/cpu) on the same Parameters bytes."""
    from oracle import cpu_port
    bh = _bh()
    rounds = (1 << (logc - 1)) - 1
    params = bh.Parameters.chain(ctx, rounds)
    w = bh.Witness.chain(ctx, rounds)
    ctx.set_tables(tables)
    try:
        if tables:
            params.prepare(w)
        dev = bh.prove_witness(ctx, params, w, 27134, 17146)
    finally:
        ctx.set_tables(True)
    port, _, _ = cpu_port.chain_prove(params.write(), rounds, threads=16)
    assert dev == port


@pytest.mark.parametrize("dense", [True, False])
def test_g2_msm_2p16_equals_cpu_port(ctx, dense):
    """A 2^16-scalar G2 multiexp (the b_g2 query of a 2^17-constraint chain's Parameters as
    bases, random dense scalars, optionally a density map with a base offset) equals
    bellman's multiexp algorithm in the C++ port."""
    from oracle import cpu_port
    from params_bytes import split_params
    bh = _bh()
    params = bh.Parameters.chain(ctx, (1 << 16) - 1)
    b_g2 = split_params(params.write())["b_g2"]
    nb = len(b_g2) // 192
    rng = np.random.default_rng(11)
    n = 1 << 16
    ex = rng.integers(0, 2**63, size=(n, 4), dtype=np.uint64)
    ex[:, 3] &= np.uint64(0x0FFFFFFFFFFFFFFF)  # < 2^252 < r: canonical
    bases = bh.Bases(ctx, bh.BH_G2, b_g2)
    if dense:
        off, bits = 0, None
        ex = ex[:nb]
    else:
        off = 3
        bits = rng.random(n) < (nb - off) / n * 0.98
    words = None if bits is None else bh.density_words(list(bits))
    got = bh.multiexp(ctx, bases, off, None if bits is None else list(bits), ex)
    want, _ = cpu_port.multiexp(2, b_g2, ex, off, words, threads=16)
    assert got == want


def test_c5_batch_proofs_pass_the_native_batch_verifier(ctx):
    """Throughput-mode proofs (distinct preimages, shared Parameters) accepted by the native
    batch verifier (verifier/batch.rs:95-169) and each by verify_proof; one tampered proof
    makes the batch fail."""
    bh = _bh()
    rounds = (1 << 11) - 1
    params = bh.Parameters.chain(ctx, rounds)
    ws = [bh.Witness.chain(ctx, rounds, seed=7, preimage_seed=20 + i) for i in range(4)]
    proofs = bh.prove_batch(ctx, params, ws, 27134, 17146)
    vk = params.vk_bytes()
    publics = [bh.fr_from_mont(bh.chain_assignment(rounds, seed=7, preimage_seed=20 + i)["inputs"])[1:]
               for i in range(4)]
    for p, pub in zip(proofs, publics):
        assert bh.verify_proof(vk, p, pub)
    rng = random.Random(5)
    zs = [rng.randrange(1, R) for _ in proofs]
    assert bh.verify_batch(vk, proofs, publics, zs)
    assert not bh.verify_batch(vk, proofs, publics[1:] + publics[:1], zs)


@pytest.mark.parametrize("value", [0, 1, 5, R - 1])
def test_degenerate_scalars_tables_plain_and_shards_agree(ctx, monkeypatch, value):
    """Edge scalars at prover size (2^17 constraints, window tables in use): every aux scalar
    equal (0: every multiexp empty; 1 and 5: all entries of a window in one bucket, whose
    continuation partials span every segment -- the log-depth fix-up path; r-1: every signed
    digit at its extreme with carries).  Not a satisfying assignment, so the proof is not
    valid, but tables vs plain windows vs two scalar shards vs 2 and 8 bucket shards compute the
    same multiexps byte for byte."""
    bh = _bh()
    rounds = (1 << 16) - 1
    params = bh.Parameters.chain(ctx, rounds)
    asg = bh.chain_assignment(rounds)
    asg["aux"][:] = bh.fr_to_mont([value])[0]
    h = bh.ctypes.c_void_p()
    bh._check(bh._lib.bh_witness_upload(ctx.h, bh._ptr(asg["a"]), bh._ptr(asg["b"]), bh._ptr(asg["c"]),
                                        asg["a"].shape[0], bh._ptr(asg["inputs"]), asg["inputs"].shape[0],
                                        bh._ptr(asg["aux"]), asg["aux"].shape[0], bh._ptr(asg["a_aux_density"]),
                                        bh._ptr(asg["b_input_density"]), bh._ptr(asg["b_aux_density"]),
                                        bh.ctypes.byref(h)), "bh_witness_upload")
    w = bh.Witness(ctx, h, asg["a"].shape[0])
    ctx.set_tables(False)
    try:
        plain = bh.prove_witness(ctx, params, w, 27134, 17146)
    finally:
        ctx.set_tables(True)
    params.prepare(w)
    assert bh.prove_witness(ctx, params, w, 27134, 17146) == plain
    parts = b"".join(bh.prove_witness_partial(ctx, params, w, k, 2) for k in range(2))
    assert bh.proof_from_partials(params.vk_bytes(), parts, 2, 27134, 17146) == plain
    # bucket shards: with every scalar equal, one rank's bucket range holds every entry
    monkeypatch.setenv("BH_SHARD_BUCKETS", "1")
    for n in (2, 8):
        parts = b"".join(bh.prove_witness_partial(ctx, params, w, k, n) for k in range(n))
        assert bh.proof_from_partials(params.vk_bytes(), parts, n, 27134, 17146) == plain


@pytest.mark.parametrize("nshards", [2, 3, 8])
def test_bucket_shards_equal_single_proof(ctx, monkeypatch, nshards):
    """BH_SHARD_BUCKETS=1 (prover.hip, bucket_shard_range): the large aux multiexps split across
    ranks by bucket range -- every rank sorts all the scalars and keeps the digits of its own
    granule-aligned range of the shared c-bit bucket set, and its reduction adds bk_lo times the
    range's plain sum -- at 2^17 constraints (window tables in use).  The per-rank partials (one
    context, rank after rank) and the virtual-rank run with the distributed H block both
    recombine to the single-device proof."""
    bh = _bh()
    rounds = (1 << 16) - 1
    params = bh.Parameters.chain(ctx, rounds)
    w = bh.Witness.chain(ctx, rounds)
    single = bh.prove_witness(ctx, params, w, 27134, 17146)
    monkeypatch.setenv("BH_SHARD_BUCKETS", "1")
    params.prepare(w, nshards)
    parts = b"".join(bh.prove_witness_partial(ctx, params, w, k, nshards) for k in range(nshards))
    assert bh.proof_from_partials(params.vk_bytes(), parts, nshards, 27134, 17146) == single
    if nshards & (nshards - 1) == 0:
        parts = bh.prove_witness_partials_local(ctx, params, w, nshards)
        assert bh.proof_from_partials(params.vk_bytes(), parts, nshards, 27134, 17146) == single


def test_msm_empty_and_single(ctx, golden):
    """Empty exponent list -> identity (multiexp.rs: the fold over no windows is zero); one
    exponent -> that multiple of the first base (against the oracle), both groups, sync and
    async seams."""
    from oracle import bls12_381 as bls
    bh = _bh()
    for group, data in ((bh.BH_G1, golden["msm_g1"]), (bh.BH_G2, golden["msm_g2"])):
        bases = _bases(ctx, group, data["bases"])
        ident = bytes([0x40]) + bytes((96 if group == bh.BH_G1 else 192) - 1)
        assert bh.multiexp(ctx, bases, 0, None, []) == ident
        assert bh.multiexp_async(ctx, bases, 0, None, []).wait() == ident
        k = 0x1234567890ABCDEF1234567890ABCDEF
        got = bh.multiexp(ctx, bases, 0, None, [k])
        G = bls.G1 if group == bh.BH_G1 else bls.G2
        base = (bls.g1_from_uncompressed if group == bh.BH_G1 else bls.g2_from_uncompressed)(
            bytes.fromhex(data["bases"][0]), checked=False)[1]
        want = G.to_affine(G.mul(G.from_affine(base), k))
        enc = bls.g1_to_uncompressed if group == bh.BH_G1 else bls.g2_to_uncompressed
        assert got == enc(want)


def test_two_contexts_share_one_parameters(ctx):
    """The 'shared Parameters' use: one Parameters and one witness, created on
    the fixture's context and without prepared tables, proved from two other contexts on two
    host threads at once.  The first proofs race to build the window tables (exclusive lock,
    synchronised build) while the other reads under the shared lock; every proof equals the
    single-context one."""
    import threading
    bh = _bh()
    rounds = (1 << 16) - 1  # 2^17 constraints: the large multiexps use window tables
    params = bh.Parameters.chain(ctx, rounds)
    w = bh.Witness.chain(ctx, rounds)
    ctxs = [bh.Context(0), bh.Context(0)]
    results, errors = [], []

    def worker(c):
        try:
            for _ in range(2):
                results.append(bh.prove_witness(c, params, w, 27134, 17146))
        except Exception as e:  # pragma: no cover - reported below
            errors.append(repr(e))

    try:
        threads = [threading.Thread(target=worker, args=(c,)) for c in ctxs]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors, errors
        assert ctxs[0].last_stats()[10] > 0  # the window tables were used
        single = bh.prove_witness(ctx, params, w, 27134, 17146)
        assert len(results) == 4 and set(results) == {single}
    finally:
        for c in ctxs:
            c.close()


@pytest.mark.parametrize("rounds", [15, 5000, (1 << 15) - 1, (1 << 17) - 1])
def test_multiexp_seam_proof_equals_prove(ctx, golden, rounds):
    """INTEGRATION.md section 2's swap at the multiexp level (multiexp.rs:252-281 inside
    create_proof, prover.rs:206-349): h computed on the device (bh_compute_h_scalars), the
    assignments uploaded once as bh_scalars, the eight multiexps submitted on the Parameters' own
    vectors (bh_params_vector, so the window tables bh_params_prepare built are used from 2^16
    set scalars up) and assembled by bh_proof_from_partials: byte-equal to bh_prove."""
    bh = _bh()
    params = bh.Parameters.chain(ctx, rounds)
    asg = bh.chain_assignment(rounds)
    want = bh.prove(ctx, params, asg, 27134, 17146)
    if rounds >= (1 << 15) - 1:
        params.prepare(bh.Witness.chain(ctx, rounds))
    assert bh.prove_seam(ctx, params, asg, 27134, 17146) == want
    if rounds == 15:
        fx = [f for f in golden["proofs"] if f["name"] == "mimc_chain_r15"][0]
        assert want.hex() == fx["proof"]


def test_scalars_outlive_their_handle(ctx):
    """A multiexp in flight keeps the device vector it reads: the bh_scalars freed right after
    submit still gives the result of a fresh run (and of the host-buffer multiexp)."""
    bh = _bh()
    rounds = (1 << 17) - 1
    params = bh.Parameters.chain(ctx, rounds)
    params.prepare(bh.Witness.chain(ctx, rounds))
    asg = bh.chain_assignment(rounds)
    L = params.vector(bh.BH_VEC_L)
    aux = bh.Scalars(ctx, asg["aux"], montgomery=True)
    want = bh.multiexp_async(ctx, L, 0, None, aux).wait()
    w = bh.multiexp_async(ctx, L, 0, None, aux)
    aux.close()
    assert w.wait() == want
    assert bh.multiexp(ctx, L, 0, None, asg["aux"], montgomery=True) == want
    assert bh.multiexp_async(ctx, L, 0, None, asg["aux"], montgomery=True).wait() == want


def test_h_scalars_deferred_submit_and_context_teardown(ctx):
    """Multiexps submitted on h while bh_compute_h_scalars' producer is still uploading are
    enqueued by that producer (create_proof's order: h first); a context destroyed with such
    jobs pending waits for the producer, then detaches them (wait raises)."""
    bh = _bh()
    rounds = (1 << 15) - 1
    params = bh.Parameters.chain(ctx, rounds)
    asg = bh.chain_assignment(rounds)
    H = params.vector(bh.BH_VEC_H)
    h = bh.compute_h_scalars(ctx, asg["a"], asg["b"], asg["c"])
    ws = [bh.multiexp_async(ctx, H, 0, None, h) for _ in range(3)]
    got = [w.wait() for w in ws]
    h.sync()
    assert got[0] == got[1] == got[2]
    hv = bh.compute_h(ctx, asg["a"], asg["b"], asg["c"])
    assert len(h) == len(hv)
    assert bh.multiexp(ctx, H, 0, None, hv) == got[0]
    c2 = bh.Context(0)
    p2 = bh.Parameters.chain(c2, rounds)
    h2 = bh.compute_h_scalars(c2, asg["a"], asg["b"], asg["c"])
    w2 = bh.multiexp_async(c2, p2.vector(bh.BH_VEC_H), 0, None, h2)
    c2.close()
    with pytest.raises(bh.SynthesisError):
        w2.wait()
    h2.close()


def test_h_scalars_submit_from_another_context_and_stamps(ctx):
    """A multiexp on an h vector that ANOTHER context of the device is still producing is
    enqueued after that producer has enqueued H (the submit waits on the host; round 4 refused
    it), and equals the multiexp of the host-computed h; the producer's stage stamps
    (bh_scalars_stamps) are ordered: a, b, c copies, H enqueued."""
    bh = _bh()
    rounds = (1 << 15) - 1
    params = bh.Parameters.chain(ctx, rounds)
    asg = bh.chain_assignment(rounds)
    H = params.vector(bh.BH_VEC_H)
    c2 = bh.Context(0)
    h = bh.compute_h_scalars(c2, asg["a"], asg["b"], asg["c"])
    got = bh.multiexp_async(ctx, H, 0, None, h).wait()
    hv = bh.compute_h(ctx, asg["a"], asg["b"], asg["c"])
    assert bh.multiexp(ctx, H, 0, None, hv) == got
    st = h.stamps()
    assert len(st) == 6 and 0 <= st[0] <= st[1] <= st[2] <= st[3] <= st[4]
    h.close()
    c2.close()


def test_shared_sorts_follow_the_vector_not_its_address(ctx):
    """Jobs over the same bh_scalars vector share digit sorts: l's full-density sort is compacted
    through b_aux's density map for b_g1_aux (the prover's derived sort), and b_g2_aux (same vector,
    density map, base offset and digit geometry) copies b_g1_aux's; a vector freed and replaced by
    another with other contents (likely at the same device address) is sorted afresh: every result
    equals the host-buffer multiexp."""
    bh = _bh()
    rounds = (1 << 15) - 1
    params = bh.Parameters.chain(ctx, rounds)
    params.prepare(bh.Witness.chain(ctx, rounds))
    asg = bh.chain_assignment(rounds)
    ni, na = asg["inputs"].shape[0], asg["aux"].shape[0]
    B1, B2 = params.vector(bh.BH_VEC_B_G1), params.vector(bh.BH_VEC_B_G2)
    Lv = params.vector(bh.BH_VEC_L)
    dens = bh.DensityWords(asg["b_aux_density"], na)
    off = bh.DensityWords(asg["b_input_density"], ni).total()
    for k in range(3):
        ex = np.ascontiguousarray(np.roll(asg["aux"], 977 * k, axis=0))
        v = bh.Scalars(ctx, ex, montgomery=True)
        wl = bh.multiexp_async(ctx, Lv, 0, None, v)
        w1 = bh.multiexp_async(ctx, B1, off, dens, v)
        w2 = bh.multiexp_async(ctx, B2, off, dens, v)
        got = (wl.wait(), w1.wait(), w2.wait())
        v.close()
        assert got == (bh.multiexp(ctx, Lv, 0, None, ex, montgomery=True),
                       bh.multiexp(ctx, B1, off, dens, ex, montgomery=True),
                       bh.multiexp(ctx, B2, off, dens, ex, montgomery=True))


_G2_DIRECT_SCRIPT = r"""
import json, os, random, sys
sys.path.insert(0, os.path.join(sys.argv[1], "bellman-mpc_amd"))
sys.path.insert(0, sys.argv[1])
import bellman_hip as bh
from oracle import bellman as bm
from oracle import bls12_381 as bls
R = %d
ctx = bh.Context(0)
E = bm.BLS12_381
aff = lambda k: E.G2.to_affine(E.G2.mul(bls.G2.generator(), k %% R))
rng = random.Random(21)
pts = [aff(11)] * 24 + [aff(R - 11)] * 24 + [aff(29)] * 16 + [aff(rng.randrange(1, R)) for _ in range(8)]
bases = bh.Bases(ctx, bh.BH_G2, b"".join(bls.g2_to_uncompressed(p) for p in pts))
e1, e2 = rng.randrange(R), rng.randrange(R)
cases = [[e1] * 48 + [e2] * 16 + [rng.randrange(R) for _ in range(8)], [1] * 24 + [R - 1] * 24 + [2] * 16 + [0] * 8]
msm = [bh.multiexp(ctx, bases, 0, None, ex).hex() for ex in cases]
rounds = (1 << 16) - 1
params = bh.Parameters.chain(ctx, rounds)
w = bh.Witness.chain(ctx, rounds)
params.prepare(w)
proof = bh.prove_witness(ctx, params, w, 27134, 17146).hex()
print(json.dumps({"cases": [[str(x) for x in ex] for ex in cases], "msm": msm, "proof": proof}))
""" % R


def test_g2_direct_accumulation_equals_default(ctx):
    """The direct-load G2 accumulation (BH_G2_DIRECT=1: no LDS prefetch slots, two waves per SIMD;
    msm_impl.cuh k_accumulate_g2d) in a process of its own: G2 multiexps with equal and opposite bases
    in one bucket equal the oracle, and a 2^17-constraint proof over window tables (its b_g2_aux
    accumulation is the G2 kernel) equals this process's proof on the default kernel."""
    import json
    import os
    import subprocess
    import sys
    bh = _bh()
    from oracle import bellman as bm
    from oracle import bls12_381 as bls
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, BH_G2_DIRECT="1")
    p = subprocess.run([sys.executable, "-c", _G2_DIRECT_SCRIPT, root], env=env, capture_output=True, text=True,
                       timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    got = json.loads(p.stdout.strip().splitlines()[-1])
    E = bm.BLS12_381
    aff = lambda k: E.G2.to_affine(E.G2.mul(bls.G2.generator(), k % R))
    rng = random.Random(21)
    pts = [aff(11)] * 24 + [aff(R - 11)] * 24 + [aff(29)] * 16 + [aff(rng.randrange(1, R)) for _ in range(8)]
    for ex, m in zip(got["cases"], got["msm"]):
        want = bls.g2_to_uncompressed(E.G2.to_affine(bm.multiexp(E, E.G2, pts, 0, None, [int(x) for x in ex])))
        assert bytes.fromhex(m) == want
    rounds = (1 << 16) - 1
    params = bh.Parameters.chain(ctx, rounds)
    w = bh.Witness.chain(ctx, rounds)
    params.prepare(w)
    assert bh.prove_witness(ctx, params, w, 27134, 17146).hex() == got["proof"]


def test_proof_stats_accumulation_wall_time(ctx):
    """bh_last_stats after a proof with window tables (2^17 constraints): the G1 / G2 launch
    sums [2] / [5], the mixed additions [8] / [9] (one per non-zero digit: at most windows x
    pairs, with at most 32 windows of c >= 8 bits), and the accumulation wall times [21] / [22] (the union of the launches, which two
    accumulation lanes can overlap): positive, and never more than the launch sums."""
    bh = _bh()
    rounds = (1 << 16) - 1
    params = bh.Parameters.chain(ctx, rounds)
    w = bh.Witness.chain(ctx, rounds)
    params.prepare(w)
    bh.prove_witness(ctx, params, w, 27134, 17146)
    st = ctx.last_stats()
    assert len(st) == 23
    g1_sum, g2_sum, g1_wall, g2_wall = st[2], st[5], st[21], st[22]
    assert 0 < g1_wall <= g1_sum * 1.0001 and 0 < g2_wall <= g2_sum * 1.0001
    assert 0 < st[8] <= 32 * st[4] and 0 < st[9] <= 32 * st[7]


@pytest.mark.parametrize("env", [{"BH_PROVER_SERIAL": "1"}, {"BH_ACC_EVENTS": "0"}])
def test_diagnostic_modes_give_the_same_proof(ctx, monkeypatch, env):
    """The library's two diagnostic switches, read per proof: BH_PROVER_SERIAL=1 (every kernel on
    one stream, for per-kernel profiles; bh_prove then enqueues H after the whole upload) and
    BH_ACC_EVENTS=0 (no timing events around the accumulations) give the default proof, from a
    resident witness and from host buffers."""
    bh = _bh()
    rounds = (1 << 15) - 1
    params = bh.Parameters.chain(ctx, rounds)
    w = bh.Witness.chain(ctx, rounds)
    asg = bh.chain_assignment(rounds)
    want = bh.prove_witness(ctx, params, w, 27134, 17146)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    assert bh.prove_witness(ctx, params, w, 27134, 17146) == want
    assert bh.prove(ctx, params, asg, 27134, 17146) == want
