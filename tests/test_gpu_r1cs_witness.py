"""The prover's witness built on the device from a resident R1CS (bh_r1cs_witness), read back with
bh_witness_read: against integer dot products, against the uploaded witness of the host-evaluated
vectors, against the native chain synthesizer, and through the provers.  Exact throughout: field
elements as canonical integers (or reduced Montgomery words), proofs as bytes."""
import ctypes
import functools
import random
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
RS = (27134, 17146)
FORK = dict(alpha=6, beta=24, gamma=6, delta=24, tau=2)
INVALID = 10


def _bh():
    import bellman_hip as bh
    return bh


def _segment(ctx):
    return _bh().R1CS.chain(ctx, 1).sizes()["segment"]


def _fx(golden, name):
    return [f for f in golden["proofs"] if f["name"] == name][0]


def _circuit(name, witness=True):
    from oracle import circuits as cc
    if name.startswith("xor"):
        return cc.XorDemo(True, False) if witness else cc.XorDemo(None, None)
    if name.startswith("and"):
        return cc.AndDemo(True, True) if witness else cc.AndDemo(None, None)
    return cc.chain_circuit(R, int(name.rsplit("r", 1)[1]), witness=witness)


# ------------------------------------------------------------------ matrices by rows, and what they must give
def _draw(rng):
    return rng.choice([0, 1, R - 1, rng.randrange(R), rng.randrange(R)])


def _rows(rng, lengths, n):
    """One list of (coeff, variable) per constraint."""
    return [[(_draw(rng), rng.randrange(n)) for _ in range(k)] for k in lengths]


def _columns(rows, n):
    cols = [[] for _ in range(n)]
    for i, row in enumerate(rows):
        for coeff, var in row:
            cols[var].append((coeff, i))
    return cols


def _rows_of_assembly(asm):
    """KeypairAssembly's columns (inputs, then aux) as rows of (coeff, variable)."""
    out = []
    for ins, auxs in ((asm.at_inputs, asm.at_aux), (asm.bt_inputs, asm.bt_aux), (asm.ct_inputs, asm.ct_aux)):
        rows = [[] for _ in range(asm.num_constraints)]
        for var, col in enumerate(ins + auxs):
            for coeff, i in col:
                rows[i].append((coeff, var))
        out.append(rows)
    return out


def _expected(mats, inputs, aux):
    """ProvingAssignment after prover.rs:187-204 as plain integers: a, b, c with the appended rows
    (not padded), and the three density maps."""
    z = list(inputs) + list(aux)
    ni, na = len(inputs), len(aux)
    vec = [[sum(c * z[v] for c, v in row) % R for row in rows] for rows in mats]
    vec[0] += [x % R for x in inputs]
    vec[1] += [0] * ni
    vec[2] += [0] * ni
    used = [{v for row in rows for _, v in row} for rows in mats]
    return dict(a=vec[0], b=vec[1], c=vec[2], inputs=[x % R for x in inputs], aux=[x % R for x in aux],
                a_aux_density=[ni + i in used[0] for i in range(na)],
                b_input_density=[i in used[1] for i in range(ni)],
                b_aux_density=[ni + i in used[1] for i in range(na)])


def _domain(nc):
    m = 1
    while m < nc:
        m *= 2
    return m


def _assert_reads(got, want):
    nc, m = len(want["a"]), _domain(len(want["a"]))
    assert (got["constraints"], got["m"], got["inputs_n"], got["aux_n"]) == (nc, m, len(want["inputs"]),
                                                                             len(want["aux"]))
    for k in ("a", "b", "c"):
        assert got[k] == want[k] + [0] * (m - nc), k
    for k in ("inputs", "aux", "a_aux_density", "b_input_density", "b_aux_density"):
        assert got[k] == want[k], k


def _read(w):
    got = w.read()
    sz = w.sizes()
    got["inputs_n"], got["aux_n"] = sz["inputs"], sz["aux"]
    return got


def _r1cs(ctx, mats, ni, na, nc):
    bh = _bh()
    return bh.R1CS.from_arrays(ctx, ni, na, nc, *[bh.flatten_columns(_columns(rows, ni + na)) for rows in mats])


LONG = {"0": lambda S: 0, "1": lambda S: 1, "S-1": lambda S: S - 1, "S": lambda S: S, "S+1": lambda S: S + 1,
        "2S+1": lambda S: 2 * S + 1, "S*S+1": lambda S: S * S + 1}
NI = 2


@functools.lru_cache(maxsize=None)
def _boundary_case(K, nc, num_aux):
    """One row of A (nc // 3) and the last row of C with K terms beside rows of 0..3 terms, a (variable,
    row) pair twice in B's row 0; coefficients and values from {0, 1, r - 1, random}.  Computed once
    per shape and shared."""
    rng = random.Random(100000 * K + 100 * nc + num_aux)
    n = NI + num_aux
    lengths = [[rng.randrange(4) for _ in range(nc)] for _ in range(3)]
    lengths[0][nc // 3] = K
    lengths[2][nc - 1] = K
    mats = [_rows(rng, l, n) for l in lengths]
    v = rng.randrange(n)
    mats[1][0] += [(_draw(rng), v), (rng.randrange(1, R), v)]
    inputs = [1] + [_draw(rng) for _ in range(NI - 1)]
    aux = [_draw(rng) for _ in range(num_aux)]
    return mats, inputs, aux, _expected(mats, inputs, aux)


# ------------------------------------------------------------------ 1. the product at its boundaries
@pytest.mark.parametrize("num_aux", [1, 63, 64, 65])
@pytest.mark.parametrize("nc", [1, 37, 255, 256, 257])
@pytest.mark.parametrize("k_expr", LONG)
def test_product_boundaries(ctx, k_expr, nc, num_aux):
    bh = _bh()
    K = LONG[k_expr](_segment(ctx))
    mats, inputs, aux, want = _boundary_case(K, nc, num_aux)
    r1cs = _r1cs(ctx, mats, NI, num_aux, nc)
    _assert_reads(_read(bh.Witness.from_r1cs(ctx, r1cs, inputs, aux)), want)


def test_one_in_thousands_of_rows(ctx):
    """ONE with a term in every one of 2100 rows of B and in S*S + 1 rows of A: one variable's
    terms scatter over thousands of row cursors, and a column of the matrices is a long one."""
    bh = _bh()
    S = _segment(ctx)
    rng = random.Random(4242)
    ni, na, nc = 2, 5, 2100
    n = ni + na
    mats = [_rows(rng, [rng.randrange(3) for _ in range(nc)], n) for _ in range(3)]
    for i in range(nc):
        mats[1][i].append((_draw(rng), 0))
    for i in rng.sample(range(nc), S * S + 1):
        mats[0][i].append((rng.randrange(1, R), 0))
    inputs, aux = [1, _draw(rng)], [_draw(rng) for _ in range(na)]
    r1cs = _r1cs(ctx, mats, ni, na, nc)
    assert r1cs.sizes()["nnz_b"] >= nc and r1cs.sizes()["nnz_a"] >= S * S + 1 + ni
    _assert_reads(_read(bh.Witness.from_r1cs(ctx, r1cs, inputs, aux)), _expected(mats, inputs, aux))


# ------------------------------------------------------------------ 2. field by field against the upload
def _assignment(want):
    def tracker(bits):
        return types.SimpleNamespace(bv=list(bits))
    return types.SimpleNamespace(a=want["a"], b=want["b"], c=want["c"], input_assignment=want["inputs"],
                                 aux_assignment=want["aux"], a_aux_density=tracker(want["a_aux_density"]),
                                 b_input_density=tracker(want["b_input_density"]),
                                 b_aux_density=tracker(want["b_aux_density"]))


@pytest.mark.parametrize("nc,num_aux", [(1, 1), (257, 65)])
@pytest.mark.parametrize("k_expr", LONG)
def test_same_as_the_uploaded_witness(ctx, k_expr, nc, num_aux):
    bh = _bh()
    K = LONG[k_expr](_segment(ctx))
    mats, inputs, aux, want = _boundary_case(K, nc, num_aux)
    uploaded = _read(bh.Witness.from_assignment(ctx, _assignment(want)))
    built = _read(bh.Witness.from_r1cs(ctx, _r1cs(ctx, mats, NI, num_aux, nc), inputs, aux))
    assert sorted(uploaded) == sorted(built)
    for k in uploaded:
        assert uploaded[k] == built[k], k


# ------------------------------------------------------------------ 3. against the native synthesizer
def _bits(words, n):
    return np.unpackbits(np.ascontiguousarray(words, dtype="<u8").view(np.uint8), bitorder="little")[:n]


def _assert_raw(got, asg):
    """got: Witness.read(raw=True); asg: chain_assignment's dict (reduced Montgomery words)."""
    nc, ni, na = asg["a"].shape[0], asg["inputs"].shape[0], asg["aux"].shape[0]
    m = _domain(nc)
    assert (got["constraints"], got["m"], got["inputs"].shape[0], got["aux"].shape[0]) == (nc, m, ni, na)
    for k in ("a", "b", "c"):
        assert got[k].shape == (m, 4)
        assert np.array_equal(got[k][:nc], asg[k]), k
        assert not got[k][nc:].any(), k + " padding"
    for k in ("inputs", "aux"):
        assert np.array_equal(got[k], asg[k]), k
    for k, n in (("a_aux_density", na), ("b_input_density", ni), ("b_aux_density", na)):
        assert np.array_equal(_bits(got[k], n), _bits(asg[k], n)), k


@pytest.mark.parametrize("rounds", [1, 15, 100, 5000, 131071, 131072])
def test_chain_against_native_assignment(ctx, rounds):
    """rounds = 131071: nc = 2^18 exactly; 131072: 2^18 + 2, almost half the domain is padding."""
    bh = _bh()
    asg = bh.chain_assignment(rounds)
    w = bh.Witness.from_r1cs(ctx, bh.R1CS.chain(ctx, rounds), asg["inputs"], asg["aux"])
    assert w.sizes() == dict(constraints=2 * rounds + 2, m=_domain(2 * rounds + 2), inputs=2, aux=2 * rounds + 1)
    _assert_raw(w.read(raw=True), asg)
    if rounds == 100:  # and the chain-built witness reads back the same through the same call
        _assert_raw(bh.Witness.chain(ctx, rounds).read(raw=True), asg)


# ------------------------------------------------------------------ 4. proofs
@pytest.mark.parametrize("name", ["xor_true_false", "and_true_true", "mimc_chain_r7", "mimc_chain_r15"])
def test_golden_proofs(ctx, golden, name):
    bh = _bh()
    r1cs = bh.R1CS.from_assembly(ctx, bh.synthesize_keypair(_circuit(name, witness=False)))
    params = bh.Parameters.generate(ctx, r1cs, **FORK)
    assert bh.create_proof_r1cs(ctx, r1cs, _circuit(name), params, *RS) == bytes.fromhex(_fx(golden, name)["proof"])


def test_every_prover_takes_the_witness(ctx):
    """rounds = 100: nc = 202, m = 256."""
    bh = _bh()
    rounds = 100
    asg = bh.chain_assignment(rounds)
    params = bh.Parameters.chain(ctx, rounds)
    w = bh.Witness.from_r1cs(ctx, bh.R1CS.chain(ctx, rounds), asg["inputs"], asg["aux"])
    want = bh.prove_witness(ctx, params, bh.Witness.chain(ctx, rounds), *RS)
    assert bh.prove_witness(ctx, params, w, *RS) == want
    assert bh.prove_batch(ctx, params, [w, w], *RS) == [want, want]
    partials = bh.prove_witness_partials_local(ctx, params, w, 2)
    assert bh.proof_from_partials(params.vk_bytes(), partials, 2, *RS) == want


# ------------------------------------------------------------------ 5. satisfaction
@functools.lru_cache(maxsize=None)
def _chain15():
    bh = _bh()
    circuit = _circuit("mimc_chain_r15")
    asm = bh.synthesize_keypair(circuit)
    p = bh.assign(circuit)
    return asm, _rows_of_assembly(asm), list(p.input_assignment), list(p.aux_assignment)


def _broken(mats, inputs, aux):
    e = _expected(mats, inputs, aux)
    return [i for i in range(len(e["a"])) if e["a"][i] * e["b"][i] % R != e["c"][i]]


def test_satisfied_gives_none_and_the_same_witness(ctx):
    bh = _bh()
    asm, mats, inputs, aux = _chain15()
    r1cs = bh.R1CS.from_assembly(ctx, asm)
    assert _broken(mats, inputs, aux) == []
    checked, first = bh.Witness.from_r1cs(ctx, r1cs, inputs, aux, check=True)
    assert first is None
    assert _read(checked) == _read(bh.Witness.from_r1cs(ctx, r1cs, inputs, aux))
    _assert_reads(_read(checked), _expected(mats, inputs, aux))


@pytest.mark.parametrize("delta", [1, 5, R - 1], ids=["plus1", "plus5", "minus1"])
def test_one_changed_aux_value(ctx, delta):
    """aux 11 stands with coefficient 1 in c of row 9: plus1 leaves a b - c = -1 there."""
    bh = _bh()
    asm, mats, inputs, aux = _chain15()
    r1cs = bh.R1CS.from_assembly(ctx, asm)
    bad = list(aux)
    bad[11] = (bad[11] + delta) % R
    broken = _broken(mats, inputs, bad)
    assert broken and broken[0] == 9
    w, first = bh.Witness.from_r1cs(ctx, r1cs, inputs, bad, check=True)
    assert first == broken[0]
    # the witness is returned all the same, and is the unchecked one
    assert _read(w) == _read(bh.Witness.from_r1cs(ctx, r1cs, inputs, bad))
    _assert_reads(_read(w), _expected(mats, inputs, bad))


def test_the_earliest_of_two_broken_rows(ctx):
    bh = _bh()
    asm, mats, inputs, aux = _chain15()
    r1cs = bh.R1CS.from_assembly(ctx, asm)
    last_own = asm.num_constraints - 1
    image = [inputs[0], (inputs[1] + 1) % R]
    assert _broken(mats, image, aux) == [last_own]  # the image stands in the last own row only
    assert bh.Witness.from_r1cs(ctx, r1cs, image, aux, check=True)[1] == last_own
    bad = list(aux)
    bad[4] = (bad[4] + 1) % R
    broken = _broken(mats, image, bad)
    assert len(broken) >= 2 and broken[0] < last_own and broken[-1] == last_own
    assert bh.Witness.from_r1cs(ctx, r1cs, image, bad, check=True)[1] == broken[0]


# ------------------------------------------------------------------ 6. reuse and statuses
def test_reuse_of_the_handle(ctx):
    """Two assignments on one handle (the second on the cached row view); the column side of the
    handle, bh_r1cs_eval and the parameter generation, is what it was before."""
    bh = _bh()
    S = _segment(ctx)
    mats, inputs, aux, want = _boundary_case(S + 1, 37, 63)
    r1cs = _r1cs(ctx, mats, NI, 63, 37)
    rng = random.Random(9)
    x = [_draw(rng) for _ in range(64)]
    eval_before = r1cs.eval(x)
    chain = bh.R1CS.chain(ctx, 15)
    params_before = bh.Parameters.generate(ctx, chain, **FORK).write()
    _assert_reads(_read(bh.Witness.from_r1cs(ctx, r1cs, inputs, aux)), want)
    inputs2, aux2 = [1, 12345], [_draw(rng) for _ in range(63)]
    _assert_reads(_read(bh.Witness.from_r1cs(ctx, r1cs, inputs2, aux2)), _expected(mats, inputs2, aux2))
    _assert_reads(_read(bh.Witness.from_r1cs(ctx, r1cs, inputs, aux)), want)
    assert r1cs.eval(x) == eval_before
    asg = bh.chain_assignment(15)
    for _ in range(2):
        _assert_raw(bh.Witness.from_r1cs(ctx, chain, asg["inputs"], asg["aux"]).read(raw=True), asg)
    assert bh.Parameters.generate(ctx, chain, **FORK).write() == params_before


def test_statuses(ctx):
    bh = _bh()
    lib = bh.lib()
    asg = bh.chain_assignment(15)
    r1cs = bh.R1CS.chain(ctx, 15)
    ins, aux = np.ascontiguousarray(asg["inputs"]), np.ascontiguousarray(asg["aux"])
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    h = ctypes.c_void_p()
    out = ctypes.byref(h)
    assert lib.bh_r1cs_witness(None, r1cs.h, p(ins), p(aux), None, out) == INVALID
    assert lib.bh_r1cs_witness(ctx.h, None, p(ins), p(aux), None, out) == INVALID
    assert lib.bh_r1cs_witness(ctx.h, r1cs.h, None, p(aux), None, out) == INVALID
    assert lib.bh_r1cs_witness(ctx.h, r1cs.h, p(ins), None, None, out) == INVALID
    assert lib.bh_r1cs_witness(ctx.h, r1cs.h, p(ins), p(aux), None, None) == INVALID
    r_words = np.array([(R >> (64 * k)) & (2 ** 64 - 1) for k in range(4)], dtype=np.uint64)
    for which, at in ((0, 1), (1, 0), (1, aux.shape[0] - 1)):
        arrs = [ins.copy(), aux.copy()]
        arrs[which][at] = r_words
        assert lib.bh_r1cs_witness(ctx.h, r1cs.h, p(arrs[0]), p(arrs[1]), None, out) == INVALID
    assert h.value is None
    sizes = (ctypes.c_size_t * 4)()
    assert lib.bh_witness_sizes(None, sizes) == INVALID
    assert lib.bh_witness_read(None, *[None] * 8) == INVALID
    w = bh.Witness.from_r1cs(ctx, r1cs, ins, aux)
    assert lib.bh_witness_sizes(w.h, None) == INVALID
    assert lib.bh_witness_read(w.h, *[None] * 8) == 0  # every pointer may be null
    # the context and the handle still build a correct witness
    _assert_raw(w.read(raw=True), asg)
    _assert_raw(bh.Witness.from_r1cs(ctx, r1cs, ins, aux, check=True)[0].read(raw=True), asg)
