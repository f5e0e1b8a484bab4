"""The crafted proof encodings of tests/proof_cases.py against the host batch verifier
(bh_verify_batch, csrc/verify.cpp): every case is rejected with the status the case names (or, for
the well-formed ones, judged invalid), at the head and at the tail of an otherwise valid batch, and
the untampered batch is accepted.  This validates the yardstick that
tests/test_gpu_verify_device.py holds the device decoder to.  Host code only: runs on the CPU."""
import random

import pytest

import proof_cases as pc


@pytest.fixture(scope="module")
def bh():
    import bellman_hip
    return bellman_hip


@pytest.fixture(scope="module")
def batch():
    """one verifying key's golden proof three times over, with random z"""
    params, items = next(iter(pc.golden_batches().items()))
    proofs = [p for p, _ in items] * 3
    inputs = [i for _, i in items] * 3
    rng = random.Random(5)
    return params, proofs[:3], inputs[:3], [rng.randrange(1, pc.R) for _ in range(3)]


def test_untampered_batch_is_accepted(bh, batch):
    params, proofs, inputs, zs = batch
    assert pc.call_batch(bh.lib().bh_verify_batch, params, proofs, inputs, zs) == (pc.OK, 1)


def _case_ids():
    proof = next(iter(pc.golden_batches().values()))[0][0]
    return [name for name, _, _ in pc.proof_cases(proof)]


@pytest.mark.parametrize("idx", range(len(_case_ids())), ids=_case_ids())
def test_host_verifier_rejects_each_case(bh, batch, idx):
    params, proofs, inputs, zs = batch
    name, crafted, status = pc.proof_cases(proofs[0])[idx]
    for j in (0, len(proofs) - 1):
        tampered = proofs[:j] + [crafted] + proofs[j + 1:]
        got = pc.call_batch(bh.lib().bh_verify_batch, params, tampered, inputs, zs)
        assert got == (status, 0), (name, j, got)


def test_case_list_covers_every_slot():
    names = _case_ids()
    for slot, extra in (("A", 0), ("B", 2), ("C", 0)):
        mine = [n for n in names if n.startswith(slot + ":")]
        assert len(mine) == 9 + extra, mine
    assert "B:c0_equals_p" in names and "B:c0_top_bit_set" in names


def test_non_residue_and_off_subgroup_points_are_what_they_claim():
    from oracle import bls12_381 as bls
    x = pc.non_residue_x("A")
    assert pow((x ** 3 + 4) % pc.P, (pc.P - 1) // 2, pc.P) == pc.P - 1
    for slot, G in (("A", bls.G1), ("B", bls.G2)):
        pt = pc.off_subgroup(slot)
        assert G.on_curve_affine(pt) and not G.is_identity(G.mul(G.from_affine(pt), pc.R))
