"""The host's share of a proof whose a, b, c are computed on the device (bh_r1cs_witness): the
assignment-only constraint system, and the rule that derives ProvingAssignment's density maps
from a KeypairAssembly's columns, both against bh.synthesize (prover.rs:55-156, 187-204).  No GPU."""
import pytest

R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


def _bh():
    import bellman_hip as bh
    return bh


class ZeroCoefficient:
    """An aux variable whose only term in A, and an input whose only term in B, has coefficient
    zero; a third variable that no constraint mentions in A or B at all."""

    def __init__(self, witness=True):
        self.witness = witness

    def synthesize(self, cs):
        v = (lambda x: (lambda: x if self.witness else None))
        x = cs.alloc("x", v(5))
        y = cs.alloc("y", v(7))
        unused = cs.alloc("only in c", v(35))
        pub = cs.alloc_input("pub", v(9))
        cs.enforce("zero in a", lambda lc: lc + (0, x) + y, lambda lc: lc + (0, pub) + x, lambda lc: lc + unused)
        cs.enforce("r - r", lambda lc: lc + (R, y), lambda lc: lc + cs.one(), lambda lc: lc)


def _circuits():
    from oracle import circuits as cc
    return {"xor": cc.XorDemo(True, False), "and": cc.AndDemo(True, True), "add": cc.AddDemo(3, 4),
            "chain_r7": cc.chain_circuit(R, 7), "zero_coefficient": ZeroCoefficient()}


NAMES = ["xor", "and", "add", "chain_r7", "zero_coefficient"]


@pytest.mark.parametrize("name", NAMES)
def test_assign_is_synthesize_without_the_evaluation(name):
    bh = _bh()
    circuit = _circuits()[name]
    p, q = bh.synthesize(circuit), bh.assign(circuit)
    assert q.input_assignment == p.input_assignment
    assert q.aux_assignment == p.aux_assignment
    assert q.input_assignment[0] == 1
    assert not hasattr(q, "a")


@pytest.mark.parametrize("name", NAMES)
def test_density_is_column_not_empty(name):
    bh = _bh()
    circuit = _circuits()[name]
    p = bh.synthesize(circuit)
    a_aux, b_in, b_aux = bh.column_densities(bh.synthesize_keypair(circuit))
    assert a_aux == p.a_aux_density.bv
    assert b_in == p.b_input_density.bv
    assert b_aux == p.b_aux_density.bv


def test_zero_coefficient_term_is_dense():
    bh = _bh()
    asm = bh.synthesize_keypair(ZeroCoefficient())
    a_aux, b_in, b_aux = bh.column_densities(asm)
    # x: its one term in A has coefficient 0; y: 1 and r (= 0 mod r); the third never appears
    assert a_aux == [True, True, False]
    # ONE has a term in B, pub only the zero one
    assert b_in == [True, True]
    assert b_aux == [True, False, False]
    assert asm.at_aux[0] == [(0, 0)] and asm.at_aux[1] == [(1, 0), (0, 1)]


@pytest.mark.parametrize("kind", ["aux", "input"])
def test_assignment_only_raises_on_a_missing_value(kind):
    bh = _bh()
    cs = bh.AssignmentOnly()
    with pytest.raises(bh.AssignmentMissing):
        (cs.alloc if kind == "aux" else cs.alloc_input)("nothing", lambda: None)
    with pytest.raises(bh.AssignmentMissing):
        bh.assign(ZeroCoefficient(witness=False))


def test_assignment_only_ignores_enforce():
    bh = _bh()
    cs = bh.AssignmentOnly()

    def boom(lc):
        raise AssertionError("enforce must not evaluate its combinations")

    x = cs.alloc("x", lambda: R + 3)
    cs.enforce("never looked at", boom, boom, boom)
    assert cs.aux_assignment == [3] and (x.kind, x.index) == ("aux", 0)
    assert cs.one() is bh.ONE and cs.namespace("n") is cs
