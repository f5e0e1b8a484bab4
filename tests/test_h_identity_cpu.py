"""The identity behind the six-transform H block, on the oracle alone (no GPU).

create_proof (prover.rs:210-231) runs ifft + coset_fft on a, b and c, then
(a*b - c) / Z(g) on the coset and one icoset_fft: seven transforms.  c has degree < m, so
coset_fft followed by icoset_fft is the identity on it, and icoset_fft is linear; with
K = 1/Z(g) = 1/(g^m - 1)

    h = icoset_fft((A_cos o B_cos - C_cos) * K) = icoset_fft(A_cos o B_cos) * K - ifft(c) * K

coefficient by coefficient, exactly in Fr and for every a, b, c (not only satisfied ones).
The device pipeline (run_h_vector / run_h_final, csrc/api.hip) computes the right-hand side."""
import random

import pytest

from oracle import bellman as bm

E = bm.BLS12_381
R = E.Fr.q


def _ten_call_h(a, b, c):
    da, db, dc = (bm.EvaluationDomain(E, list(x)) for x in (a, b, c))
    for d in (da, db, dc):
        d.ifft()
        d.coset_fft()
    da.mul_assign(db)
    da.sub_assign(dc)
    da.divide_by_z_on_coset()
    da.icoset_fft()
    return da.coeffs


def _six_transform_h(a, b, c):
    da, db, dc = (bm.EvaluationDomain(E, list(x)) for x in (a, b, c))
    for d in (da, db):
        d.ifft()
        d.coset_fft()
    da.mul_assign(db)
    da.icoset_fft()
    dc.ifft()  # no coset powers, no forward transform
    k = E.Fr.inv(da.z(E.Fr.generator))
    return [(u - v) * k % R for u, v in zip(da.coeffs, dc.coeffs)]


def _inputs(m):
    rng = random.Random(0x4836 + m)
    rnd = lambda: [rng.randrange(R) for _ in range(m)]
    yield "random", rnd(), rnd(), rnd()
    for name, v in (("zero", 0), ("one", 1), ("r-1", R - 1)):
        yield name + " everywhere", [v] * m, [v] * m, [v] * m
        yield name + " as c", rnd(), rnd(), [v] * m
        yield name + " as a", [v] * m, rnd(), rnd()
    # the three special values mixed into random vectors
    a, b, c = rnd(), rnd(), rnd()
    for i, v in enumerate((0, 1, R - 1)):
        a[i], b[(i + 1) % m], c[(i + 2) % m] = v, v, v
    yield "mixed", a, b, c


@pytest.mark.parametrize("m", [8, 16])
def test_h_equals_product_transform_minus_ifft_c(m):
    for name, a, b, c in _inputs(m):
        if name == "random":
            assert any(x * y % R != z for x, y, z in zip(a, b, c)), "inputs must not satisfy a*b = c"
        want = _ten_call_h(a, b, c)
        got = _six_transform_h(a, b, c)
        assert len(want) == len(got) == m
        for i in range(m):
            assert got[i] == want[i], (name, m, i)
