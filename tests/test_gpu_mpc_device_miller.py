"""bh_mpc_common_verify's Miller loops on the device (the default) and on the host
(BH_MPC_HOST_MILLER=1): the same verdicts on an honest contribution, a tampered one and one whose
"mine" list holds a twist point of order 13, which makes the device loop meet a zero denominator and
hand that vector pair to the host loop.

The switch is read from the environment, so each setting runs in a fresh child process (this file
run as a script), once for both lengths; the tests read the two children's reports."""
import json
import os
import random
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENS = (5, 65)
PAIR, M2 = 576, 384  # a ParameterPair's bytes and its g2_mine offset (tests/test_gpu_mpc.py)


def _list_at(data, j):
    o = 2 * PAIR
    for _ in range(j):
        o += 4 + int.from_bytes(data[o:o + 4], "big") * PAIR
    return o + 4


def _child(order13_hex):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "bellman-mpc_amd"))
    import bellman_hip as bh
    from oracle import bls12_381 as bls
    ctx = bh.Context(0)
    full = 0x6F0E1D2C3B4A59687786A5B4C3D2E1F00112233445566778899AABBCCDDEEFF1 % bls.R
    report = {}
    for n in LENS:
        z = [3 + 2 ** 127 + 1000003 * i * i for i in range(n)]
        st = bh.initial_common_paramters(ctx, n)
        honest = bh.mpc_common_paramters_generator(ctx, st, (3, full, 5)).write()

        def verdict(data):
            c = bh.CommonParamter.read(ctx, bytes(data), checked=False)
            ok = bh.verify_common_paramter(ctx, st, c, z=z) is not None
            return [ok, bh.lib().bh_mpc_last_miller_device()]

        a_off = _list_at(honest, 1)  # alpha_mul_tau
        tampered = bytearray(honest)
        wrong = bls.g2_to_uncompressed(bls.G2.to_affine(bls.G2.mul(bls.G2.generator(), 4242)))
        tampered[a_off + (n - 2) * PAIR + M2:a_off + (n - 2) * PAIR + M2 + 192] = wrong
        degenerate = bytearray(honest)
        degenerate[a_off + (n - 1) * PAIR + M2:a_off + (n - 1) * PAIR + M2 + 192] = bytes.fromhex(order13_hex)
        report[str(n)] = {"honest": verdict(honest), "tampered": verdict(tampered), "degenerate": verdict(degenerate)}
    ctx.close()
    print("REPORT " + json.dumps(report))


if __name__ == "__main__":
    _child(sys.argv[1])
    sys.exit(0)


pytestmark = pytest.mark.gpu


def _order13_bytes():
    """a twist point of order 13 (tests/test_gpu_pairing.py shows why the loop divides by zero on it)"""
    from oracle import bls12_381 as bls
    from oracle import pairing as pr
    x = -pr.X_ABS
    h2 = (x ** 8 - 4 * x ** 7 + 5 * x ** 6 - 4 * x ** 4 + 6 * x ** 3 - 4 * x ** 2 - 4 * x + 13) // 9
    rng = random.Random(13)
    while True:
        xs = (rng.randrange(bls.P), rng.randrange(bls.P))
        ys = pr._fp2_sqrt(bls.Fp2Ops.add(bls.Fp2Ops.mul(bls.Fp2Ops.sqr(xs), xs), (4, 4)))
        if ys is None:
            continue
        q = bls.G2.to_affine(bls.G2.mul(bls.G2.from_affine((xs, ys)), bls.R * h2 // 169))
        if q is not None:
            assert bls.G2.to_affine(bls.G2.mul(bls.G2.from_affine(q), 13)) is None
            return bls.g2_to_uncompressed(q)


@pytest.fixture(scope="module")
def reports():
    point = _order13_bytes().hex()
    out = {}
    for host in (False, True):
        env = dict(os.environ)
        env.pop("BH_MPC_HOST_MILLER", None)
        if host:
            env["BH_MPC_HOST_MILLER"] = "1"
        r = subprocess.run([sys.executable, os.path.abspath(__file__), point], env=env, capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        line = [x for x in r.stdout.splitlines() if x.startswith("REPORT ")][-1]
        out[host] = json.loads(line[7:])
    return out


@pytest.mark.parametrize("n", LENS)
def test_honest_contribution_on_both_paths(reports, n):
    assert reports[False][str(n)]["honest"] == [True, 2]  # both vector pairs on the device
    assert reports[True][str(n)]["honest"] == [True, 0]


@pytest.mark.parametrize("n", LENS)
def test_tampered_mine_is_refused_on_both_paths(reports, n):
    assert reports[False][str(n)]["tampered"][0] is False
    assert reports[True][str(n)]["tampered"] == [False, 0]


@pytest.mark.parametrize("n", LENS)
def test_degenerate_mine_gets_the_host_verdict(reports, n):
    dev, host = reports[False][str(n)]["degenerate"], reports[True][str(n)]["degenerate"]
    assert dev[0] == host[0]
    # the first vector pair fell back to the host; the second runs (on the device) only after an accept
    assert dev[1] == (1 if dev[0] else 0) and host[1] == 0
