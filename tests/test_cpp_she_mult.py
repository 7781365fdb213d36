"""Runs tests/cpp_she_mult/test_she_mult.cpp on the GPU: the adapter's KeySwitchHybrid::EvalMult / EvalSquare /
Relinearize / Rescale (upmem--openfhe_amd/host/ofhe_dcrt.hpp) reproduce the words the Python restatement
(tests/she_mult_ref.py) writes to a fixture, at N = 2^12 and 2^13, for CKKS and BGV, and throw math_error on
bad arguments."""
import os
import subprocess

import numpy as np
import pytest
from conftest import ROOT

MAGIC = 0x5348454D31


@pytest.fixture(scope="module")
def she_bin():
    d = os.path.join(ROOT, "tests", "cpp_she_mult")
    subprocess.run(["make", "-s", "-C", d], check=True)
    return os.path.join(d, "test_she_mult_bin")


def test_cpp_she_mult_builds(she_bin):
    """The adapter members compile against the header (no device needed)."""
    assert os.access(she_bin, os.X_OK)


def write_fixture(path, log_n, sq, sp, dnum, l, B, scheme, t, levels):
    """The layout test_she_mult.cpp documents; every array as little-endian u64."""
    import keyswitch as K
    import she_mult_ref as S
    from test_keyswitch_oracle import _bases, _uniform

    n = 1 << log_n
    q, rq, p, rp = _bases(log_n, sq, sp)
    kp = K.KeySwitchParams(n, q, rq, p, rp, dnum)
    rng = np.random.default_rng([log_n, scheme, t])
    cv = [_uniform(rng, B, q[:l], n) for _ in range(4)]
    keys = [(_uniform(rng, dnum, q + p, n), _uniform(rng, dnum, q + p, n)) for _ in range(2)]
    out = [[MAGIC, log_n, sq, sp, dnum, l, B, scheme, t, levels], q, rq, p, rp] + cv
    out += [keys[0][0], keys[0][1], keys[1][0], keys[1][1]]
    out += list(S.eval_mult(kp, cv[0], cv[1], cv[2], cv[3], keys[0][0], keys[0][1], scheme, t, levels))
    out += list(S.eval_mult(kp, cv[0], cv[1], None, None, keys[0][0], keys[0][1], scheme, t, levels))
    out += list(S.relinearize(kp, cv, keys, t))
    out += S.rescale(kp, cv[:2], scheme, t, levels)
    with open(path, "wb") as f:
        for a in out:
            f.write(np.ascontiguousarray(np.asarray(a, dtype=np.uint64)).astype("<u8").tobytes())


@pytest.mark.gpu
@pytest.mark.parametrize("scheme,t", [(0, 0), (1, 65537)], ids=["ckks", "bgv"])
@pytest.mark.parametrize("log_n,sq,sp,dnum,l,B,levels", [(12, 4, 2, 2, 4, 2, 1), (13, 5, 2, 3, 4, 3, 2)])
def test_cpp_she_mult(she_bin, tmp_path, log_n, sq, sp, dnum, l, B, levels, scheme, t):
    fixture = tmp_path / "she_mult.bin"
    write_fixture(fixture, log_n, sq, sp, dnum, l, B, scheme, t, levels)
    r = subprocess.run([she_bin, str(fixture)], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "she mult: 0 failures" in r.stdout, r.stdout
