"""Runs tests/cpp_bv/test_bv.cpp: the adapter's KeySwitchBV (upmem--openfhe_amd/host/ofhe_dcrt.hpp) reproduces
on the GPU the words the Python restatement (tests/bv_digits_ref.py) writes to a fixture, at N = 2^12 and 2^13,
for digitSize 0 and 20, and throws math_error on bad arguments; with no device, KeySwitchBV::DigitCount agrees
with the binding's bv_digit_count and the restatement on chains of 22 - 60 bits."""
import os
import subprocess

import numpy as np
import pytest
from conftest import ROOT

MAGIC, MAGIC_COUNT = 0x4256444947, 0x4256434E54


@pytest.fixture(scope="module")
def bv_bin():
    d = os.path.join(ROOT, "tests", "cpp_bv")
    subprocess.run(["make", "-s", "-C", d], check=True)
    return os.path.join(d, "test_bv_bin")


def _write(path, arrays):
    with open(path, "wb") as f:
        for a in arrays:
            f.write(np.ascontiguousarray(np.asarray(a, dtype=np.uint64)).astype("<u8").tobytes())


def test_cpp_bv_builds(bv_bin):
    """The adapter class compiles against the header (no device needed)."""
    assert os.access(bv_bin, os.X_OK)


def test_digit_count_agrees_with_the_adapter(bv_bin, tmp_path):
    """Python (the binding's device-free function and the restatement) against KeySwitchBV::DigitCount."""
    import bv_digits_ref as R
    import ofhe_hip as H
    from test_mixed_moduli_oracle import mixed_chain

    cases = []
    for bits in ([60, 59, 59, 30, 45], [22, 23, 31, 32, 60], [29, 30, 58], [40, 22]):
        for generic in (False, True):
            q, _ = mixed_chain(6, bits, generic)
            assert [m.bit_length() for m in q] == bits
            for r in (0, 1, 7, 29, 30):
                for towers in {1, len(q) - 1, len(q)}:
                    want = R.digit_count(q[:towers], r)
                    assert want == H.bv_digit_count(q[:towers], r)
                    cases.append([len(q), towers, r, want] + list(q))
    path = tmp_path / "count.bin"
    _write(path, [[MAGIC_COUNT, len(cases)]] + cases)
    r = subprocess.run([bv_bin, "count", str(path)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "bv count: 0 failures" in r.stdout, r.stdout


def write_fixture(path, log_n, l, B, r):
    """The layout test_bv.cpp documents."""
    import bv_digits_ref as R
    import oracle as O
    from test_mixed_moduli_oracle import bv_chain, uniform

    n = 1 << log_n
    q, rq = bv_chain(log_n, extra=(45,))
    T = len(q)
    ql, rl = q[:l], rq[:l]
    rng = np.random.default_rng([log_n, r])
    c, a0, a1 = (uniform(rng, B, ql, n) for _ in range(3))
    nk = R.digit_count(q, r)
    kb = np.stack([uniform(rng, 1, q, n)[0] for _ in range(nk)])
    ka = np.stack([uniform(rng, 1, q, n)[0] for _ in range(nk)])
    digits = R.crt_decompose(c, ql, rl, r)
    ct0, ct1 = R.bv_fast_core_digits(digits, kb, ka, ql)
    two0, two1 = R.key_switch_in_place([a0, c], kb, ka, ql, rl, r)
    three0, three1 = R.key_switch_in_place([a0, a1, c], kb, ka, ql, rl, r)
    assert np.array_equal(two1, ct1) and np.array_equal(two0, O.eltwise("add", a0, ct0, ql))
    _write(path, [[MAGIC, log_n, T, l, B, r], q, rq, c, a0, a1, kb, ka, digits, ct0, ct1, two0, three0, three1])


@pytest.mark.gpu
@pytest.mark.parametrize("r", [0, 20])
@pytest.mark.parametrize("log_n,l,B", [(12, 4, 2), (13, 5, 1)])
def test_cpp_bv(bv_bin, tmp_path, log_n, l, B, r):
    fixture = tmp_path / "bv.bin"
    write_fixture(fixture, log_n, l, B, r)
    res = subprocess.run([bv_bin, str(fixture)], capture_output=True, text=True, timeout=300)
    print(res.stdout)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "bv: 0 failures" in res.stdout, res.stdout
