"""Runs tests/cpp_linear_transform/test_linear_transform.cpp on the GPU: the adapter's
KeySwitchHybrid::LinearTransform and the three stage methods (KeySwitchExt, MultExtSum,
FastRotationExtSum in upmem--openfhe_amd/host/ofhe_dcrt.hpp) reproduce the words the Python
reference composition (tests/linear_transform_ref.py) writes to a fixture, at N = 2^6, Q = 5,
P = 3, dnum = 2 with nbaby = 3, ngiant = 2, batch 3 and one absent diagonal."""
import os
import subprocess

import numpy as np
import pytest
from conftest import ROOT

MAGIC = 0x4C54465831


@pytest.fixture(scope="module")
def lt_bin():
    d = os.path.join(ROOT, "tests", "cpp_linear_transform")
    subprocess.run(["make", "-s", "-C", d], check=True)
    return os.path.join(d, "test_linear_transform_bin")


def test_cpp_linear_transform_builds(lt_bin):
    """The adapter members compile against the header (no device needed)."""
    assert os.access(lt_bin, os.X_OK)


def write_fixture(path):
    """The layout test_linear_transform.cpp documents; every array as little-endian u64."""
    import keyswitch as K
    import linear_transform_ref as LT
    from test_keyswitch_oracle import _bases, _uniform

    log_n, sq, sp, dnum, B, t = 6, 5, 3, 2, 3, 65537
    l, n = sq, 1 << log_n
    q, rq, p, rp = _bases(log_n, sq, sp)
    kp = K.KeySwitchParams(n, q, rq, p, rp, dnum)
    rng = np.random.default_rng(606)
    baby, giant = [1, 5, 2 * n - 1], [1, 25]
    present = [1, 1, 1, 1, 1, 0]
    nb, ng = len(baby), len(giant)
    c0, c1 = _uniform(rng, B, q, n), _uniform(rng, B, q, n)
    diag = _uniform(rng, nb * ng, q + p, n)
    key = lambda k: None if k == 1 else (_uniform(rng, dnum, q + p, n), _uniform(rng, dnum, q + p, n))  # noqa: E731
    bkeys, gkeys = [key(k) for k in baby], [key(k) for k in giant]
    out = [[MAGIC, log_n, sq, sp, dnum, l, B, nb, ng, t], q, rq, p, rp, baby, giant, present, c0, c1, diag]
    for k in bkeys + gkeys:
        out.append([0 if k is None else 1])
        if k is not None:
            out += [k[0], k[1]]
    out += list(LT.bsgs_ref(kp, c0, c1, baby, giant, bkeys, gkeys, diag, present, t))
    out.append(LT.ext_ref(kp, c0))
    r0, r1 = LT.baby_steps_ref(kp, c0, c1, baby, bkeys)
    i0, i1 = LT.mult_ext_sum_ref(kp, l, r0, r1, diag, present, ng)
    out += [r0, r1, i0, i1]
    rot = [j for j, k in enumerate(giant) if not LT.is_identity(k, n)]
    ident = [j for j, k in enumerate(giant) if LT.is_identity(k, n)]
    m1 = np.stack([K.ks_mod_down(kp, i1[j], t) for j in rot])
    digits = np.stack([K.ks_precompute(kp, x) for x in m1])
    addend = np.stack([i1[j] for j in ident])
    outer = LT.fast_rotation_ext_sum_ref(kp, digits, [giant[j] for j in rot], [gkeys[j] for j in rot], addend)
    out += [[len(rot), len(ident)], [giant[j] for j in rot], rot, m1, addend, outer[0], outer[1]]
    with open(path, "wb") as f:
        for a in out:
            f.write(np.ascontiguousarray(np.asarray(a, dtype=np.uint64)).astype("<u8").tobytes())


@pytest.mark.gpu
def test_cpp_linear_transform(lt_bin, tmp_path):
    fixture = tmp_path / "linear_transform.bin"
    write_fixture(fixture)
    r = subprocess.run([lt_bin, str(fixture)], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "linear transform: 0 failures" in r.stdout, r.stdout
