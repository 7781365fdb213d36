"""GPU parity for the fused N = 2^16 block pass with two polynomial quads per
thread (k_block NR = 2, QP = 2): set s of a wave's team tm runs polynomial
8 bo + 4 s + tm, so a batch tail can leave set 1 wholly empty (B mod 8 in
1..4), set 0 partly empty (B < 4), set 1 with one to three live teams, or a
second octet with any of these.  Fused pipeline only: the standalone forward,
inverse and forward-subtract block passes keep one quad per thread and stay
with test_gpu_block_teams.py.  Bit-exact against the oracle; 3 towers and at
most 17 polynomials (26 MiB) per case."""
import functools

import numpy as np
import pytest

import oracle as O
from test_gpu_block_teams import T, N, _chain, _pipeline, _plan, _tables
from test_gpu_parity import dev, host, stream

pytestmark = pytest.mark.gpu

BMAX = {False: 17, True: 13}  # polynomials of the special-prime and the generic-moduli cases


@functools.lru_cache(maxsize=None)
def _inputs(generic):
    """(a, b): BMAX polynomials each; a case of batch B copies the first B to the device."""
    q, _ = _chain(generic)
    return O.uniform_dcrt(BMAX[generic], T, N, q, 31), O.uniform_dcrt(BMAX[generic], T, N, q, 32)


@functools.lru_cache(maxsize=None)
def _ref(generic):
    """Oracle pipeline for all BMAX polynomials, computed once; the polynomials
    are independent, so batch B compares with the first B."""
    a, b = _inputs(generic)
    out = O.ntt_mul_intt(a, b, _tables(generic))
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("B", [1, 3, 4, 5, 7, 8, 9, 12, 13, 16, 17])
def test_pipeline_batch(hip, B):
    """set 1 empty (1, 3, 4), with set 0 partly empty (1, 3); set 1 with one
    and three live teams (5, 7); a full octet (8); the second octet's tails
    (9, 12, 13); two octets (16) and a third with one polynomial (17)"""
    a, b = _inputs(False)
    plan = _plan(hip)
    got = _pipeline(plan, a[:B], b[:B])
    plan.close()
    assert np.array_equal(got, _ref(False)[:B])


@pytest.mark.parametrize("B", [5, 13])
def test_pipeline_generic_moduli(hip, B):
    a, b = _inputs(True)
    plan = _plan(hip, generic=True)
    got = _pipeline(plan, a[:B], b[:B])
    plan.close()
    assert np.array_equal(got, _ref(True)[:B])


def test_pipeline_c_aliases_a(hip):
    a, b = _inputs(False)
    plan = _plan(hip)
    got = _pipeline(plan, a[:13], b[:13], alias=True)
    plan.close()
    assert np.array_equal(got, _ref(False)[:13])


def test_pipeline_all_q_minus_1(hip):
    """every word of a and b at q - 1: the lazy bounds' extremes in both sets"""
    q, _ = _chain(False)
    a = np.broadcast_to((np.array(q, np.uint64) - np.uint64(1))[None, :, None], (9, T, N)).copy()
    plan = _plan(hip)
    got = _pipeline(plan, a, a)
    plan.close()
    # nine equal polynomials: the oracle runs one
    want = O.ntt_mul_intt(a[:1], a[:1], _tables(False))
    assert np.array_equal(got, np.broadcast_to(want, got.shape))


def test_pipeline_stage_calls(hip):
    """the three launches one by one leave what the one-call pipeline leaves"""
    import torch

    B = 13
    a, b = _inputs(False)
    plan = _plan(hip)
    da, db = dev(a[:B]), dev(b[:B])
    dc = torch.empty_like(da)
    for st in (0, 1, 2):
        plan.ntt_mul_intt_stage(st, da.data_ptr(), db.data_ptr(), dc.data_ptr(), B, stream())
    staged = host(dc)
    one = _pipeline(plan, a[:B], b[:B])
    plan.close()
    assert np.array_equal(staged, one)
    assert np.array_equal(one, _ref(False)[:B])
