"""GPU parity for the N = 2^16 block pass (k_block NR = 2), whose waves give
their four 16-lane teams the same 256-element group of four consecutive
polynomials of the batch: every MODE of the kernel (fused pipeline, standalone
forward / inverse, ModDown's forward-subtract), special-prime and generic
moduli, and the batch sizes that leave teams of the last wave-quad empty
(batch % 4 != 0), fill one quad, a quad plus a tail, and two quads plus a tail.
Bit-exact against the oracle; at most 3 towers and 9 polynomials per case."""
import functools

import numpy as np
import pytest

import keyswitch as K
import oracle as O
from test_gpu_parity import dev, host, stream

pytestmark = pytest.mark.gpu

LOG_N, N, T, BMAX = 16, 1 << 16, 3, 9


@functools.lru_cache(maxsize=None)
def _chain(generic):
    """Three towers: the bench chain's first three (q = 2^60 - d, d < 2^32: the
    special-prime kernels), or primes = 1 mod 2^17 just above 3 * 2^58
    (2^60 - q > 2^32: the generic kernels)."""
    if not generic:
        q, r = O.moduli_chain(LOG_N, T)
        assert all((1 << 60) - x < (1 << 32) for x in q)
        return tuple(q), tuple(r)
    m = 2 << LOG_N
    q, x = [], 3 * (1 << 58) + 1
    while len(q) < T:
        x = O.next_prime(x, m)
        q.append(x)
    assert all((1 << 60) - x >= (1 << 32) and x < (1 << 60) for x in q)
    return tuple(q), tuple(O.root_of_unity(m, x) for x in q)


@functools.lru_cache(maxsize=None)
def _tables(generic):
    q, r = _chain(generic)
    return O.Tables(N, list(q), list(r))


@functools.lru_cache(maxsize=None)
def _inputs(generic):
    """(a, b): BMAX polynomials each; a case of batch B copies the first B to the device."""
    q, _ = _chain(generic)
    return O.uniform_dcrt(BMAX, T, N, q, 21), O.uniform_dcrt(BMAX, T, N, q, 22)


@functools.lru_cache(maxsize=None)
def _ref(kind, generic):
    """Oracle results for all BMAX polynomials, computed once per kind; the
    polynomials are independent, so batch B compares with the first B."""
    a, b = _inputs(generic)
    tb = _tables(generic)
    out = {"pipeline": lambda: O.ntt_mul_intt(a, b, tb), "fwd": lambda: O.ntt_fwd(a, tb),
           "inv": lambda: O.ntt_inv(a, tb)}[kind]()
    out.setflags(write=False)
    return out


def _plan(hip, generic=False):
    H, ctx = hip
    q, r = _chain(generic)
    return H.NTTPlan(ctx, LOG_N, list(q), list(r))


def _pipeline(plan, a, b, alias=False):
    import torch

    B = a.shape[0]
    da, db = dev(a), dev(b)
    dc = da if alias else torch.empty_like(da)
    plan.ntt_mul_intt(da.data_ptr(), db.data_ptr(), dc.data_ptr(), B, stream())
    return host(dc)


@pytest.mark.parametrize("B", [1, 2, 3, 4, 5, 8, 9])
def test_pipeline_batch(hip, B):
    """empty teams (1, 2, 3), a full quad (4), a quad plus a tail (5), two
    quads (8), two quads plus a tail (9)"""
    a, b = _inputs(False)
    plan = _plan(hip)
    got = _pipeline(plan, a[:B], b[:B])
    plan.close()
    assert np.array_equal(got, _ref("pipeline", False)[:B])


def test_pipeline_generic_moduli(hip):
    a, b = _inputs(True)
    plan = _plan(hip, generic=True)
    got = _pipeline(plan, a[:5], b[:5])
    plan.close()
    assert np.array_equal(got, _ref("pipeline", True)[:5])


def test_pipeline_c_aliases_a(hip):
    a, b = _inputs(False)
    plan = _plan(hip)
    got = _pipeline(plan, a[:5], b[:5], alias=True)
    plan.close()
    assert np.array_equal(got, _ref("pipeline", False)[:5])


def test_pipeline_all_q_minus_1(hip):
    """every word of a and b at q - 1: the lazy bounds' extremes"""
    q, _ = _chain(False)
    a = np.broadcast_to((np.array(q, np.uint64) - np.uint64(1))[None, :, None], (5, T, N)).copy()
    plan = _plan(hip)
    got = _pipeline(plan, a, a)
    plan.close()
    assert np.array_equal(got, O.ntt_mul_intt(a, a, _tables(False)))


def test_pipeline_stage_calls(hip):
    """the three launches one by one leave what the one-call pipeline leaves"""
    import torch

    a, b = _inputs(False)
    plan = _plan(hip)
    da, db = dev(a[:5]), dev(b[:5])
    dc = torch.empty_like(da)
    for st in (0, 1, 2):
        plan.ntt_mul_intt_stage(st, da.data_ptr(), db.data_ptr(), dc.data_ptr(), 5, stream())
    staged = host(dc)
    one = _pipeline(plan, a[:5], b[:5])
    plan.close()
    assert np.array_equal(staged, one)
    assert np.array_equal(one, _ref("pipeline", False)[:5])


@pytest.mark.parametrize("B", [3, 5])
def test_standalone_forward_inverse(hip, B):
    a, _ = _inputs(False)
    plan = _plan(hip)
    x = dev(a[:B])
    plan.forward(x.data_ptr(), B, stream())
    fwd = host(x)
    y = dev(a[:B])
    plan.inverse(y.data_ptr(), B, stream())
    inv = host(y)
    plan.close()
    assert np.array_equal(fwd, _ref("fwd", False)[:B])
    assert np.array_equal(inv, _ref("inv", False)[:B])


def test_ranged_transforms_wide_strides(hip):
    """towers [1, 3) of the plan, batch 5, source rows inside a 4-tower buffer
    and destination rows inside a 6-tower buffer (both strides larger than
    the plan's towers * N); nothing outside the range is written"""
    import torch

    B = 5
    a, _ = _inputs(False)
    plan = _plan(hip)
    for fn, kind in ((plan.forward_range, "fwd"), (plan.inverse_range, "inv")):
        src = torch.zeros((B, 4, N), dtype=torch.int64, device="cuda")
        src[:, 1:3] = dev(a[:B, 1:3])
        dst = torch.zeros((B, 6, N), dtype=torch.int64, device="cuda")
        fn(1, 2, src[:, 1].data_ptr(), dst[:, 3].data_ptr(), 4 * N, 6 * N, B, stream())
        got = host(dst)
        assert np.array_equal(got[:, 3:5], _ref(kind, False)[:B, 1:3]), kind
        assert not got[:, :3].any() and not got[:, 5:].any(), kind
    plan.close()


def test_mod_down_forward_subtract(hip):
    """ApproxModDown through the key switch, Q = 3, P = 2, batch 3: its last
    step runs in the block pass of the Q towers' forward transform"""
    import torch

    H, ctx = hip
    sq, sp, dnum, B = 3, 2, 3, 3
    m, r = O.moduli_chain(LOG_N, sq + sp)
    q, rq, p, rp = m[:sq], r[:sq], m[sq:], r[sq:]
    kp = K.KeySwitchParams(N, q, rq, p, rp, dnum)
    ks = H.KeySwitch(ctx, LOG_N, q, rq, p, rp, dnum)
    x = O.uniform_dcrt(B, sq + sp, N, q + p, 23)
    dx = dev(x)
    out = torch.empty((B, sq, N), dtype=torch.int64, device="cuda")
    ks.mod_down(sq, dx.data_ptr(), out.data_ptr(), 0, B, stream())
    got = host(out)
    ks.close()
    assert np.array_equal(got, K.ks_mod_down(kp, x, 0))
