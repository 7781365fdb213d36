"""GPU parity for the N = 2^16 forward column pass with two columns per thread
(k_tcols CPT = 2: a workgroup owns 32 columns x 256 rows, thread (h, r) holds
columns 2r and 2r + 1 and moves 16 bytes per global access; the inverse pass
keeps one column per thread and is covered with it).  The launcher takes that
kernel only when source and destination are 16-byte aligned and both batch
strides are even; any other call runs one column per thread and must leave
the same words.  Covered: the fused pipeline in one call and stage by stage,
c aliasing a, the standalone and the ranged transforms, the lazy bounds'
extremes in both column sets, generic moduli, and every way a call falls
back.  Bit-exact against the oracle; 3 towers and at most 5 polynomials per
case."""
import functools

import numpy as np
import pytest

import oracle as O
from test_gpu_block_teams import N, T, _chain, _pipeline, _plan, _tables
from test_gpu_parity import dev, host, stream

pytestmark = pytest.mark.gpu

BMAX = 5


@functools.lru_cache(maxsize=None)
def _inputs(generic):
    """(a, b): BMAX polynomials each; a case of batch B copies the first B to the device."""
    q, _ = _chain(generic)
    return O.uniform_dcrt(BMAX, T, N, q, 41), O.uniform_dcrt(BMAX, T, N, q, 42)


@functools.lru_cache(maxsize=None)
def _ref(kind, generic):
    """Oracle results for all BMAX polynomials, computed once per kind."""
    a, b = _inputs(generic)
    tb = _tables(generic)
    out = {"pipeline": lambda: O.ntt_mul_intt(a, b, tb), "fwd": lambda: O.ntt_fwd(a, tb),
           "inv": lambda: O.ntt_inv(a, tb)}[kind]()
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("B", [1, 2, 5])
def test_pipeline_batch(hip, B):
    a, b = _inputs(False)
    plan = _plan(hip)
    got = _pipeline(plan, a[:B], b[:B])
    plan.close()
    assert np.array_equal(got, _ref("pipeline", False)[:B])


def test_pipeline_stage_calls(hip):
    """the three launches one by one leave what the one-call pipeline leaves"""
    import torch

    a, b = _inputs(False)
    plan = _plan(hip)
    da, db = dev(a), dev(b)
    dc = torch.empty_like(da)
    for st in (0, 1, 2):
        plan.ntt_mul_intt_stage(st, da.data_ptr(), db.data_ptr(), dc.data_ptr(), BMAX, stream())
    staged = host(dc)
    one = _pipeline(plan, a, b)
    plan.close()
    assert np.array_equal(staged, one)
    assert np.array_equal(one, _ref("pipeline", False))


def test_pipeline_c_aliases_a(hip):
    a, b = _inputs(False)
    plan = _plan(hip)
    got = _pipeline(plan, a, b, alias=True)
    plan.close()
    assert np.array_equal(got, _ref("pipeline", False))


def test_pipeline_all_q_minus_1(hip):
    """every word of a and b at q - 1: the lazy bounds' extremes in both column sets"""
    q, _ = _chain(False)
    a = np.broadcast_to((np.array(q, np.uint64) - np.uint64(1))[None, :, None], (2, T, N)).copy()
    plan = _plan(hip)
    got = _pipeline(plan, a, a)
    plan.close()
    # two equal polynomials: the oracle runs one
    want = O.ntt_mul_intt(a[:1], a[:1], _tables(False))
    assert np.array_equal(got, np.broadcast_to(want, got.shape))


@pytest.mark.parametrize("generic", [False, True])
def test_standalone_forward_inverse(hip, generic):
    """in place: each against the oracle, and inverse(forward(x)) == x"""
    B = 3
    a, _ = _inputs(generic)
    plan = _plan(hip, generic=generic)
    x = dev(a[:B])
    plan.forward(x.data_ptr(), B, stream())
    fwd = host(x)
    plan.inverse(x.data_ptr(), B, stream())
    back = host(x)
    y = dev(a[:B])
    plan.inverse(y.data_ptr(), B, stream())
    inv = host(y)
    plan.close()
    assert np.array_equal(fwd, _ref("fwd", generic)[:B])
    assert np.array_equal(inv, _ref("inv", generic)[:B])
    assert np.array_equal(back, a[:B])


def test_pipeline_generic_moduli(hip):
    a, b = _inputs(True)
    plan = _plan(hip, generic=True)
    got = _pipeline(plan, a, b)
    plan.close()
    assert np.array_equal(got, _ref("pipeline", True))


def _ranged(plan, kind, B, src_stride, dst_stride, src_off=0, dst_off=0):
    """Towers [1, 3) of the first B polynomials, out of place, through flat
    buffers: batch entry i of the source starts src_off + i * src_stride words
    into a 16-byte aligned buffer, the destination likewise.  Returns the
    [B][2][N] result and whether every other word of the destination is
    still zero."""
    import torch

    a, _ = _inputs(False)
    fn = plan.forward_range if kind == "fwd" else plan.inverse_range
    src = torch.zeros(src_off + B * src_stride, dtype=torch.int64, device="cuda")
    dst = torch.zeros(dst_off + B * dst_stride, dtype=torch.int64, device="cuda")
    assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
    rows = dev(a[:B, 1:3]).reshape(B, 2 * N)
    for i in range(B):
        src[src_off + i * src_stride:][:2 * N] = rows[i]
    fn(1, 2, src.data_ptr() + 8 * src_off, dst.data_ptr() + 8 * dst_off, src_stride, dst_stride, B, stream())
    out = host(dst)
    got = np.stack([out[dst_off + i * dst_stride:][:2 * N].reshape(2, N) for i in range(B)])
    mask = np.ones(out.shape, bool)
    for i in range(B):
        mask[dst_off + i * dst_stride:][:2 * N] = False
    return got, not out[mask].any()


@pytest.mark.parametrize("kind", ["fwd", "inv"])
def test_ranged_transforms_wide_strides(hip, kind):
    """t0 = 1, count = 2, source rows inside a 4-tower buffer and destination
    rows inside a 6-tower one; nothing outside the range is written"""
    B = 5
    plan = _plan(hip)
    got, clean = _ranged(plan, kind, B, 4 * N, 6 * N)
    plan.close()
    assert np.array_equal(got, _ref(kind, False)[:B, 1:3])
    assert clean


# (src_off, dst_off, src_stride - 4N, dst_stride - 6N): each keeps the launcher off the 16-byte kernel
FALLBACKS = {"src_off": (1, 0, 0, 0), "dst_off": (0, 1, 0, 0), "src_stride_odd": (0, 0, 1, 0),
             "dst_stride_odd": (0, 0, 0, 1)}


@pytest.mark.parametrize("kind", ["fwd", "inv"])
@pytest.mark.parametrize("case", sorted(FALLBACKS))
def test_ranged_fallback_same_words(hip, kind, case):
    """a source or destination one word past a 16-byte boundary, or an odd
    batch stride, gives the words of the aligned call"""
    B = 3
    so, do, ss, ds = FALLBACKS[case]
    plan = _plan(hip)
    want, _ = _ranged(plan, kind, B, 4 * N, 6 * N)
    got, clean = _ranged(plan, kind, B, 4 * N + ss, 6 * N + ds, so, do)
    plan.close()
    assert np.array_equal(got, want)
    assert np.array_equal(got, _ref(kind, False)[:B, 1:3])
    assert clean


def test_pipeline_fallback_a_at_odd_word(hip):
    """a one word past a 16-byte boundary: the forward column pass reads it
    with 8-byte loads, the result is the aligned call's"""
    import torch

    B = 3
    a, b = _inputs(False)
    plan = _plan(hip)
    buf = torch.zeros(1 + B * T * N, dtype=torch.int64, device="cuda")
    assert buf.data_ptr() % 16 == 0
    buf[1:] = dev(a[:B]).reshape(-1)
    db = dev(b[:B])
    dc = torch.empty_like(db)
    plan.ntt_mul_intt(buf.data_ptr() + 8, db.data_ptr(), dc.data_ptr(), B, stream())
    got = host(dc)
    plan.close()
    assert np.array_equal(got, _ref("pipeline", False)[:B])
