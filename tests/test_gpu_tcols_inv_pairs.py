"""GPU parity for the N = 2^16 inverse column pass with two columns per thread
(k_tcols_inv2: a workgroup owns 32 columns x 256 rows, thread (h, r) holds
columns 2r and 2r + 1 and moves 16 bytes per global access).  The launcher
takes it when source and destination are 16-byte aligned and both batch
strides are even; every other call, and N = 2^17, runs one column per thread
and must leave the same words.  Two towers per plan (the bench chain's
special primes, and generic moduli), batches 1, 2 and 3, plan.inverse and
ntt_mul_intt against the oracle word for word, random and all-(q - 1) inputs,
in place and out of place, each fallback, and the OFHE_TCOLS_CPT_INV=1
variant library when it has been built."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle as O
from test_gpu_parity import dev, host, stream

pytestmark = pytest.mark.gpu

LOG_N, N, T, BMAX = 16, 1 << 16, 2, 3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANT = os.path.join(ROOT, "upmem--openfhe_amd", "lib", "variants", "libofhe_hip_cptinv1.so")


@functools.lru_cache(maxsize=None)
def _chain(generic, log_n=LOG_N):
    """Two towers: q = 2^60 - d with d < 2^32 (the special-prime kernel), or
    primes just above 3 * 2^58 (2^60 - q > 2^32: the generic kernel)."""
    if not generic:
        q, r = O.moduli_chain(log_n, T)
        assert all((1 << 60) - x < (1 << 32) for x in q)
        return tuple(q), tuple(r)
    m = 2 << log_n
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
def _inputs(generic, extreme):
    """(a, b): BMAX polynomials each, uniform or with every word at q - 1."""
    q, _ = _chain(generic)
    if extreme:
        a = np.broadcast_to((np.array(q, np.uint64) - np.uint64(1))[None, :, None], (BMAX, T, N)).copy()
        return a, a
    return O.uniform_dcrt(BMAX, T, N, q, 51), O.uniform_dcrt(BMAX, T, N, q, 52)


@functools.lru_cache(maxsize=None)
def _ref(kind, generic, extreme):
    """Oracle result, computed once per (kind, chain, input): the polynomials
    are independent (all equal when extreme, where the oracle runs one)."""
    a, b = _inputs(generic, extreme)
    n = 1 if extreme else BMAX
    tb = _tables(generic)
    out = O.ntt_mul_intt(a[:n], b[:n], tb) if kind == "pipeline" else O.ntt_inv(a[:n], tb)
    if extreme:
        out = np.broadcast_to(out, (BMAX, T, N)).copy()
    out.setflags(write=False)
    return out


def _plan(hip, generic):
    H, ctx = hip
    q, r = _chain(generic)
    return H.NTTPlan(ctx, LOG_N, list(q), list(r))


CASES = [(g, e) for g in (False, True) for e in (False, True)]
IDS = [("generic" if g else "special") + ("-qm1" if e else "-random") for g, e in CASES]


@pytest.mark.parametrize("B", [1, 2, 3])
@pytest.mark.parametrize("generic,extreme", CASES, ids=IDS)
def test_inverse_in_place(hip, generic, extreme, B):
    a, _ = _inputs(generic, extreme)
    plan = _plan(hip, generic)
    x = dev(a[:B])
    plan.inverse(x.data_ptr(), B, stream())
    got = host(x)
    plan.close()
    assert np.array_equal(got, _ref("inv", generic, extreme)[:B])


def _inverse_range(plan, a, B, src_stride, dst_stride, dst_off=0):
    """plan.inverse_range of all T towers, out of place through flat 16-byte
    aligned buffers: batch entry i of the destination starts dst_off +
    i * dst_stride words in.  Returns the [B][T][N] result and whether every
    other word of the destination is still zero."""
    import torch

    src = torch.zeros(B * src_stride, dtype=torch.int64, device="cuda")
    dst = torch.zeros(dst_off + B * dst_stride, dtype=torch.int64, device="cuda")
    assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
    rows = dev(a[:B]).reshape(B, T * N)
    for i in range(B):
        src[i * src_stride:][:T * N] = rows[i]
    plan.inverse_range(0, T, src.data_ptr(), dst.data_ptr() + 8 * dst_off, src_stride, dst_stride, B, stream())
    out = host(dst)
    got = np.stack([out[dst_off + i * dst_stride:][:T * N].reshape(T, N) for i in range(B)])
    mask = np.ones(out.shape, bool)
    for i in range(B):
        mask[dst_off + i * dst_stride:][:T * N] = False
    return got, not out[mask].any()


# (dst_off, src_stride - T N, dst_stride - T N); the last three keep the launcher off the 16-byte kernel
LAYOUTS = {"dense": (0, 0, 0), "wide_even": (0, 2, 4), "dst_off_8_bytes": (1, 0, 0), "src_stride_odd": (0, 1, 0),
           "dst_stride_odd": (0, 0, 1)}


@pytest.mark.parametrize("B", [1, 2, 3])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("generic,extreme", CASES, ids=IDS)
def test_inverse_out_of_place_and_fallbacks(hip, generic, extreme, layout, B):
    """the two-column kernel (dense, wide_even) and each fallback leave the oracle's words and nothing else"""
    do, ss, ds = LAYOUTS[layout]
    a, _ = _inputs(generic, extreme)
    plan = _plan(hip, generic)
    got, clean = _inverse_range(plan, a, B, T * N + ss, T * N + ds, do)
    plan.close()
    assert np.array_equal(got, _ref("inv", generic, extreme)[:B])
    assert clean


@pytest.mark.parametrize("B", [1, 2, 3])
@pytest.mark.parametrize("alias", [False, True], ids=["out_of_place", "in_place"])
@pytest.mark.parametrize("generic,extreme", CASES, ids=IDS)
def test_pipeline(hip, generic, extreme, alias, B):
    import torch

    a, b = _inputs(generic, extreme)
    plan = _plan(hip, generic)
    da, db = dev(a[:B]), dev(b[:B])
    dc = da if alias else torch.empty_like(da)
    plan.ntt_mul_intt(da.data_ptr(), db.data_ptr(), dc.data_ptr(), B, stream())
    got = host(dc)
    plan.close()
    assert np.array_equal(got, _ref("pipeline", generic, extreme)[:B])


@pytest.mark.parametrize("generic", [False, True], ids=["special", "generic"])
def test_pipeline_fallback_c_at_odd_word(hip, generic):
    """c one word past a 16-byte boundary: the inverse column pass runs one column per thread, same words"""
    import torch

    B = 3
    a, b = _inputs(generic, False)
    plan = _plan(hip, generic)
    da, db = dev(a[:B]), dev(b[:B])
    buf = torch.zeros(1 + B * T * N, dtype=torch.int64, device="cuda")
    assert buf.data_ptr() % 16 == 0
    plan.ntt_mul_intt(da.data_ptr(), db.data_ptr(), buf.data_ptr() + 8, B, stream())
    out = host(buf)
    plan.close()
    assert out[0] == 0
    assert np.array_equal(out[1:].reshape(B, T, N), _ref("pipeline", generic, False)[:B])


_CHILD = r"""
import sys
import numpy as np
sys.path[:0] = [{pkg!r}, {tests!r}]
import torch
import ofhe_hip as H
H.LIB_PATH = {lib!r}
d = np.load({inp!r})
ctx = H.Context(0)
out = {{}}
for g in (0, 1):
    plan = H.NTTPlan(ctx, 16, [int(x) for x in d["q%d" % g]], [int(x) for x in d["r%d" % g]])
    x = torch.from_numpy(d["a%d" % g].view(np.int64)).cuda()
    plan.inverse(x.data_ptr(), x.shape[0], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    out["inv%d" % g] = x.cpu().numpy().view(np.uint64)
    plan.close()
ctx.close()
np.savez({outp!r}, **out)
"""


@pytest.mark.skipif(not os.path.exists(VARIANT), reason="make variant V=cptinv1 D=-DOFHE_TCOLS_CPT_INV=1 not built")
def test_one_column_variant_library_same_words(hip, tmp_path):
    """the OFHE_TCOLS_CPT_INV=1 build, loaded in a process of its own, leaves the same words"""
    inp, outp = str(tmp_path / "in.npz"), str(tmp_path / "out.npz")
    arrays = {}
    for g in (0, 1):
        q, r = _chain(bool(g))
        arrays.update({f"q{g}": np.array(q, np.uint64), f"r{g}": np.array(r, np.uint64),
                       f"a{g}": _inputs(bool(g), False)[0]})
    np.savez(inp, **arrays)
    code = _CHILD.format(pkg=os.path.join(ROOT, "upmem--openfhe_amd"), tests=os.path.dirname(__file__), lib=VARIANT,
                         inp=inp, outp=outp)
    subprocess.run([sys.executable, "-c", code], check=True, timeout=120)
    res = np.load(outp)
    for g in (0, 1):
        assert np.array_equal(res[f"inv{g}"], _ref("inv", bool(g), False))


def test_n17_keeps_one_column_per_thread(hip):
    """N = 2^17 (no two-column kernel exists there): inverse and pipeline against the oracle"""
    H, ctx = hip
    n = 1 << 17
    q, r = _chain(False, 17)
    tb = O.Tables(n, list(q), list(r))
    a, b = O.uniform_dcrt(1, T, n, q, 53), O.uniform_dcrt(1, T, n, q, 54)
    plan = H.NTTPlan(ctx, 17, list(q), list(r))
    x = dev(a)
    plan.inverse(x.data_ptr(), 1, stream())
    inv = host(x)
    da, db = dev(a), dev(b)
    plan.ntt_mul_intt(da.data_ptr(), db.data_ptr(), da.data_ptr(), 1, stream())
    pipe = host(da)
    plan.close()
    assert np.array_equal(inv, O.ntt_inv(a, tb))
    assert np.array_equal(pipe, O.ntt_mul_intt(a, b, tb))
