"""Seeded randomized parity of the ops built on the transforms: the rescaling
callers (DropLastElementAndScale, ModReduce), BV key switching with
digitSize = 0 and the HYBRID key-switch engine with its creation options,
bit-exact against oracle/keyswitch.py.

tests/test_gpu_fuzz.py sweeps the plan ops, the base conversion and
ApproxModUp / ApproxModDown; this file sweeps their callers the same way.
The draws live in tests/tier2_cases.py (plain data, no GPU): ring dimensions
2^1 .. 2^17, levels below the plan's tower count, distinct moduli of 22 (key
switch: 30) to 60 bits of mixed size and form, every valid plan split,
generic_moduli, in place / padded strides, and for the key switch dnum, level,
t, batch and the options chunk, single_stream, separate_cols, separate_icol.
tests/test_tier2_cases.py checks on the CPU that the committed seed ranges
reach every SwitchModulus branch, every ring-size class and split, beta = 1 ..
>= 5, ragged chunks and the options at N = 2^17.  Inputs are edge-heavy (0, 1,
q - 1, and q/2, q/2 + 1 in the tower that is switched).  Two fixed key-switch
shapes follow that do not depend on the draw: batch 5 in chunks of 2, and
single_stream = 1, at N = 2^13 and N = 2^17 (12 + 4 towers, dnum 3)."""
from functools import lru_cache

import numpy as np
import pytest

import keyswitch as K
import tier2_cases as C
from test_gpu_fuzz import _edge_inputs
from test_gpu_parity import dev, host, stream
from test_mixed_moduli_oracle import mixed_chain

pytestmark = pytest.mark.gpu


def _half_words(rng, x, tower, q):
    """q/2 and q/2 + 1 (SwitchModulus's sign boundary) at random places of one tower."""
    n = x.shape[2]
    for val in (q // 2, q // 2 + 1):
        for b in range(x.shape[0]):
            x[b, tower, rng.integers(0, n, size=max(1, n // 8))] = val
    return x


def _msg(c):
    return ", ".join(f"{k} {v}" for k, v in c.items() if k not in ("r", "rq", "rp", "special", "data_seed"))


@pytest.mark.parametrize("seed", range(C.SEEDS["rescale"] * C.SCALE))
def test_fuzz_rescale(hip, seed):
    import torch

    H, ctx = hip
    c = C.case("rescale", seed)
    log_n, T, Bn, ev = c["log_n"], c["towers"], c["batch"], c["eval_form"]
    n = 1 << log_n
    q, r = c["q"][:T], c["r"][:T]
    rng = np.random.default_rng(c["data_seed"])
    # edge words in coefficient form, so that in evaluation form they are what SwitchModulus sees after the
    # op's inverse transform of the dropped tower (the other towers' words enter the arithmetic as they are)
    x = _half_words(rng, _edge_inputs(rng, Bn, q, n), T - 1, q[-1])
    if ev:
        x[:, T - 1:] = K.set_format(x[:, T - 1:], q[-1:], r[-1:], True)
    cc, a = K.rescale_tables(q)
    if c["op"] == "drop_last":
        want = K.drop_last_and_scale(x, q, r, ev, cc, a)
    else:
        negtinv = (-pow(c["t"], -1, q[-1])) % q[-1]
        want = K.mod_reduce(x, q, r, ev, c["t"], negtinv, a)
    plan = H.NTTPlan(ctx, log_n, c["q"], c["r"], split=getattr(H, c["split"]), generic_moduli=bool(c["generic_moduli"]))
    # the input's stride carries the pad too, so that in place (equal strides) sees it as well
    xs = (T + c["pad"]) * n
    dx = torch.zeros((Bn, T + c["pad"], n), dtype=torch.int64, device="cuda")
    dx[:, :T] = dev(x)
    if c["in_place"]:
        out, os_, OT = dx, xs, T + c["pad"]
    else:
        OT = T - 1 + c["pad"]
        out, os_ = torch.zeros((Bn, OT, n), dtype=torch.int64, device="cuda"), OT * n
    if c["op"] == "drop_last":
        plan.drop_last_and_scale(T, dx.data_ptr(), xs, out.data_ptr(), os_, ev, cc, a, Bn, stream())
    else:
        plan.mod_reduce(T, dx.data_ptr(), xs, out.data_ptr(), os_, ev, c["t"], negtinv, a, Bn, stream())
    got = host(out)
    assert np.array_equal(got[:, :T - 1], want), _msg(c)
    if not c["in_place"]:
        assert not got[:, T - 1:].any(), "pad written: " + _msg(c)
        assert np.array_equal(host(dx)[:, :T], x), "input changed: " + _msg(c)
    elif c["pad"]:
        assert not got[:, T:].any(), "pad written: " + _msg(c)
    plan.close()


@pytest.mark.parametrize("seed", range(C.SEEDS["bv"] * C.SCALE))
def test_fuzz_bv(hip, seed):
    import torch

    H, ctx = hip
    c = C.case("bv", seed)
    log_n, T, TK, Bn = c["log_n"], c["towers"], c["plan_towers"], c["batch"]
    n = 1 << log_n
    qa, ra = c["q"], c["r"]
    q, rq = qa[:T], ra[:T]
    rng = np.random.default_rng(c["data_seed"])
    coef = _edge_inputs(rng, Bn, q, n)
    for t in range(T):
        _half_words(rng, coef, t, q[t])
    x = K.set_format(coef, q, rq, True)
    kb, ka = _edge_inputs(rng, T, qa, n), _edge_inputs(rng, T, qa, n)
    want_d = K.crt_decompose0(x, q, rq)
    want0, want1 = K.bv_fast_core(want_d, kb, ka, q)
    plan = H.NTTPlan(ctx, log_n, qa, ra, split=getattr(H, c["split"]), generic_moduli=bool(c["generic_moduli"]))
    dc = dev(x)
    dd = torch.zeros((Bn, T, T, n), dtype=torch.int64, device="cuda")
    plan.bv_precompute(T, dc.data_ptr(), dd.data_ptr(), Bn, stream())
    assert np.array_equal(host(dd), want_d), "precompute: " + _msg(c)
    dkb, dka = dev(kb), dev(ka)
    o0 = torch.zeros((Bn, T, n), dtype=torch.int64, device="cuda")
    o1 = torch.zeros_like(o0)
    plan.bv_core(T, dd.data_ptr(), dkb.data_ptr(), dka.data_ptr(), TK, o0.data_ptr(), o1.data_ptr(), Bn, stream())
    assert np.array_equal(host(o0), want0) and np.array_equal(host(o1), want1), "core: " + _msg(c)
    plan.close()


def _ks_options(H, c):
    opt = H.KsOptions()
    opt.plan = H.PlanOptions(getattr(H, c["split"]), c["generic_moduli"])
    opt.separate_cols, opt.separate_icol = c["separate_cols"], c["separate_icol"]
    opt.chunk, opt.single_stream = c["chunk"], c["single_stream"]
    return opt


def _ks_check(ks, kp, l, t, x, kb, ka, want, msg):
    """precompute, fast_core_ext, mod_down and core of one engine against the
    oracle's steps (want: digits, ct0, ct1, out0, out1)."""
    import torch

    Bn, n, sp = x.shape[0], x.shape[2], len(kp.p)
    wd, w0, w1, r0, r1 = want
    dc, dkb, dka = dev(x), dev(kb), dev(ka)
    d = torch.zeros((Bn, kp.beta(l), l + sp, n), dtype=torch.int64, device="cuda")
    ks.precompute(l, dc.data_ptr(), d.data_ptr(), Bn, stream())
    assert np.array_equal(host(d), wd), "precompute: " + msg
    c0 = torch.zeros((Bn, l + sp, n), dtype=torch.int64, device="cuda")
    c1 = torch.zeros_like(c0)
    ks.fast_core_ext(l, d.data_ptr(), dkb.data_ptr(), dka.data_ptr(), c0.data_ptr(), c1.data_ptr(), Bn, stream())
    assert np.array_equal(host(c0), w0) and np.array_equal(host(c1), w1), "fast_core_ext: " + msg
    o0 = torch.zeros((Bn, l, n), dtype=torch.int64, device="cuda")
    o1 = torch.zeros_like(o0)
    ks.mod_down(l, c0.data_ptr(), o0.data_ptr(), t, Bn, stream())
    ks.mod_down(l, c1.data_ptr(), o1.data_ptr(), t, Bn, stream())
    assert np.array_equal(host(o0), r0) and np.array_equal(host(o1), r1), "mod_down: " + msg
    o0.zero_()
    o1.zero_()
    ks.core(l, dc.data_ptr(), dkb.data_ptr(), dka.data_ptr(), o0.data_ptr(), o1.data_ptr(), t, Bn, stream())
    assert np.array_equal(host(o0), r0) and np.array_equal(host(o1), r1), "core: " + msg
    assert np.array_equal(host(dc), x), "core changed its input: " + msg


def _ks_oracle(kp, x, kb, ka, t):
    wd = K.ks_precompute(kp, x)
    w0, w1 = K.ks_fast_core_ext(kp, wd, kb, ka)
    return wd, w0, w1, K.ks_mod_down(kp, w0, t), K.ks_mod_down(kp, w1, t)


@pytest.mark.parametrize("seed", range(C.SEEDS["keyswitch"] * C.SCALE))
def test_fuzz_keyswitch(hip, seed):
    H, ctx = hip
    c = C.case("keyswitch", seed)
    log_n, l, Bn = c["log_n"], c["level"], c["batch"]
    n = 1 << log_n
    q, rq, p, rp = c["q"], c["rq"], c["p"], c["rp"]
    kp = K.KeySwitchParams(n, q, rq, p, rp, c["dnum"])
    rng = np.random.default_rng(c["data_seed"])
    x = _edge_inputs(rng, Bn, q[:l], n)
    kb, ka = _edge_inputs(rng, c["dnum"], q + p, n), _edge_inputs(rng, c["dnum"], q + p, n)
    want = _ks_oracle(kp, x, kb, ka, c["t"])
    ks = H.KeySwitch(ctx, log_n, q, rq, p, rp, c["dnum"], _ks_options(H, c))
    assert ks.digits(l) == (kp.alpha, c["beta"])
    _ks_check(ks, kp, l, c["t"], x, kb, ka, want, _msg(c))
    ks.close()


# --- fixed shapes: chunked batches and the single-stream engine ------------------
FIXED_BITS = [60, 45, 50, 40, 55, 59, 48, 52, 58, 42, 57, 44, 60, 59, 58, 60]  # 12 Q towers, 4 P towers
FIXED_DNUM, FIXED_B = 3, 5


@lru_cache(maxsize=1)
def _fixed_ref(log_n, l):
    n = 1 << log_n
    m, r = mixed_chain(log_n, FIXED_BITS)
    q, rq, p, rp = m[:12], r[:12], m[12:], r[12:]
    kp = K.KeySwitchParams(n, q, rq, p, rp, FIXED_DNUM)
    rng = np.random.default_rng(500 + log_n + l)
    x = _edge_inputs(rng, FIXED_B, q[:l], n)
    kb, ka = _edge_inputs(rng, FIXED_DNUM, q + p, n), _edge_inputs(rng, FIXED_DNUM, q + p, n)
    return kp, x, kb, ka, _ks_oracle(kp, x, kb, ka, 0)


@pytest.mark.parametrize("log_n,level,option", [(log_n, level, option) for log_n in (13, 17) for level in (12, 9)
                                                for option in ("chunk2", "single_stream")])  # one reference per pair
def test_keyswitch_chunked_and_single_stream(hip, log_n, level, option):
    """Batch 5 through ModUp in chunks of 2 (2 + 2 + 1: the ragged last chunk
    and the chunk's pointer offsets into c and the digits), and the engine
    without side streams, at N = 2^13 (unfused conversion) and N = 2^17 with
    12 + 4 towers and dnum 3 (k_bconv_cols at full level; the unfused kernels
    one digit lower)."""
    H, ctx = hip
    kp, x, kb, ka, want = _fixed_ref(log_n, level)
    opt = H.KsOptions()
    if option == "chunk2":
        opt.chunk = 2
    else:
        opt.single_stream = 1
    ks = H.KeySwitch(ctx, log_n, kp.q, kp.rq, kp.p, kp.rp, FIXED_DNUM, opt)
    _ks_check(ks, kp, level, 0, x, kb, ka, want, f"{option} log_n {log_n} level {level}")
    ks.close()
