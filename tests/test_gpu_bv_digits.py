"""GPU parity for BV key switching with a digit size (ofhe_hip_bv_digit_count,
ofhe_hip_bv_precompute_digits, ofhe_hip_bv_core_digits, ofhe_hip_bv_key_switch)
through the C ABI, bit-exact against tests/bv_digits_ref.py (pinned by the
identities of tests/test_bv_digits_oracle.py; "parity unpinned" against
reference-run data, none exists for this path).  The cases and what they reach
are in tests/bv_digit_cases.py and tests/test_bv_digit_cases.py."""
import numpy as np
import pytest

import bv_digit_cases as C
import bv_digits_ref as R
import keyswitch as K
import oracle as O
from test_gpu_parity import dev, host, stream
from test_mixed_moduli_oracle import mixed_chain

pytestmark = pytest.mark.gpu


def _empty(*shape):
    import torch

    return torch.empty(shape, dtype=torch.int64, device="cuda")


def _run_case(hip, ref, r, split="SPLIT_AUTO", forced=False):
    """digit count, the decomposition, the inner product and the one-call key switch of one case."""
    H, ctx = hip
    qa, ra, q = ref["qa"], ref["ra"], ref["q"]
    B, T, n = ref["c"].shape
    TK, nd = len(qa), ref["n_digits"]
    log_n = n.bit_length() - 1
    plan = H.NTTPlan(ctx, log_n, qa, ra, split=getattr(H, split), generic_moduli=forced)
    try:
        assert plan.bv_digit_count(T, r) == nd == H.bv_digit_count(q, r)
        dc, dkb, dka = dev(ref["c"]), dev(ref["kb"]), dev(ref["ka"])
        dd = _empty(B, nd, T, n)
        plan.bv_precompute_digits(T, r, dc.data_ptr(), dd.data_ptr(), B, stream())
        assert np.array_equal(host(dd), ref["digits"])
        o0, o1 = _empty(B, T, n), _empty(B, T, n)
        plan.bv_core_digits(T, nd, dd.data_ptr(), dkb.data_ptr(), dka.data_ptr(), TK, o0.data_ptr(), o1.data_ptr(), B,
                            stream())
        assert np.array_equal(host(o0), ref["ct0"]) and np.array_equal(host(o1), ref["ct1"])
        k0, k1 = _empty(B, T, n), _empty(B, T, n)
        plan.bv_key_switch(T, r, dc.data_ptr(), dkb.data_ptr(), dka.data_ptr(), TK, 0, 0, k0.data_ptr(),
                           k1.data_ptr(), 2, B, stream())
        assert np.array_equal(host(k0), ref["ct0"]) and np.array_equal(host(k1), ref["ct1"])
        assert np.array_equal(host(dc), ref["c"])
    finally:
        plan.close()


@pytest.mark.parametrize("log_n,split", C.LAUNCH_PATHS, ids=[f"{a}-{b}" for a, b in C.LAUNCH_PATHS])
def test_launch_paths(hip, log_n, split):
    _run_case(hip, C.reference(*C.launch_args(log_n)), C.LAUNCH_R, split)


@pytest.mark.parametrize("log_n,r,form,towers", C.DIGIT_SIZES, ids=["-".join(map(str, c)) for c in C.DIGIT_SIZES])
def test_digit_sizes(hip, log_n, r, form, towers):
    """r = 1, 13, 29, 30 on bv_chain, at the top level and one level down on five-tower keys."""
    _run_case(hip, C.reference(log_n, r, form, towers), r, forced=C.FORMS[form][2])


@pytest.mark.parametrize("B", C.CHUNK_BATCHES)
def test_every_chunking(hip, B):
    """bv_key_switch = bv_precompute_digits + bv_core_digits + the additions, for every chunking, with both
    addends, with add1 = NULL and in place; once from a caller's own stream."""
    import torch

    H, ctx = hip
    log_n, r, form, T = C.CHUNK_CASE
    ref = C.reference(log_n, r, form, T, B)
    qa, ra, q = ref["qa"], ref["ra"], ref["q"]
    n, TK, nd = 1 << log_n, len(qa), ref["n_digits"]
    rng = np.random.default_rng(5)
    a0, a1 = C.uniform(rng, B, q, n), C.uniform(rng, B, q, n)
    plan = H.NTTPlan(ctx, log_n, qa, ra)
    dc, dkb, dka, da0, da1 = dev(ref["c"]), dev(ref["kb"]), dev(ref["ka"]), dev(a0), dev(a1)
    # the separate calls on the device, and the restatement's additions
    dd, o0, o1 = _empty(B, nd, T, n), _empty(B, T, n), _empty(B, T, n)
    plan.bv_precompute_digits(T, r, dc.data_ptr(), dd.data_ptr(), B, stream())
    plan.bv_core_digits(T, nd, dd.data_ptr(), dkb.data_ptr(), dka.data_ptr(), TK, o0.data_ptr(), o1.data_ptr(), B,
                        stream())
    assert np.array_equal(host(o0), ref["ct0"]) and np.array_equal(host(o1), ref["ct1"])
    want0 = O.eltwise("add", a0, host(o0), q)
    want1 = O.eltwise("add", a1, host(o1), q)
    w3_0, w3_1 = R.key_switch_in_place([a0, a1, ref["c"]], ref["kb"], ref["ka"], q, ref["rq"], r)
    w2_0, w2_1 = R.key_switch_in_place([a0, ref["c"]], ref["kb"], ref["ka"], q, ref["rq"], r)
    assert np.array_equal(want0, w3_0) and np.array_equal(want1, w3_1)
    assert np.array_equal(want0, w2_0) and np.array_equal(host(o1), w2_1)
    for chunk in C.chunkings(nd):
        k0, k1 = _empty(B, T, n), _empty(B, T, n)
        plan.bv_key_switch(T, r, dc.data_ptr(), dkb.data_ptr(), dka.data_ptr(), TK, da0.data_ptr(), da1.data_ptr(),
                           k0.data_ptr(), k1.data_ptr(), chunk, B, stream())
        assert np.array_equal(host(k0), want0) and np.array_equal(host(k1), want1), chunk
        plan.bv_key_switch(T, r, dc.data_ptr(), dkb.data_ptr(), dka.data_ptr(), TK, da0.data_ptr(), 0,
                           k0.data_ptr(), k1.data_ptr(), chunk, B, stream())
        assert np.array_equal(host(k0), want0) and np.array_equal(host(k1), w2_1), chunk
        # in place: the addends are the outputs (three elements), then c itself is out1 (two elements)
        i0, i1 = dev(a0), dev(a1)
        plan.bv_key_switch(T, r, dc.data_ptr(), dkb.data_ptr(), dka.data_ptr(), TK, i0.data_ptr(), i1.data_ptr(),
                           i0.data_ptr(), i1.data_ptr(), chunk, B, stream())
        assert np.array_equal(host(i0), want0) and np.array_equal(host(i1), want1), chunk
        i0, ic = dev(a0), dev(ref["c"])
        plan.bv_key_switch(T, r, ic.data_ptr(), dkb.data_ptr(), dka.data_ptr(), TK, i0.data_ptr(), 0, i0.data_ptr(),
                           ic.data_ptr(), chunk, B, stream())
        assert np.array_equal(host(i0), want0) and np.array_equal(host(ic), w2_1), chunk
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    k0, k1 = _empty(B, T, n), _empty(B, T, n)
    with torch.cuda.stream(side):
        plan.bv_key_switch(T, r, dc.data_ptr(), dkb.data_ptr(), dka.data_ptr(), TK, da0.data_ptr(), da1.data_ptr(),
                           k0.data_ptr(), k1.data_ptr(), 4, B, side.cuda_stream)
    side.synchronize()
    assert np.array_equal(host(k0), want0) and np.array_equal(host(k1), want1)
    plan.close()


def test_more_than_256_digits(hip):
    """r = 1 on six towers (298 digits) at N = 2^6: all-(q - 1) digits and keys, the largest sums the fold
    meets, through bv_core_digits under every setting of the inner product; then one real decomposition."""
    H, ctx = hip
    log_n, T = C.MANY_LOG_N, len(C.MANY_BITS)
    n = 1 << log_n
    q, rq = mixed_chain(log_n, C.MANY_BITS)
    nd = R.digit_count(q, 1)
    assert nd == 298
    plan = H.NTTPlan(ctx, log_n, q, rq)
    qm = np.array(q, np.uint64)[None, :, None] - np.uint64(1)
    try:
        for B in (1, 3):
            big = np.broadcast_to(qm[:, None], (B, nd, T, n)).copy()
            keys = np.broadcast_to(qm, (nd, T, n)).copy()
            want0, want1 = R.bv_fast_core_digits(big, keys, keys, q)
            dbig, dkey = dev(big), dev(keys)
            for nb in (1, 2, 4, 0):
                H.bv_tune(nb)
                o0, o1 = _empty(B, T, n), _empty(B, T, n)
                plan.bv_core_digits(T, nd, dbig.data_ptr(), dkey.data_ptr(), dkey.data_ptr(), T, o0.data_ptr(),
                                    o1.data_ptr(), B, stream())
                assert np.array_equal(host(o0), want0) and np.array_equal(host(o1), want1), (B, nb)
    finally:
        H.bv_tune(0)
    ref = C.reference(log_n, 1, "special30", T, 2, False, tuple(C.MANY_BITS))
    assert ref["n_digits"] == nd
    _run_case(hip, ref, 1)
    plan.close()


def test_key_stationary_settings_give_the_same_words(hip):
    """The key-stationary inner product (2 and 4 batch entries per thread) against the plain loop, with a short
    last group (batch 3 and 5) and through the accumulating chunks of the one-call key switch."""
    H, ctx = hip
    log_n, r, form, T = C.CHUNK_CASE
    try:
        for B in (3, 5):
            ref = C.reference(log_n, r, form, T, B)
            n, TK = 1 << log_n, len(ref["qa"])
            plan = H.NTTPlan(ctx, log_n, ref["qa"], ref["ra"])
            dc, dkb, dka = dev(ref["c"]), dev(ref["kb"]), dev(ref["ka"])
            for nb in (2, 4):
                H.bv_tune(nb)
                k0, k1 = _empty(B, T, n), _empty(B, T, n)
                plan.bv_key_switch(T, r, dc.data_ptr(), dkb.data_ptr(), dka.data_ptr(), TK, 0, 0, k0.data_ptr(),
                                   k1.data_ptr(), 4, B, stream())
                assert np.array_equal(host(k0), ref["ct0"]) and np.array_equal(host(k1), ref["ct1"]), (B, nb)
            plan.close()
    finally:
        H.bv_tune(0)


@pytest.mark.parametrize("log_n", [10, 13])
def test_digit_size_zero_is_the_existing_calls(hip, log_n):
    H, ctx = hip
    ref = C.reference(log_n, 0, "special30", 4)
    qa, ra = ref["qa"], ref["ra"]
    B, T, n = ref["c"].shape
    TK = len(qa)
    plan = H.NTTPlan(ctx, log_n, qa, ra)
    assert plan.bv_digit_count(T, 0) == T
    dc, dkb, dka = dev(ref["c"]), dev(ref["kb"]), dev(ref["ka"])
    old_d, new_d = _empty(B, T, T, n), _empty(B, T, T, n)
    plan.bv_precompute(T, dc.data_ptr(), old_d.data_ptr(), B, stream())
    plan.bv_precompute_digits(T, 0, dc.data_ptr(), new_d.data_ptr(), B, stream())
    assert np.array_equal(host(old_d), host(new_d)) and np.array_equal(host(new_d), ref["digits"])
    outs = [_empty(B, T, n) for _ in range(6)]
    p = [o.data_ptr() for o in outs]
    plan.bv_core(T, old_d.data_ptr(), dkb.data_ptr(), dka.data_ptr(), TK, p[0], p[1], B, stream())
    plan.bv_core_digits(T, T, new_d.data_ptr(), dkb.data_ptr(), dka.data_ptr(), TK, p[2], p[3], B, stream())
    plan.bv_key_switch(T, 0, dc.data_ptr(), dkb.data_ptr(), dka.data_ptr(), TK, 0, 0, p[4], p[5], 0, B, stream())
    for k in (2, 4):
        assert np.array_equal(host(outs[0]), host(outs[k])) and np.array_equal(host(outs[1]), host(outs[k + 1]))
    assert np.array_equal(host(outs[0]), ref["ct0"])
    plan.close()


def test_semantic_identities_on_device_outputs(hip):
    """Real keys at N = 2^12, T = 4, r = 10: ct0 + ct1 s_new = c s_old - sum_d digit_d e_d exactly, and the
    centred error is the small integer polynomial sum_d D_d e_d (identities (c), (d) of the oracle test)."""
    H, ctx = hip
    log_n, T, r, E = 12, 4, 10, 3
    n = 1 << log_n
    q, rq = O.moduli_chain(log_n, T)
    rng = np.random.default_rng(23)
    c = C.uniform(rng, 1, q, n)
    s_old = K.small_poly_eval(rng.integers(-1, 2, size=n), q, rq)[0]
    s_new = K.small_poly_eval(rng.integers(-1, 2, size=n), q, rq)[0]
    kb, ka, es, _ = R.bv_keygen_digits(q, rq, s_old, s_new, r, rng, E)
    nd = R.digit_count(q, r)
    plan = H.NTTPlan(ctx, log_n, q, rq)
    dc, dkb, dka = dev(c), dev(kb), dev(ka)
    dd, o0, o1 = _empty(1, nd, T, n), _empty(1, T, n), _empty(1, T, n)
    plan.bv_precompute_digits(T, r, dc.data_ptr(), dd.data_ptr(), 1, stream())
    plan.bv_key_switch(T, r, dc.data_ptr(), dkb.data_ptr(), dka.data_ptr(), T, 0, 0, o0.data_ptr(), o1.data_ptr(), 0,
                       1, stream())
    d = host(dd)
    lhs = O.eltwise("add", host(o0), O.eltwise("mul", host(o1), s_new[None], q), q)
    noise = O.eltwise("mul", d[:, 0], es[0:1], q)
    for i in range(1, nd):
        noise = O.eltwise("add", noise, O.eltwise("mul", d[:, i], es[i:i + 1], q), q)
    cs = O.eltwise("mul", c, s_old[None], q)
    assert np.array_equal(lhs, O.eltwise("sub", cs, noise, q))
    err = K.crt_centered(K.set_format(O.eltwise("sub", cs, lhs, q), q, rq, False)[0], q)
    assert max(abs(v) for v in err) <= nd * n * ((1 << r) - 1) * E
    plan.close()


def test_plan_dependent_argument_rules(hip):
    H, ctx = hip
    q, rq = O.moduli_chain(10, 3)
    plan = H.NTTPlan(ctx, 10, q, rq)
    n = 1 << 10
    x = _empty(2, 3, 3, n)
    o0, o1 = _empty(1, 3, n), _empty(1, 3, n)
    with pytest.raises(H.MathError):
        plan.bv_digit_count(4, 10)
    with pytest.raises(H.MathError):
        plan.bv_digit_count(0, 10)
    with pytest.raises(H.MathError):  # more digits than the towers have at digit_size = 1
        plan.bv_core_digits(3, H.bv_digit_count(q, 1) + 1, x.data_ptr(), x.data_ptr(), x.data_ptr(), 3,
                            o0.data_ptr(), o1.data_ptr(), 1, stream())
    with pytest.raises(H.MathError):  # digits overlapping an output
        plan.bv_core_digits(3, 3, x.data_ptr(), x.data_ptr(), x.data_ptr(), 3, o0.data_ptr(),
                            x.data_ptr() + 8 * n, 1, stream())
    plan.close()
