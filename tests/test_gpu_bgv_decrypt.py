"""GPU parity of BGV decryption and the decryption core, bit for bit against tests/bgv_decrypt_ref.py: the
ModReduce chain kernel alone on every path it takes (one launch up to BGV_CHAIN_K + 1 towers, blocked passes
past that, both endings), ofhe_hip_bgv_decrypt in both of the reference's branches, ofhe_hip_decrypt_core, and
encrypt -> BGV EvalMult with one ModReduce -> decrypt end to end."""
import numpy as np
import pytest

import bgv_decrypt_ref as G
import keyswitch as K
import oracle as O
from test_gpu_bfv import dev, host, out_buf, stream
from test_gpu_caller_stream import OnStream, delay  # noqa: F401  (delay is a fixture)

pytestmark = pytest.mark.gpu

CAP = 9  # towers one launch takes: BGV_CHAIN_K retired and one left (asserted against the binding below)
# 1, 2, 3; the cap and one past it (two launches); 18 (three launches, both scratch blocks); the handle's limit
SIZES = [1, 2, 3, CAP, CAP + 1, 2 * CAP, 64]
SMALL_Q0 = (22, 60, 45, 59, 33, 60, 28, 51)  # a 22-bit q_0 below 60-bit towers


def t_values(q):
    """2, 65537, a power of two, and the first value above every 22-bit tower that is invertible modulo the
    chain: reduced mod those towers, and on the SMALL_Q0 chains, whose q_0 is the largest of them, the
    t > q_0 case of Mod t"""
    from math import gcd

    t = max(m for m in q if m < 1 << 22) + 2
    while any(gcd(t, m) != 1 for m in q[1:]):
        t += 2
    return [2, 65537, 1 << 20, t]


_chains = {}


def chain_case(size_ql, bits=G.mixed_chain.__defaults__[0]):
    key = (size_ql, bits)
    if key not in _chains:
        _chains[key] = G.mixed_chain(size_ql, bits)
    return _chains[key]


def run_chain(H, ctx, q, t, log_n, batch, seed):
    """both endings at every size_ql the chain q allows among SIZES, from one handle"""
    n = 1 << log_n
    dec = H.BgvDecrypt(ctx, log_n, q, t)
    for size_ql in [s for s in SIZES if s <= len(q)]:
        x = G.planted(batch, q[:size_ql], n, seed + size_ql)
        dx = dev(x)
        for plain in (False, True):
            out = out_buf(batch, n)
            dec.mod_reduce_chain(size_ql, dx.data_ptr(), out.data_ptr(), plain, batch, stream())
            got, want = host(out), G.chain(x, q[:size_ql], t, plain)
            bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
            assert bad.size == 0, (size_ql, plain, bad[:8], got.reshape(-1)[bad[:8]], want.reshape(-1)[bad[:8]])
        assert np.array_equal(host(dx), x)  # the input is only read
    dec.close()


@pytest.mark.parametrize("ti", range(4), ids=["t2", "t65537", "tpow2", "tabove"])
@pytest.mark.parametrize("bits", [G.mixed_chain.__defaults__[0], SMALL_Q0], ids=["q0-45bit", "q0-22bit"])
def test_chain_every_size_and_t(hip, bits, ti):
    """N = 2^4, batch 2, towers of 22 to 60 bits ordered so that SwitchModulus meets q_i > q_j, q_i <= q_j and
    q_j > 2 q_i within one call; 0, q - 1, q >> 1, (q >> 1) + 1 planted on every tower"""
    H, ctx = hip
    assert CAP == H.BGV_CHAIN_K + 1 and SIZES[-1] == H.BGV_DECRYPT_MAX_TOWERS
    q = chain_case(64, bits)
    t = t_values(q)[ti]
    if ti == 3:
        assert t > min(q[1:]) and (t > q[0]) == (bits is SMALL_Q0)
    run_chain(H, ctx, q, t, 4, 2, 10 * ti)


@pytest.mark.parametrize("ti", [0, 3], ids=["t2", "tabove"])
def test_chain_below_one_wave(hip, ti):
    """N = 2: a grid of two threads"""
    H, ctx = hip
    q = chain_case(CAP + 1, SMALL_Q0)
    run_chain(H, ctx, q, t_values(q)[ti], 1, 1, 50 + ti)


def test_chain_ragged_grid(hip):
    """N = 2^9, batch 3: 1536 coefficients, six workgroups, in two launches"""
    H, ctx = hip
    q = chain_case(CAP + 1)
    run_chain(H, ctx, q, 65537, 9, 3, 60)


def test_chain_argument_checks(hip):
    H, ctx = hip
    q = chain_case(3)
    dec = H.BgvDecrypt(ctx, 4, q, 65537)
    x, out = dev(G.planted(1, q, 16, 1)), out_buf(1, 16)
    for size_ql, msg in ((0, "size_ql"), (4, "size_ql")):
        with pytest.raises(H.MathError, match=msg):
            dec.mod_reduce_chain(size_ql, x.data_ptr(), out.data_ptr(), True, 1, stream())
    with pytest.raises(H.MathError, match="overlaps"):
        dec.mod_reduce_chain(3, x.data_ptr(), x.data_ptr() + 16 * 8, True, 1, stream())
    with pytest.raises(H.MathError, match="aligned"):
        dec.mod_reduce_chain(3, x.data_ptr() + 8, out.data_ptr(), True, 1, stream())
    with pytest.raises(H.MathError, match="bad data"):
        dec.mod_reduce_chain(3, 0, out.data_ptr(), True, 1, stream())
    assert not host(out).any()
    dec.close()


# ---- decrypt ----------------------------------------------------------------------------------------------
T_PLAIN = 65537
_dec = {}


def decrypt_case(log_n, sq=4):
    """(q, rq, s_eval [sq][n], per size_ql: [c0, c1, c2] each [3][size_ql][n] in evaluation form): batch entry
    0 is a real encryption of 3 elements, entries 1 and 2 are uniform; the chain has 60-, 50- and 40-bit towers
    in an order that is not monotone"""
    if log_n not in _dec:
        n = 1 << log_n
        q = [O.previous_prime(O.first_prime(b, 2 * n), 2 * n) for b in (50, 60, 40, 59)][:sq]
        rq = [O.root_of_unity(2 * n, m) for m in q]
        rng = np.random.default_rng(40 + log_n)
        s = np.array([int(v) for v in rng.integers(-1, 2, size=n)], dtype=np.int64)
        s_eval = K.small_poly_eval(s, q, rq)[0]
        cts = {}
        for size_ql in (sq, sq - 1):
            ql = q[:size_ql]
            # c1, c2 uniform; c0 = m + t e - c1 s - c2 s^2 formed in evaluation form
            c1, c2 = O.uniform_dcrt(1, size_ql, n, ql, 11), O.uniform_dcrt(1, size_ql, n, ql, 12)
            m = rng.integers(0, T_PLAIN, size=n)
            v = K.small_poly_eval(m + T_PLAIN * rng.integers(-3, 4, size=n), ql, rq[:size_ql])
            c0 = O.eltwise("sub", v, O.eltwise("sub", G.decrypt_core([v, c1, c2], s_eval, ql), v, ql), ql)
            cts[size_ql] = (m, [np.concatenate([c, O.uniform_dcrt(2, size_ql, n, ql, 970 + k)])
                                for k, c in enumerate((c0, c1, c2))])
        _dec[log_n] = (q, rq, s_eval, cts)
    return _dec[log_n]


def scale_to_plain(q, size_ql, t):
    f = 1
    for m in q[1:size_ql]:
        f = f * pow(int(m), -1, t) % t
    return f


@pytest.mark.parametrize("eval_form", [True, False], ids=["eval", "coef"])
@pytest.mark.parametrize("elements", [2, 3])
@pytest.mark.parametrize("log_n", [4, 11, 13])
def test_bgv_decrypt(hip, log_n, elements, eval_form):
    """against the restated branch at full and at dropped size_ql, batch 3; the 3-element real encryption of
    batch entry 0 returns m (q_1 .. q_l)^-1 mod t"""
    H, ctx = hip
    q, rq, s_eval, cts = decrypt_case(log_n)
    n, batch = 1 << log_n, 3
    plan, dec = H.NTTPlan(ctx, log_n, q, rq), H.BgvDecrypt(ctx, log_n, q, T_PLAIN)
    ds = dev(s_eval)
    for size_ql in (len(q), len(q) - 1):
        m, full = cts[size_ql]
        elems = full[:elements]
        if not eval_form:
            elems = [K.set_format(c, q[:size_ql], rq[:size_ql], False) for c in elems]
        want = G.decrypt(elems, s_eval, q, rq, T_PLAIN, eval_form)
        ins, out = [dev(c) for c in elems], out_buf(batch, n)
        dec.decrypt(plan, size_ql, [x.data_ptr() for x in ins], ds.data_ptr(), out.data_ptr(), eval_form, batch,
                    stream())
        got = host(out)
        assert np.array_equal(got, want), size_ql
        if elements == 3:
            assert np.array_equal(got[0], (m * scale_to_plain(q, size_ql, T_PLAIN) % T_PLAIN).astype(np.uint64))
        for x, c in zip(ins, elems):
            assert np.array_equal(host(x), c)
    dec.close()
    plan.close()


def test_bgv_decrypt_one_tower_and_t_two(hip):
    """size_ql = 1 (the coefficient-form branch reuses the chain kernel's ending) and t = 2, both branches"""
    H, ctx = hip
    log_n = 4
    q, rq, s_eval, cts = decrypt_case(log_n)
    n, batch = 1 << log_n, 3
    plan, ds = H.NTTPlan(ctx, log_n, q, rq), dev(s_eval)
    for t, size_ql in ((T_PLAIN, 1), (2, 1), (2, 3)):
        dec = H.BgvDecrypt(ctx, log_n, q, t)
        for eval_form in (True, False):
            elems = [np.ascontiguousarray(c[:, :size_ql]) for c in cts[3][1]]
            if not eval_form:
                elems = [K.set_format(c, q[:size_ql], rq[:size_ql], False) for c in elems]
            ins, out = [dev(c) for c in elems], out_buf(batch, n)
            dec.decrypt(plan, size_ql, [x.data_ptr() for x in ins], ds.data_ptr(), out.data_ptr(), eval_form, batch,
                        stream())
            assert np.array_equal(host(out), G.decrypt(elems, s_eval, q, rq, t, eval_form)), (t, size_ql, eval_form)
        dec.close()
    plan.close()


@pytest.mark.parametrize("eval_form", [True, False], ids=["eval", "coef"])
def test_bgv_decrypt_on_caller_stream(hip, delay, eval_form):  # noqa: F811
    """the whole call (scratch, transforms, kernels) ordered on the caller's stream alone"""
    H, ctx = hip
    log_n, batch = 11, 3
    q, rq, s_eval, cts = decrypt_case(log_n)
    elems = cts[3][1]
    if not eval_form:
        elems = [K.set_format(c, q[:3], rq[:3], False) for c in elems]
    want = G.decrypt(elems, s_eval, q, rq, T_PLAIN, eval_form)
    plan, dec = H.NTTPlan(ctx, log_n, q, rq), H.BgvDecrypt(ctx, log_n, q, T_PLAIN)
    run = OnStream(delay)
    ins, ds = [run.input(c) for c in elems], run.input(s_eval)
    out = run.output(batch, 1 << log_n)
    run.begin()
    dec.decrypt(plan, 3, [x.data_ptr() for x in ins], ds.data_ptr(), out.data_ptr(), eval_form, batch, run.h)
    run.fetch(out)
    assert np.array_equal(run.wait()[0], want)
    import torch

    torch.cuda.synchronize()
    dec.close()
    plan.close()


def test_bgv_decrypt_argument_checks(hip):
    H, ctx = hip
    log_n = 4
    q, rq, s_eval, cts = decrypt_case(log_n)
    plan, rev = H.NTTPlan(ctx, log_n, q, rq), H.NTTPlan(ctx, log_n, q[::-1], rq[::-1])
    dec = H.BgvDecrypt(ctx, log_n, q, T_PLAIN)
    x, out = dev(cts[4][1][0]), out_buf(3, 1 << log_n)
    p = x.data_ptr()
    with pytest.raises(H.MathError, match="towers"):
        dec.decrypt(rev, 4, [p, p], p, out.data_ptr(), True, 1, stream())
    with pytest.raises(H.MathError, match="2 or 3"):
        dec.decrypt(plan, 4, [p], p, out.data_ptr(), True, 1, stream())
    with pytest.raises(H.MathError, match="size_ql"):
        dec.decrypt(plan, 5, [p, p], p, out.data_ptr(), True, 1, stream())
    with pytest.raises(H.MathError, match="bad data"):
        dec.decrypt(plan, 4, [p, p, 0], p, out.data_ptr(), True, 1, stream())
    with pytest.raises(H.MathError, match="other overlap"):
        plan.decrypt_core(4, [p, p], p, p, True, False, 1, stream())
    assert not host(out).any()
    for h in (dec, rev, plan):
        h.close()


# ---- DecryptCore ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("coeff_out", [False, True], ids=["eval-out", "coeff-out"])
@pytest.mark.parametrize("log_n", [4, 13])
def test_decrypt_core(hip, log_n, coeff_out):
    """2 and 3 elements, evaluation- and coefficient-form inputs, at full and dropped size_ql, into a buffer
    of its own and into c0"""
    H, ctx = hip
    q, rq, s_eval, cts = decrypt_case(log_n)
    n, batch = 1 << log_n, 3
    plan, ds = H.NTTPlan(ctx, log_n, q, rq), dev(s_eval)
    for size_ql, elements, eval_form, in_place in ((4, 3, True, False), (4, 2, True, True), (3, 3, False, True),
                                                   (3, 2, False, False)):
        elems = cts[size_ql][1][:elements]
        if not eval_form:
            elems = [K.set_format(c, q[:size_ql], rq[:size_ql], False) for c in elems]
        want = G.decrypt_core_call(elems, s_eval, q[:size_ql], rq[:size_ql], eval_form, coeff_out)
        ins = [dev(c) for c in elems]
        out = ins[0] if in_place else out_buf(batch, size_ql, n)
        plan.decrypt_core(size_ql, [x.data_ptr() for x in ins], ds.data_ptr(), out.data_ptr(), eval_form, coeff_out,
                          batch, stream())
        assert np.array_equal(host(out), want), (size_ql, elements, eval_form, in_place)
        for x, c in list(zip(ins, elems))[1 if in_place else 0:]:
            assert np.array_equal(host(x), c)
    plan.close()


# ---- end to end -------------------------------------------------------------------------------------------
def test_encrypt_multiply_mod_reduce_decrypt(hip):
    """N = 2^10, t = 257, every q_i and p_j = 1 mod t (the choice the reference's BGV parameters make, so that
    ModReduce and ModDown leave the plaintext as it is): two host encryptions over 3 towers, the HYBRID
    EvalMult in BGV mode with levels = 1, then ofhe_hip_bgv_decrypt over the 2 towers left = the negacyclic
    product of the messages mod t"""
    H, ctx = hip
    log_n, t, sq, sp, dnum = 10, 257, 3, 2, 2
    n = 1 << log_n
    m_ = 2 * n * t
    q = [O.previous_prime(O.first_prime(50, m_), m_)]
    q += [O.previous_prime(q[-1], m_)]
    q += [O.previous_prime(q[-1], m_)]
    p = [O.previous_prime(O.first_prime(60, m_), m_)]
    p += [O.previous_prime(p[-1], m_)]
    assert all(x % t == 1 for x in q + p)
    rq, rp = [O.root_of_unity(2 * n, x) for x in q], [O.root_of_unity(2 * n, x) for x in p]
    kp = K.KeySwitchParams(n, q, rq, p, rp, dnum)
    rng = np.random.default_rng(77)
    s = K.ternary(n, rng)
    s_obj = np.array([int(v) for v in s], dtype=object)
    s2 = np.array([int(v) for v in G.negacyclic(s_obj, s_obj)], dtype=np.int64)
    kb, ka = K.keyswitch_gen(kp, s2, s, rng, err_bound=0)
    # the key's error, a multiple of t: kb += t e
    for part in range(kb.shape[0]):
        te = K.small_poly_eval(t * rng.integers(-3, 4, size=n), q + p, rq + rp)
        kb[part] = O.eltwise("add", np.ascontiguousarray(kb[part][None]), te, q + p)[0]
    s_eval = K.small_poly_eval(s, q, rq)
    ms, cts = [], []
    for k in range(2):
        m = rng.integers(0, t, size=n)
        a = O.uniform_dcrt(1, sq, n, q, 300 + k)
        v = K.small_poly_eval(m + t * rng.integers(-3, 4, size=n), q, rq)
        cts += [O.eltwise("sub", v, O.eltwise("mul", a, s_eval, q), q), a]
        ms.append(np.array([int(x) for x in m], dtype=object))
    ks = H.KeySwitch(ctx, log_n, q, rq, p, rp, dnum)
    plan, dec = H.NTTPlan(ctx, log_n, q, rq), H.BgvDecrypt(ctx, log_n, q, t)
    d = [dev(c) for c in cts]
    dkb, dka, ds = dev(kb), dev(ka), dev(s_eval[0])
    o0, o1, plain = out_buf(1, sq - 1, n), out_buf(1, sq - 1, n), out_buf(1, n)
    ks.eval_mult(sq, *[x.data_ptr() for x in d], dkb.data_ptr(), dka.data_ptr(), o0.data_ptr(), o1.data_ptr(),
                 H.SHE_BGV, t, 1, 1, stream())
    dec.decrypt(plan, sq - 1, [o0.data_ptr(), o1.data_ptr()], ds.data_ptr(), plain.data_ptr(), True, 1, stream())
    want = (G.negacyclic(ms[0], ms[1]) % t).astype(np.uint64)
    assert np.array_equal(host(plain)[0], want)
    for h in (dec, plan, ks):
        h.close()
