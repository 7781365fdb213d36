"""GPU parity of BFV decryption and TimesQovert, bit for bit against
tests/decrypt_ref.py: ofhe_hip_bfv_decrypt_scale_round in all eight loops A-H
of the reference, under BEHZ and on the one-tower path, ofhe_hip_bfv_decrypt
and ofhe_hip_times_q_over_t, and encrypt -> EvalMult -> decrypt end to end
under HPS and BEHZ.  The scale-round inputs are decrypt_ref's cases: a real
encryption, planted coefficients on the rounding boundaries (on which
tests/test_bfv_decrypt_oracle.py asserts that a fused multiply-add chain gives
another output) and uniform towers."""
import copy

import numpy as np
import pytest

import behz_ref as Z
import bfv_ref as BR
import bfv_tables as BT
import decrypt_ref as D
import oracle as O
from test_gpu_bfv import dev, host, out_buf, stream
from test_gpu_caller_stream import OnStream, delay  # noqa: F401  (delay is a fixture)

pytestmark = pytest.mark.gpu


def run_scale_round(H, ctx, k, technique, want):
    T, n, batch = k["T"], k["n"], k["batch"]
    dec = H.BfvDecrypt(ctx, k["log_n"], T, technique)
    dx, out = dev(k["x"]), out_buf(batch, n)
    dec.scale_round(dx.data_ptr(), out.data_ptr(), batch, stream())
    got, branch = host(out), dec.branch
    assert np.array_equal(host(dx), k["x"])  # the input is only read
    dec.close()
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    assert bad.size == 0, (bad[:8], got.reshape(-1)[bad[:8]], want.reshape(-1)[bad[:8]])
    return branch


@pytest.mark.parametrize("c", D.HPS_CASES, ids=[D.case_id(c) for c in D.HPS_CASES])
def test_scale_round_every_loop(hip, c):
    """every loop A-H with 2 and 5 towers at N = 2^8, batch 3; G through sizeQMSB; 17 and 33 towers; a
    grid below one workgroup (N = 2) and sixteen workgroups per batch entry (N = 2^12)"""
    H, ctx = hip
    k = D.hps_case(O, c)
    technique = H.BFV_HPSPOVERQ if c[3] == 5 else H.BFV_HPS  # the HPS family shares the loops
    branch = run_scale_round(H, ctx, k, technique, D.scale_round(k["x"], k["T"]))
    assert BT.BRANCHES[branch] == c[0]


@pytest.mark.parametrize("c", D.BEHZ_CASES, ids=[D.case_id(c) for c in D.BEHZ_CASES])
def test_scale_round_behz(hip, c):
    H, ctx = hip
    k = D.behz_case(O, c)
    assert run_scale_round(H, ctx, k, H.BFV_BEHZ, D.scale_round_behz(k["x"], k["T"])) == H.BFV_DECRYPT_BEHZ


@pytest.mark.parametrize("behz", [False, True])
@pytest.mark.parametrize("c", D.ONE_TOWER_CASES, ids=[D.case_id(c) for c in D.ONE_TOWER_CASES])
def test_scale_round_one_tower(hip, c, behz):
    """MultiplyAndRound + SwitchModulus under either technique; x = q >> 1, (q >> 1) + 1, 0, q - 1 included"""
    H, ctx = hip
    k = D.one_tower_case(O, c)
    T = k["T"]
    want = D.one_tower(k["x"], T.q[0], T.t)
    assert run_scale_round(H, ctx, k, H.BFV_BEHZ if behz else H.BFV_HPS, want) == H.BFV_DECRYPT_ONE_TOWER


@pytest.mark.parametrize("towers", [1, 5])
def test_times_q_over_t(hip, towers):
    """against the restatement at N = 2^8, batch 3, on 0, t - 1, q_i - 1 and uniform words; then in place"""
    H, ctx = hip
    log_n, batch, t = 8, 3, 65537
    n = 1 << log_n
    q = D.towers_below(O, log_n, 60, towers)
    T = BT.DecryptTables(q, t)
    rng = np.random.default_rng(80 + towers)
    x = np.stack([np.stack([rng.integers(0, m, size=n, dtype=np.uint64) for m in q]) for _ in range(batch)])
    x[0, :, 0], x[0, :, 1], x[0, :, 2] = 0, t - 1, [m - 1 for m in q]
    x[2, :, n - 1] = [m - 1 for m in q]
    want = D.times_q_over_t(x, T)
    dec = H.BfvDecrypt(ctx, log_n, T)
    dx, out = dev(x), out_buf(batch, towers, n)
    dec.times_q_over_t(dx.data_ptr(), out.data_ptr(), batch, stream())
    assert np.array_equal(host(out), want) and np.array_equal(host(dx), x)
    dec.times_q_over_t(dx.data_ptr(), dx.data_ptr(), batch, stream())
    assert np.array_equal(host(dx), want)
    dec.close()


# ---- decrypt ----------------------------------------------------------------------------------
T_PLAIN = 65537
_dec_cache = {}


def secret(rng, n, q, tb):
    s = np.array([int(v) for v in rng.integers(-1, 2, size=n)], dtype=object)
    return s, O.ntt_fwd(BR.residues(s.reshape(1, n), q), tb)[0]


def decrypt_case(log_n, sq=3):
    """(T, roots, tb, s_eval, plaintext, [c0, c1, c2] each [3][Q][n] evaluation form): batch entry 0 is a real
    encryption (c2 = 0 there, so it decrypts with 2 and with 3 elements), entries 1 and 2 uniform"""
    if log_n not in _dec_cache:
        n = 1 << log_n
        q, rq = O.moduli_chain(log_n, sq)
        tb = O.Tables(n, q, rq)
        rng = np.random.default_rng(90 + log_n)
        s, s_eval = secret(rng, n, q, tb)
        m = np.array([int(v) for v in rng.integers(0, T_PLAIN, size=n)], dtype=object)
        cts = list(BR.encrypt(O, rng, m, s, q, tb, T_PLAIN)) + [np.zeros((1, sq, n), dtype=np.uint64)]
        cts = [np.concatenate([c, O.uniform_dcrt(2, sq, n, q, 970 + k)]) for k, c in enumerate(cts)]
        _dec_cache[log_n] = (BT.DecryptTables(q, T_PLAIN), rq, tb, s_eval, m, cts)
    return _dec_cache[log_n]


@pytest.mark.parametrize("behz", [False, True])
@pytest.mark.parametrize("eval_form", [True, False])
@pytest.mark.parametrize("elements", [2, 3])
@pytest.mark.parametrize("log_n", [10, 13])
def test_bfv_decrypt(hip, log_n, elements, eval_form, behz):
    """against the restated composition, and against the plaintext for batch entry 0"""
    H, ctx = hip
    T, rq, tb, s_eval, m, cts = decrypt_case(log_n)
    n, batch, sq = 1 << log_n, 3, len(T.q)
    elems = cts[:elements] if eval_form else [O.ntt_inv(c, tb) for c in cts[:elements]]
    want = D.decrypt(O, elems, s_eval, T, tb, eval_form, behz)
    plan = H.NTTPlan(ctx, log_n, T.q, rq)
    dec = H.BfvDecrypt(ctx, log_n, T, H.BFV_BEHZ if behz else H.BFV_HPS)
    ins, ds, out = [dev(c) for c in elems], dev(s_eval), out_buf(batch, n)
    dec.decrypt(plan, [t.data_ptr() for t in ins], ds.data_ptr(), out.data_ptr(), eval_form, batch, stream())
    got = host(out)
    assert np.array_equal(got, want)
    assert (got[0] % np.uint64(T.t) == m.astype(np.uint64)).all()
    for t, c in zip(ins, elems):
        assert np.array_equal(host(t), c)
    assert sq == 3
    dec.close()
    plan.close()


def test_bfv_decrypt_on_caller_stream(hip, delay):  # noqa: F811
    """the whole call (scratch, transforms, three kernels) ordered on the caller's stream alone"""
    H, ctx = hip
    log_n, batch = 10, 3
    T, rq, tb, s_eval, m, cts = decrypt_case(log_n)
    coef = [O.ntt_inv(c, tb) for c in cts]
    want = D.decrypt(O, coef, s_eval, T, tb, False)
    plan = H.NTTPlan(ctx, log_n, T.q, rq)
    dec = H.BfvDecrypt(ctx, log_n, T)
    run = OnStream(delay)
    ins = [run.input(c) for c in coef]
    ds = run.input(s_eval)
    out = run.output(batch, 1 << log_n)
    run.begin()
    dec.decrypt(plan, [t.data_ptr() for t in ins], ds.data_ptr(), out.data_ptr(), False, batch, run.h)
    run.fetch(out)
    got = run.wait()[0]
    assert np.array_equal(got, want)
    import torch

    torch.cuda.synchronize()
    dec.close()
    plan.close()


# ---- end to end -------------------------------------------------------------------------------
def device_encrypt(H, dec, plan, rng, m, s, q, tb):
    """bfv_ref.encrypt with the message scaled on the device: c0 = TimesQovert(m) + e - a s, c1 = a, evaluation
    form.  TimesQovert(m) is ceil(Q m / t) where bfv_ref.encrypt uses floor(Q / t) m."""
    n, sq = len(m), len(q)
    dm = dev(BR.residues(m.reshape(1, n), q))
    dec.times_q_over_t(dm.data_ptr(), dm.data_ptr(), 1, stream())
    scaled = BR.crt_lift(host(dm), q)[0]
    Q = BT.product(q)
    assert all(int(v) == -(-Q * int(mi) // T_PLAIN) for v, mi in zip(scaled[:16], m[:16]))
    a = np.array([int(rng.integers(0, 1 << 62)) * (1 << 62) + int(rng.integers(0, 1 << 62)) for _ in range(n)],
                 dtype=object) % Q
    e = np.array([int(v) for v in rng.integers(-3, 4, size=n)], dtype=object)
    c0 = (scaled + e - BR.negacyclic(a, s)) % Q
    enc = lambda v: O.ntt_fwd(BR.residues(v.reshape(1, n), q), tb)  # noqa: E731
    assert sq == plan.towers
    return enc(c0), enc(a)


@pytest.mark.parametrize("behz", [False, True])
def test_encrypt_multiply_decrypt(hip, behz):
    """N = 2^10, t = 65537: encrypt (message scaled by the device TimesQovert), EvalMult, device decrypt of
    the 3 elements = the negacyclic product of the plaintexts mod t"""
    H, ctx = hip
    log_n, sq, t = 10, 4, T_PLAIN
    n = 1 << log_n
    rng = np.random.default_rng(123 + behz)
    if behz:
        q, rq = O.moduli_chain(log_n, sq)
        b, msk, _ = Z.behz_bases(O, log_n, q, t)
        TB = BT.BehzTables(q, b, msk, t)
        ring = Z.Ring(O, log_n, TB, rq)
        mult, plans = H.Behz(ctx, log_n, TB), [H.NTTPlan(ctx, log_n, q, rq), H.NTTPlan(ctx, log_n, TB.bsk, ring.rbsk),
                                               H.NTTPlan(ctx, log_n, q + TB.bsk, rq + ring.rbsk)]
        handles = [mult] + plans
        tb_q = ring.tb_q
    else:
        m_, r_ = O.moduli_chain(log_n, 2 * sq + 1)
        q, rq, r, rr = m_[:sq], r_[:sq], m_[sq:], r_[sq:]
        TH = BT.BfvTables(q, r, t, BT.HPS)
        plans = [H.NTTPlan(ctx, log_n, q, rq), H.NTTPlan(ctx, log_n, r, rr), H.NTTPlan(ctx, log_n, q + r, rq + rr)]
        conv = [H.BaseConverter(ctx, log_n, q, r, BT.hat_inv(q), BT.BfvTables.flat(BT.hat_mod(q, r))),
                H.BaseConverter(ctx, log_n, r, q, BT.hat_inv(r), BT.BfvTables.flat(BT.hat_mod(r, q)))]
        sr = H.ScaleRound(ctx, log_n, q, r, TH.out_is_q, TH.sr_table, TH.sr_frac)
        mult = H.BfvMult(ctx, H.BFV_HPS, plans[0], plans[1], plans[2], conv[0], conv[1], None, sr)
        handles = [mult, sr] + conv + plans
        tb_q = O.Tables(n, q, rq)
    T = BT.DecryptTables(q, t)
    dec = H.BfvDecrypt(ctx, log_n, T, H.BFV_BEHZ if behz else H.BFV_HPS)
    s, s_eval = secret(rng, n, q, tb_q)
    ms = [np.array([int(v) for v in rng.integers(0, t, size=n)], dtype=object) for _ in range(2)]
    cts = [dev(c) for m in ms for c in device_encrypt(H, dec, plans[0], rng, m, s, q, tb_q)]
    outs = [out_buf(1, sq, n) for _ in range(3)]
    ptrs = [x.data_ptr() for x in cts + outs]
    if behz:
        mult.eval_mult(*plans, *ptrs, 1, stream())
    else:
        mult.eval_mult(*ptrs, 1, stream())
    ds, plain = dev(s_eval), out_buf(1, n)
    dec.decrypt(plans[0], [o.data_ptr() for o in outs], ds.data_ptr(), plain.data_ptr(), False, 1, stream())
    got = host(plain)[0] % np.uint64(t)
    assert (got == (BR.negacyclic(ms[0], ms[1]) % t).astype(np.uint64)).all()
    for h in [dec] + handles:
        h.close()


def test_decrypt_argument_checks(hip):
    """the calls refuse a plan that does not match, a wrong element count and NULL data, and leave the
    output untouched; TimesQovert is refused on a handle created without its tables"""
    H, ctx = hip
    log_n = 4
    n = 1 << log_n
    q, rq = O.moduli_chain(log_n, 2)
    T = BT.DecryptTables(q, T_PLAIN)
    dec = H.BfvDecrypt(ctx, log_n, T)
    plan, rev = H.NTTPlan(ctx, log_n, q, rq), H.NTTPlan(ctx, log_n, q[::-1], rq[::-1])
    x, out = dev(O.uniform_dcrt(1, 2, n, q, 5)), out_buf(1, n)
    p = x.data_ptr()
    with pytest.raises(H.MathError, match="towers"):
        dec.decrypt(rev, [p, p], p, out.data_ptr(), True, 1, stream())
    with pytest.raises(H.MathError, match="2 or 3"):
        dec.decrypt(plan, [p], p, out.data_ptr(), True, 1, stream())
    with pytest.raises(H.MathError, match="bad data"):
        dec.decrypt(plan, [p, p, 0], p, out.data_ptr(), True, 1, stream())
    with pytest.raises(H.MathError, match="bad data"):
        dec.scale_round(0, out.data_ptr(), 1, stream())
    assert not host(out).any()
    bare_tables = copy.copy(T)
    bare_tables.tInvModq = bare_tables.negQModt = None
    bare = H.BfvDecrypt(ctx, log_n, bare_tables)
    with pytest.raises(H.MathError, match="without tInvModq"):
        bare.times_q_over_t(p, p, 1, stream())
    for h in (bare, rev, plan, dec):
        h.close()
