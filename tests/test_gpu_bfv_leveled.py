"""GPU parity of BFV multiplication and relinearisation by HPSPOVERQLEVELED with dropped levels,
bit for bit against the CPU restatement in tests/bfv_leveled_ref.py: ExpandCRTBasisQlHat (with and
without the addend, in place), the fused ScaleAndRound + lift, the drop through the shipped
ScaleAndRound, the levelled EvalMult / EvalSquare and RelinearizeCore.  The scale-round-lift inputs
carry planted coefficients on which a fused double sum gives another floor(nu)
(tests/test_bfv_leveled_oracle.py asserts that on these very inputs).  No case faults by design;
bad arguments are CPU tests (tests/test_abi_leveled.py) except those that need live handles."""
import numpy as np
import pytest

import bfv_leveled_ref as LR
import bfv_ref as R
import bfv_tables as BT
import keyswitch as K
import leveled_cases as C
import oracle as O
from test_gpu_bfv import converter, dev, host, out_buf, stream
from test_gpu_caller_stream import OnStream, delay  # noqa: F401  (delay is a fixture)

pytestmark = pytest.mark.gpu

T_PLAIN = C.T_PLAIN


def filled(*shape):
    """an output buffer of 0xFF.. words: a store the kernel misses shows"""
    import torch

    return torch.full(shape, -1, dtype=torch.int64, device="cuda")


class Level:
    """A BfvLevel and every handle it is composed from, for towers q / r at level l"""

    def __init__(self, H, ctx, log_n, q, rq, r, rr, t, l, generic=False, full_mult=False):
        self.T = T = BT.LeveledTables(q, r, t, l)
        L = l + 1
        plan = lambda m, ro: H.NTTPlan(ctx, log_n, m, ro, generic_moduli=generic)  # noqa: E731
        self.pq, self.pql, self.prl = plan(q, rq), plan(q[:L], rq[:L]), plan(r[:L], rr[:L])
        self.pqlrl = plan(list(q[:L]) + list(r[:L]), list(rq[:L]) + list(rr[:L]))
        self.ql_to_rl, self.rl_to_ql = converter(H, ctx, log_n, T.ql, T.rl), converter(H, ctx, log_n, T.rl, T.ql)
        self.neg = H.BaseConverter(ctx, log_n, q, T.rl, T.neg_rl_q_hat_inv_modq, BT.BfvTables.flat(T.q_inv_modr))
        self.drop = H.ScaleRound(ctx, log_n, T.ql, q[L:], True, T.drop_table, T.drop_frac) if T.dropped else None
        self.sr = H.ScaleRound(ctx, log_n, T.ql, T.rl, True, T.sr_table, T.sr_frac)
        self.level = H.BfvLevel(ctx, l, self.pq, self.pql, self.prl, self.pqlrl, self.ql_to_rl, self.rl_to_ql,
                                self.neg, self.drop, self.sr, T.ql_hat_modq)
        self.mult = None
        if full_mult:  # the shipped HPSPOVERQ call over the same handles (l = size_q - 1)
            assert not T.dropped
            self.mult = H.BfvMult(ctx, H.BFV_HPSPOVERQ, self.pq, self.prl, self.pqlrl, self.ql_to_rl, self.rl_to_ql,
                                  self.neg, self.sr)

    def close(self):
        for h in (self.mult, self.level, self.sr, self.drop, self.neg, self.rl_to_ql, self.ql_to_rl, self.pqlrl,
                  self.prl, self.pql, self.pq):
            if h is not None:
                h.close()


# ---- ExpandCRTBasisQlHat -----------------------------------------------------------------------
def mixed_towers(log_n, sq):
    """sq ciphertext towers of 22 to 60 bits mixed in one chain, and as many auxiliary ones"""
    from test_mixed_moduli_oracle import mixed_chain

    bits = ([60, 22, 45, 31, 58, 50, 27, 40, 36, 54, 33, 47, 24, 59, 38, 29, 52] * 2)[:2 * sq]
    m, ro = mixed_chain(log_n, bits, generic=True)
    return m[:sq], ro[:sq], m[sq:], ro[sq:]


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("sq", [1, 4, 17])
@pytest.mark.parametrize("log_n", [1, 5, 10])
def test_expand_ql_hat(hip, log_n, sq, batch):
    """l = 0, a middle value and size_q - 1; with and without the addend and with out aliasing it;
    inputs holding 0 and q_i - 1; out pre-filled with 0xFF.. words"""
    H, ctx = hip
    n = 1 << log_n
    q, rq, r, rr = mixed_towers(log_n, sq)
    for l in sorted({0, sq // 2, sq - 1}):
        lv = Level(H, ctx, log_n, q, rq, r, rr, T_PLAIN, l, generic=True)
        T, L = lv.T, l + 1
        x = O.uniform_dcrt(batch, L, n, T.ql, 11 * l + sq)
        add = O.uniform_dcrt(batch, sq, n, q, 13 * l + sq)
        x[0, :, 0], x[0, :, n - 1] = 0, [m - 1 for m in T.ql]
        add[0, :, 0], add[0, :, n - 1] = [m - 1 for m in q], [m - 1 for m in q]
        dx = dev(x)
        out = filled(batch, sq, n)
        lv.level.expand_ql_hat(dx.data_ptr(), out.data_ptr(), 0, batch, stream())
        assert np.array_equal(host(out), LR.expand_ql_hat(x, T)), (l, "no addend")
        want = LR.expand_ql_hat(x, T, add)
        dadd, out = dev(add), filled(batch, sq, n)
        lv.level.expand_ql_hat(dx.data_ptr(), out.data_ptr(), dadd.data_ptr(), batch, stream())
        assert np.array_equal(host(out), want), (l, "addend")
        assert np.array_equal(host(dadd), add) and np.array_equal(host(dx), x)
        lv.level.expand_ql_hat(dx.data_ptr(), dadd.data_ptr(), dadd.data_ptr(), batch, stream())
        assert np.array_equal(host(dadd), want), (l, "in place")
        lv.close()


# ---- ScaleAndRound + lift in one launch ------------------------------------------------------------
@pytest.mark.parametrize("log_n,L,k", C.SR_LIFT_CASES)
def test_scale_round_expand_ql_hat(hip, log_n, L, k):
    """the fused launch against the restatement and, word for word, against scale_and_round followed
    by expand_ql_hat on the device; batch 3 and batch 1"""
    H, ctx = hip
    T, x, planted = C.sr_lift_case(log_n, L, k)
    assert planted >= 1
    n, sq = 1 << log_n, L + k
    q, rq, r, rr = C.level_chain(log_n, sq)
    lv = Level(H, ctx, log_n, q, rq, r, rr, C.SR_T, L - 1)
    want = C.cached(("srl-want", log_n, L, k), lambda: LR.scale_round_lift(x, T))
    for batch in (C.BATCH, 1):
        dx, out = dev(x[:batch]), filled(batch, sq, n)
        lv.level.scale_round_expand(dx.data_ptr(), out.data_ptr(), batch, stream())
        got = host(out)
        bad = np.argwhere(got != want[:batch])
        assert not len(bad), f"{len(bad)} words differ, first (batch, tower, coefficient) {bad[0]}"
        mid, two = filled(batch, L, n), filled(batch, sq, n)
        lv.sr.run(dx.data_ptr(), mid.data_ptr(), batch, stream())
        lv.level.expand_ql_hat(mid.data_ptr(), two.data_ptr(), 0, batch, stream())
        assert np.array_equal(host(two), got)
        assert np.array_equal(host(dx), x[:batch])
    lv.close()


# ---- the drop through the shipped ScaleAndRound ----------------------------------------------------
@pytest.mark.parametrize("log_n,sq,k", [(5, 2, 1), (10, 5, 3), (5, 17, 16), (10, 18, 1)])
def test_drop_with_level_tables(hip, log_n, sq, k):
    """ofhe_hip_scale_and_round with QlQHatInvModqDivqModq(l) / Frac(l): 1, 3 and 16 dropped towers"""
    H, ctx = hip
    n, batch = 1 << log_n, 2
    q, _, r, _ = C.level_chain(log_n, sq)
    T = BT.LeveledTables(q, r, T_PLAIN, sq - k - 1)
    x = O.uniform_dcrt(batch, sq, n, q, 40 + sq)
    x[0, :, 0], x[0, :, 1] = 0, [m - 1 for m in q]
    want = LR.drop(x, T)
    sr = H.ScaleRound(ctx, log_n, T.ql, q[T.l + 1:], True, T.drop_table, T.drop_frac)
    dx, out = dev(x), filled(batch, T.l + 1, n)
    sr.run(dx.data_ptr(), out.data_ptr(), batch, stream())
    assert np.array_equal(host(out), want)
    sr.close()


# ---- EvalMult ---------------------------------------------------------------------------------------
# (log_n, size_q, l, mixed chain): l = 0, a middle value, size_q - 2 and size_q - 1 for size_q = 2, 5, 9
# at N = 2^5 and 2^10; N = 2^13 is the smallest ring with split plans; size_q = 17 runs the negated
# converter 17 -> 1 and 17 -> 16, past the 16-source limb cap
LEVELS = {2: (0, 1), 5: (0, 2, 3, 4), 9: (0, 4, 7, 8)}
MULT_CASES = [(log_n, sq, l, False) for log_n in (5, 10, 13) for sq in (2, 5, 9) for l in LEVELS[sq]] + \
    [(5, 17, 0, False), (5, 17, 15, False), (5, 5, 0, True), (5, 5, 4, True), (10, 5, 2, True)]


def mult_case(log_n, sq, l, mixed):
    """(q, rq, r, rr, T, cts [c0, c1, d0, d1] each [3][size_q][n] uniform, want)"""
    def build():
        q, rq, r, rr = C.level_chain(log_n, sq, mixed)
        T = BT.LeveledTables(q, r, T_PLAIN, l)
        ring = LR.LevelRing(O, log_n, q, rq, r, rr, l)
        n = 1 << log_n
        cts = [O.uniform_dcrt(C.BATCH, sq, n, q, 900 + 7 * k + l) for k in range(4)]
        return q, rq, r, rr, T, cts, LR.eval_mult(O, T, ring, *cts)
    return C.cached(("mult", log_n, sq, l, mixed), build)


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("log_n,sq,l,mixed", MULT_CASES)
def test_eval_mult_leveled(hip, log_n, sq, l, mixed, batch):
    H, ctx = hip
    q, rq, r, rr, T, cts, want = mult_case(log_n, sq, l, mixed)
    n = 1 << log_n
    lv = Level(H, ctx, log_n, q, rq, r, rr, T_PLAIN, l, generic=mixed, full_mult=(l == sq - 1))
    ins = [dev(c[:batch]) for c in cts]
    outs = [filled(batch, sq, n) for _ in range(3)]
    lv.level.eval_mult(*[t.data_ptr() for t in ins + outs], batch, stream())
    got = [host(o) for o in outs]
    for k, (g, w) in enumerate(zip(got, want)):
        bad = np.argwhere(g != w[:batch])
        assert not len(bad), f"out{k}: {len(bad)} words differ, first (batch, tower, coefficient) {bad[0]}"
    for t, c in zip(ins, cts):
        assert np.array_equal(host(t), c[:batch])
    if lv.mult is not None:
        # at the full level: exactly the words of the shipped HPSPOVERQ call
        outs2 = [filled(batch, sq, n) for _ in range(3)]
        lv.mult.eval_mult(*[t.data_ptr() for t in ins + outs2], batch, stream())
        for g, o in zip(got, outs2):
            assert np.array_equal(host(o), g)
    lv.close()


@pytest.mark.parametrize("l", [0, 2, 4])
def test_eval_square_is_mult_by_itself(hip, l):
    """aliased inputs (d0 == c0, d1 == c1): EvalSquare's values"""
    H, ctx = hip
    log_n, sq, batch = 10, 5, 2
    q, rq, r, rr, T, cts, _ = mult_case(log_n, sq, 2, False)
    ring = LR.LevelRing(O, log_n, q, rq, r, rr, l)
    TL = BT.LeveledTables(q, r, T_PLAIN, l)
    c0, c1 = cts[0][:batch], cts[1][:batch]
    want = LR.eval_mult(O, TL, ring, c0, c1, c0, c1)
    lv = Level(H, ctx, log_n, q, rq, r, rr, T_PLAIN, l)
    d0, d1 = dev(c0), dev(c1)
    outs = [filled(batch, sq, 1 << log_n) for _ in range(3)]
    lv.level.eval_square(d0.data_ptr(), d1.data_ptr(), *[o.data_ptr() for o in outs], batch, stream())
    for o, w in zip(outs, want):
        assert np.array_equal(host(o), w)
    lv.close()


def test_eval_mult_leveled_on_caller_stream(hip, delay):  # noqa: F811
    """stream-ordered scratch and some twenty launches, ordered on the caller's stream alone"""
    H, ctx = hip
    log_n, sq, l, batch = 10, 5, 2, 3
    q, rq, r, rr, T, cts, want = mult_case(log_n, sq, l, False)
    lv = Level(H, ctx, log_n, q, rq, r, rr, T_PLAIN, l)
    # the converters' exact tables are uploaded on their first use (a wait on the null stream):
    # have that happen before the ordered run
    warm = [dev(c[:1]) for c in cts] + [filled(1, sq, 1 << log_n) for _ in range(3)]
    lv.level.eval_mult(*[t.data_ptr() for t in warm], 1, stream())
    run = OnStream(delay)
    ins = [run.input(c) for c in cts]
    outs = [run.output(batch, sq, 1 << log_n) for _ in range(3)]
    run.begin()
    lv.level.eval_mult(*[t.data_ptr() for t in ins + outs], batch, run.h)
    run.fetch(*outs)
    got = run.wait()
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    import torch

    torch.cuda.synchronize()
    lv.close()


def test_eval_mult_leveled_decrypts_at_every_level(hip):
    """encrypt, multiply on the device at every l, decrypt on the host with exact integers (N = 2^4)"""
    H, ctx = hip
    log_n, sq, n = 4, 4, 16
    q, rq, r, rr = C.level_chain(log_n, sq)
    tb_q = O.Tables(n, q, rq)
    rng = np.random.default_rng(77)
    s = np.array([int(v) for v in rng.integers(-1, 2, size=n)], dtype=object)
    ms = [np.array([int(v) for v in rng.integers(0, T_PLAIN, size=n)], dtype=object) for _ in range(2)]
    cts = [O.ntt_fwd(c, tb_q) for m in ms for c in LR.encrypt_coef(rng, m, s, q, T_PLAIN)]
    want = R.negacyclic(ms[0], ms[1]) % T_PLAIN
    for l in range(sq):
        lv = Level(H, ctx, log_n, q, rq, r, rr, T_PLAIN, l)
        ins = [dev(c) for c in cts]
        outs = [filled(1, sq, n) for _ in range(3)]
        lv.level.eval_mult(*[t.data_ptr() for t in ins + outs], 1, stream())
        got = [host(o) for o in outs]
        assert (R.decrypt3(got, s, q, T_PLAIN) == want).all(), l
        ring = LR.LevelRing(O, log_n, q, rq, r, rr, l)
        for g, w in zip(got, LR.eval_mult(O, lv.T, ring, *cts)):
            assert np.array_equal(g, w)
        lv.close()


# ---- RelinearizeCore ----------------------------------------------------------------------------------
_relin = {}


def relin_case():
    """N = 2^10, Q 4, P 2, dnum 2: secret, plaintexts, the two ciphertexts, a relinearisation key"""
    if not _relin:
        log_n, sq, sp, dnum = 10, 4, 2, 2
        n = 1 << log_n
        m, ro = O.moduli_chain(log_n, 2 * sq + sp)
        q, rq, r, rr, p, rp = m[:sq], ro[:sq], m[sq:2 * sq], ro[sq:2 * sq], m[2 * sq:], ro[2 * sq:]
        kp = K.KeySwitchParams(n, q, rq, p, rp, dnum)
        rng = np.random.default_rng(5)
        s = K.ternary(n, rng)
        s_obj = np.array([int(v) for v in s], dtype=object)
        s2 = R.negacyclic(s_obj, s_obj)
        kb, ka = K.keyswitch_gen(kp, [int(v) for v in s2], s, rng)
        ms = [np.array([int(v) for v in rng.integers(0, T_PLAIN, size=n)], dtype=object) for _ in range(2)]
        tb_q = O.Tables(n, q, rq)
        cts = [O.ntt_fwd(c, tb_q) for mm in ms for c in LR.encrypt_coef(rng, mm, s_obj, q, T_PLAIN)]
        _relin.update(dict(log_n=log_n, n=n, q=q, rq=rq, r=r, rr=rr, p=p, rp=rp, dnum=dnum, kp=kp, s=s_obj, ms=ms,
                           cts=cts, kb=kb, ka=ka, tb_q=tb_q))
    return _relin


@pytest.mark.parametrize("eval_form", [True, False])
@pytest.mark.parametrize("l", [0, 1, 2, 3])
def test_relinearize_leveled(hip, l, eval_form):
    """encrypt -> multiply -> relinearise (3 elements) -> ofhe_hip_bfv_decrypt gives the product; the
    words equal the restatement's; the 2-element form (a key switch of c1) equals its restatement"""
    H, ctx = hip
    c = relin_case()
    log_n, n, q, sq = c["log_n"], c["n"], c["q"], len(c["q"])
    lv = Level(H, ctx, log_n, q, c["rq"], c["r"], c["rr"], T_PLAIN, l)
    ring = LR.LevelRing(O, log_n, q, c["rq"], c["r"], c["rr"], l)
    ks = H.KeySwitch(ctx, log_n, q, c["rq"], c["p"], c["rp"], c["dnum"])
    ins = [dev(x) for x in c["cts"]]
    prod = [filled(1, sq, n) for _ in range(3)]
    lv.level.eval_mult(*[t.data_ptr() for t in ins + prod], 1, stream())
    coef = [host(o) for o in prod]  # coefficient form, as EvalMult leaves it
    elements = coef if not eval_form else [O.ntt_fwd(x, c["tb_q"]) for x in coef]
    dkb, dka = dev(c["kb"]), dev(c["ka"])
    for count in (3, 2):
        el = elements[:count]
        want = LR.relinearize(O, K, lv.T, ring, c["kp"], el, eval_form, c["kb"], c["ka"])
        d_el = [dev(x) for x in el]
        o0, o1 = filled(1, sq, n), filled(1, sq, n)
        lv.level.relinearize(ks, [t.data_ptr() for t in d_el], eval_form, dkb.data_ptr(), dka.data_ptr(),
                             o0.data_ptr(), o1.data_ptr(), 1, stream())
        assert np.array_equal(host(o0), want[0]), (count, "out0")
        assert np.array_equal(host(o1), want[1]), (count, "out1")
        for t, x in zip(d_el, el):
            assert np.array_equal(host(t), x)
        if count == 3:
            DT = BT.DecryptTables(q, T_PLAIN)
            dec = H.BfvDecrypt(ctx, log_n, DT, H.BFV_HPSPOVERQ)
            ds = dev(K.small_poly_eval([int(v) for v in c["s"]], q, c["rq"]))
            plain = out_buf(1, n)
            dec.decrypt(lv.pq, [o0.data_ptr(), o1.data_ptr()], ds.data_ptr(), plain.data_ptr(), True, 1, stream())
            want_m = R.negacyclic(c["ms"][0], c["ms"][1]) % T_PLAIN
            assert (host(plain)[0].astype(object) == want_m).all()
            dec.close()
    ks.close()
    lv.close()


def test_leveled_argument_checks(hip):
    """what needs live handles: a wrong level, mismatched handles, overlapping buffers"""
    H, ctx = hip
    log_n, sq, l, n = 3, 3, 1, 8
    q, rq, r, rr = C.level_chain(log_n, sq)
    lv = Level(H, ctx, log_n, q, rq, r, rr, T_PLAIN, l)
    T = lv.T
    mk = lambda **kw: H.BfvLevel(ctx, kw.get("l", l), lv.pq, kw.get("pql", lv.pql), lv.prl, kw.get("pqlrl", lv.pqlrl),  # noqa: E731
                                 lv.ql_to_rl, lv.rl_to_ql, kw.get("neg", lv.neg), kw.get("drop", lv.drop),
                                 kw.get("sr", lv.sr), kw.get("hat", T.ql_hat_modq))
    with pytest.raises(H.MathError, match="l must be"):
        mk(l=sq, hat=[0] * (sq + 1))
    with pytest.raises(H.MathError, match="l \\+ 1 towers"):
        mk(l=0, hat=[0])
    with pytest.raises(H.MathError, match="prefix"):
        mk(pql=lv.prl)
    swapped = H.NTTPlan(ctx, log_n, list(r[:2]) + list(q[:2]), list(rr[:2]) + list(rq[:2]))
    with pytest.raises(H.MathError, match="followed by"):
        mk(pqlrl=swapped)
    swapped.close()
    with pytest.raises(H.MathError, match="q_to_rl_neg"):
        mk(neg=lv.ql_to_rl)
    with pytest.raises(H.MathError, match="drop is NULL"):
        mk(drop=None)
    with pytest.raises(H.MathError, match="drop must have"):
        mk(drop=lv.sr)
    with pytest.raises(H.MathError, match="scale_round must have"):
        mk(sr=lv.drop)
    with pytest.raises(H.MathError, match="below its modulus"):
        mk(hat=[q[0], 0])
    other = H.Context(0)
    with pytest.raises(H.MathError, match="belong to ctx"):
        H.BfvLevel(other, l, lv.pq, lv.pql, lv.prl, lv.pqlrl, lv.ql_to_rl, lv.rl_to_ql, lv.neg, lv.drop, lv.sr,
                   T.ql_hat_modq)
    other.close()
    buf = out_buf(1, sq + 2, n)
    with pytest.raises(H.MathError, match="overlaps x"):
        lv.level.expand_ql_hat(buf.data_ptr() + 8 * n, buf.data_ptr(), 0, 1, stream())
    with pytest.raises(H.MathError, match="without being addend"):
        lv.level.expand_ql_hat(out_buf(1, 2, n).data_ptr(), buf.data_ptr(), buf.data_ptr() + 8 * n, 1, stream())
    with pytest.raises(H.MathError, match="overlaps x"):
        lv.level.scale_round_expand(buf.data_ptr(), buf.data_ptr() + 8 * n, 1, stream())
    # the handle still works
    x = O.uniform_dcrt(1, 2, n, T.ql, 1)
    out = filled(1, sq, n)
    lv.level.expand_ql_hat(dev(x).data_ptr(), out.data_ptr(), 0, 1, stream())
    assert np.array_equal(host(out), LR.expand_ql_hat(x, T))
    lv.close()
