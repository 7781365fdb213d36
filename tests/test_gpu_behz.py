"""GPU parity of the BFV (BEHZ) calls against tests/behz_ref.py (exact
integers): ofhe_hip_behz_q_to_bsk / _expand / _floor / _conv_sk / _floor_sk and
ofhe_hip_bfv_eval_mult_behz.  Every comparison is bit-exact.  The inputs are
behz_ref.case's; tests/test_behz_oracle.py asserts on the same draws that they
reach every branch (the planted Montgomery remainders and alphas, both signs,
a tower below msk / 2)."""
import copy

import numpy as np
import pytest

import behz_ref as Z
import bfv_ref as BR
import bfv_tables as BT
import oracle as O
from test_gpu_bfv import dev, host, out_buf, stream
from test_gpu_caller_stream import OnStream, delay  # noqa: F401  (delay is a fixture)

pytestmark = pytest.mark.gpu

KAT = Z.load_vectors()
NAMES = [c[0] for c in Z.CASES]
_want = {}


def want(name, which):
    """the reference output of one case, computed once; the batch-1 run uses entry 0"""
    key = (name, which)
    if key not in _want:
        c = Z.case(O, name)
        fn, x = {"q_to_bsk": (Z.q_to_bsk, c["xq"]), "floor": (Z.floor_q, c["xqb"]), "sk": (Z.conv_sk, c["xb"])}[which]
        _want[key] = fn(x, c["T"], fast=c["fast"])
    return _want[key]


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("name", NAMES)
def test_behz_standalone_calls(hip, name, batch):
    """the three single-launch calls on every shape of behz_ref.CASES"""
    H, ctx = hip
    c = Z.case(O, name)
    T, n = c["T"], c["n"]
    Q, K = len(T.q), len(T.bsk)
    bz = H.Behz(ctx, c["log_n"], T)
    for which, x, towers, call in (("q_to_bsk", c["xq"], K, bz.q_to_bsk), ("floor", c["xqb"], K, bz.floor),
                                   ("sk", c["xb"], Q, bz.conv_sk)):
        dx, out = dev(x[:batch]), out_buf(batch, towers, n)
        call(dx.data_ptr(), out.data_ptr(), batch, stream())
        assert np.array_equal(host(out), want(name, which)[:batch]), which
        assert np.array_equal(host(dx), x[:batch]), which  # the input is only read
    bz.close()


def kat_handles(H, ctx):
    T = BT.BehzTables(KAT["q"], KAT["bsk"][:-1], KAT["bsk"][-1], KAT["t"])
    ring = Z.Ring(O, KAT["log_n"], T)
    return T, ring, H.NTTPlan(ctx, KAT["log_n"], T.q, ring.rq), H.NTTPlan(ctx, KAT["log_n"], T.bsk, ring.rbsk)


def test_behz_expand_known_answer(hip):
    """UnitTestBFVrnsCRTOperations.cpp:197-287 through ofhe_hip_behz_expand, evaluation-form input"""
    H, ctx = hip
    T, ring, pq, pb = kat_handles(H, ctx)
    bz = H.Behz(ctx, KAT["log_n"], T)
    x = np.array([KAT["x"]], dtype=np.uint64)
    out = out_buf(1, 5, 8)
    bz.expand(pq, pb, True, dev(x).data_ptr(), out.data_ptr(), 1, stream())
    assert np.array_equal(host(out)[0], np.array(KAT["expected"], dtype=np.uint64))
    for h in (bz, pb, pq):
        h.close()


def expand_case(log_n, sq):
    q, rq = (KAT["q"], None) if (log_n, sq) == (3, 2) else O.moduli_chain(log_n, sq)
    b, msk, _ = Z.behz_bases(O, log_n, q, Z.T_PLAIN)
    T = BT.BehzTables(q, b, msk, Z.T_PLAIN)
    return T, Z.Ring(O, log_n, T, rq)


@pytest.mark.parametrize("eval_form", [True, False])
@pytest.mark.parametrize("log_n,sq", [(3, 2), (10, 4), (13, 3)])
def test_behz_expand(hip, log_n, sq, eval_form):
    H, ctx = hip
    T, ring = expand_case(log_n, sq)
    n, batch, K = 1 << log_n, 2, len(T.bsk)
    x = O.uniform_dcrt(batch, sq, n, T.q, 60 + log_n)
    ref = Z.behz_expand(O, x, T, ring, eval_form, fast=True)
    pq, pb = H.NTTPlan(ctx, log_n, T.q, ring.rq), H.NTTPlan(ctx, log_n, T.bsk, ring.rbsk)
    bz = H.Behz(ctx, log_n, T)
    dx, out = dev(x), out_buf(batch, sq + K, n)
    bz.expand(pq, pb, eval_form, dx.data_ptr(), out.data_ptr(), batch, stream())
    assert np.array_equal(host(out), ref)
    assert np.array_equal(host(dx), x)
    for h in (bz, pb, pq):
        h.close()


@pytest.mark.parametrize("name", ["cap", "cap1", "odd", "mixed", "uneven"])
def test_behz_fused_floor_sk(hip, name):
    """floor -> SK in one launch equals the two separate calls and behz_ref: at the column cap
    (size_b = 16, N = 2^12: sixteen workgroups per batch row), one past it (the two-launch fallback
    of BEHZ_AUTO; BEHZ_FUSED is refused), and on the small, mixed and uneven shapes"""
    H, ctx = hip
    c = Z.case(O, name)
    T, n, batch = c["T"], c["n"], Z.BATCH
    Q, K = len(T.q), len(T.bsk)
    fits = len(T.b) <= H.BEHZ_FUSED_MAX_B
    assert fits == (name != "cap1")
    ref = Z.conv_sk(want(name, "floor"), T, fast=c["fast"])
    bz = H.Behz(ctx, c["log_n"], T)
    dx = dev(c["xqb"])
    mid, two = out_buf(batch, K, n), out_buf(batch, Q, n)
    bz.floor(dx.data_ptr(), mid.data_ptr(), batch, stream())
    bz.conv_sk(mid.data_ptr(), two.data_ptr(), batch, stream())
    assert np.array_equal(host(two), ref)
    for mode in (H.BEHZ_TWO_LAUNCHES, H.BEHZ_AUTO) + ((H.BEHZ_FUSED,) if fits else ()):
        out = out_buf(batch, Q, n)
        bz.floor_sk(dx.data_ptr(), out.data_ptr(), batch, stream(), fused=mode)
        assert np.array_equal(host(out), ref), mode
    if not fits:
        out = out_buf(batch, Q, n)
        with pytest.raises(H.MathError, match="too many B towers"):
            bz.floor_sk(dx.data_ptr(), out.data_ptr(), batch, stream(), fused=H.BEHZ_FUSED)
        assert not host(out).any()
    assert np.array_equal(host(dx), c["xqb"])
    bz.close()


# ---- EvalMult --------------------------------------------------------------------------------
_mult_cache = {}


def mult_case(log_n, sq):
    """(T, ring, secret, plaintexts, [c0, c1, d0, d1] each [3][Q][n], want): batch entry 0 is a real
    encryption (it decrypts), entries 1 and 2 are uniform towers (parity only)"""
    key = (log_n, sq)
    if key not in _mult_cache:
        q, rq = O.moduli_chain(log_n, sq)
        b, msk, _ = Z.behz_bases(O, log_n, q, Z.T_PLAIN)
        T = BT.BehzTables(q, b, msk, Z.T_PLAIN)
        ring = Z.Ring(O, log_n, T, rq)
        rng = np.random.default_rng(70 + log_n + sq)
        n = 1 << log_n
        s = np.array([int(v) for v in rng.integers(-1, 2, size=n)], dtype=object)
        ms = [np.array([int(v) for v in rng.integers(0, Z.T_PLAIN, size=n)], dtype=object) for _ in range(2)]
        cts = list(BR.encrypt(O, rng, ms[0], s, q, ring.tb_q, Z.T_PLAIN)) + \
            list(BR.encrypt(O, rng, ms[1], s, q, ring.tb_q, Z.T_PLAIN))
        cts = [np.concatenate([c, O.uniform_dcrt(2, sq, n, q, 950 + k)]) for k, c in enumerate(cts)]
        _mult_cache[key] = (T, ring, s, ms, cts, Z.eval_mult_behz(O, T, ring, *cts, fast=True))
    return _mult_cache[key]


def mult_handles(H, ctx, T, ring, log_n):
    plans = [H.NTTPlan(ctx, log_n, T.q, ring.rq), H.NTTPlan(ctx, log_n, T.bsk, ring.rbsk),
             H.NTTPlan(ctx, log_n, T.q + T.bsk, ring.rq + ring.rbsk)]
    return H.Behz(ctx, log_n, T), plans


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("sq", [2, 4])
@pytest.mark.parametrize("log_n", [4, 10])
def test_bfv_eval_mult_behz(hip, log_n, sq, batch):
    """against the restated composition; batch entry 0 also decrypts to the product of the plaintexts"""
    H, ctx = hip
    T, ring, s, ms, cts, ref = mult_case(log_n, sq)
    n = 1 << log_n
    bz, plans = mult_handles(H, ctx, T, ring, log_n)
    ins = [dev(c[:batch]) for c in cts]
    outs = [out_buf(batch, sq, n) for _ in range(3)]
    bz.eval_mult(*plans, *[t.data_ptr() for t in ins + outs], batch, stream())
    got = [host(o) for o in outs]
    for g, w in zip(got, ref):
        assert np.array_equal(g, w[:batch])
    for t, c in zip(ins, cts):
        assert np.array_equal(host(t), c[:batch])
    if log_n == 4 or batch == 1:
        assert (BR.decrypt3([g[:1] for g in got], s, T.q, Z.T_PLAIN) == BR.negacyclic(ms[0], ms[1]) % Z.T_PLAIN).all()
    for h in [bz] + plans:
        h.close()


def test_bfv_eval_mult_behz_on_caller_stream(hip, delay):  # noqa: F811
    """the multiplication (stream-ordered scratch, a dozen launches) ordered on the caller's stream alone"""
    H, ctx = hip
    log_n, sq, batch = 10, 2, 3
    T, ring, _, _, cts, ref = mult_case(log_n, sq)
    bz, plans = mult_handles(H, ctx, T, ring, log_n)
    run = OnStream(delay)
    ins = [run.input(c) for c in cts]
    outs = [run.output(batch, sq, 1 << log_n) for _ in range(3)]
    run.begin()
    bz.eval_mult(*plans, *[t.data_ptr() for t in ins + outs], batch, run.h)
    run.fetch(*outs)
    got = run.wait()
    for g, w in zip(got, ref):
        assert np.array_equal(g, w)
    import torch

    torch.cuda.synchronize()
    for h in [bz] + plans:
        h.close()


def test_behz_argument_checks(hip):
    """create refuses bad bases and tables; the calls refuse plans that do not match the handle and
    overlapping expand buffers, leave their outputs untouched, and the handle stays usable"""
    H, ctx = hip
    T, ring, pq, pb = kat_handles(H, ctx)
    log_n, n = KAT["log_n"], 8

    def tables(q=T.q, b=T.b, msk=T.msk):
        """the good tables presented with other moduli (only the moduli are wrong)"""
        bad = copy.copy(T)
        bad.q, bad.b, bad.bsk = list(q), list(b), list(b) + [msk]
        return bad

    for match, bad in (("odd", tables(q=[T.q[0], T.q[1] - 1])), ("below 2\\^60", tables(msk=(1 << 60) + 33)),
                       ("exceed 2\\^16", tables(b=[T.b[0], 65521])), ("repeated", tables(b=[T.b[0], T.q[0]])),
                       ("repeated", tables(msk=T.b[1]))):
        with pytest.raises(H.MathError, match=match):
            H.Behz(ctx, log_n, bad)
    bz = H.Behz(ctx, log_n, T)
    x = np.array([KAT["x"]], dtype=np.uint64)
    buf = out_buf(1, 5, n)
    for xp in (buf.data_ptr(), buf.data_ptr() + 8 * 4 * n):  # x at the head of out, and across its tail
        with pytest.raises(H.MathError, match="overlaps"):
            bz.expand(pq, pb, True, xp, buf.data_ptr(), 1, stream())
    assert not host(buf).any()
    other = H.Context(0)
    pq_other = H.NTTPlan(other, log_n, T.q, ring.rq)
    m4, r4 = O.moduli_chain(4, 2)
    pq_n16 = H.NTTPlan(ctx, 4, m4, r4)
    pq_rev = H.NTTPlan(ctx, log_n, T.q[::-1], ring.rq[::-1])
    pqb = H.NTTPlan(ctx, log_n, T.q + T.bsk, ring.rq + ring.rbsk)
    out = out_buf(1, 5, n)
    dx = dev(x)
    for match, a, b in (("context", pq_other, pb), ("ring dimension", pq_n16, pb), ("towers", pq_rev, pb),
                        ("towers", pb, pb), ("towers", pq, pq)):
        with pytest.raises(H.MathError, match=match):
            bz.expand(a, b, True, dx.data_ptr(), out.data_ptr(), 1, stream())
    outs = [out_buf(1, 2, n) for _ in range(3)]
    with pytest.raises(H.MathError, match="plan_qbsk"):
        bz.eval_mult(pq, pb, pb, *[dx.data_ptr()] * 4, *[o.data_ptr() for o in outs], 1, stream())
    with pytest.raises(H.MathError, match="towers"):
        bz.eval_mult(pq_rev, pb, pqb, *[dx.data_ptr()] * 4, *[o.data_ptr() for o in outs], 1, stream())
    with pytest.raises(H.MathError, match="bad data"):
        bz.floor(0, out.data_ptr(), 1, stream())
    assert not host(out).any() and not any(host(o).any() for o in outs)
    bz.expand(pq, pb, True, dx.data_ptr(), out.data_ptr(), 1, stream())
    assert np.array_equal(host(out)[0], np.array(KAT["expected"], dtype=np.uint64))
    for h in (bz, pqb, pq_rev, pq_n16, pq_other, pb, pq):
        h.close()
    other.close()
