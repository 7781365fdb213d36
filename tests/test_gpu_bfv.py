"""GPU parity of the BFV (HPS family) multiplication steps, bit for bit against
the CPU restatement in tests/bfv_ref.py: the exact SwitchCRTBasis (matrix-core,
limb and 128-bit kernels), ExpandCRTBasis, ScaleAndRound (both alpha branches)
and EvalMult for HPS and HPSPOVERQ.  The switch inputs carry the planted
near-Q/2 coefficients on which a fused or reordered double sum gives another
alpha (tests/test_bfv_oracle.py asserts that property on these very inputs,
bfv_ref.SWITCH_CASES and SWITCH_CASES_MMA; the latter reach every K-step count
of the matrix-core kernel, a second target chunk and, with SWITCH_CAP_CASE, the
grid cap)."""
import numpy as np
import pytest
from conftest import load_golden

import bfv_ref as R
import bfv_tables as BT
import oracle as O
from test_gpu_caller_stream import OnStream, delay  # noqa: F401  (delay is a fixture)

pytestmark = pytest.mark.gpu

REF = load_golden("reference_fixtures.json")
T_PLAIN = 65537


def dev(x):
    import torch

    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.uint64).view(np.int64)).cuda()


def host(t):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint64)


def stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def out_buf(*shape):
    import torch

    return torch.zeros(shape, dtype=torch.int64, device="cuda")


def chain(log_n, sq, sp):
    m, r = O.moduli_chain(log_n, sq + sp)
    return m[:sq], r[:sq], m[sq:], r[sq:]


def converter(H, ctx, log_n, q, p, kernel=0):
    """a BaseConverter with the true CRT tables of q -> p"""
    return H.BaseConverter(ctx, log_n, q, p, BT.hat_inv(q), BT.BfvTables.flat(BT.hat_mod(q, p)), kernel=kernel)


# ---- exact switch ------------------------------------------------------------------------
_switch_want = {}


def switch_case(log_n, sq, sp):
    """(q, p, x [3][sq][n], want [3][sp][n]) of one R.SWITCH_CASES entry: the reference is computed
    once, the batch-1 run uses entry 0"""
    q, p, x, _ = R.switch_case(O, log_n, sq, sp)
    key = (log_n, sq, sp)
    if key not in _switch_want:
        _switch_want[key] = R.switch_crt_basis(x, q, p)
    return q, p, x, _switch_want[key]


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("log_n,sq,sp", R.SWITCH_CASES)
def test_switch_crt_basis(hip, log_n, sq, sp, batch):
    """ofhe_hip_switch_crt_basis with every kernel the handle can select (AUTO; LIMB up to 16
    sources; WIDE), inputs unchanged afterwards."""
    H, ctx = hip
    q, p, x, want = switch_case(log_n, sq, sp)
    x, want = x[:batch], want[:batch]
    kernels = [H.BCONV_KERNEL_AUTO, H.BCONV_KERNEL_WIDE] + ([H.BCONV_KERNEL_LIMB] if sq <= 16 else [])
    for kernel in kernels:
        bc = converter(H, ctx, log_n, q, p, kernel)
        dx, out = dev(x), out_buf(batch, sp, 1 << log_n)
        bc.switch_exact(dx.data_ptr(), out.data_ptr(), batch, stream())
        got = host(out)
        assert np.array_equal(got, want), f"kernel {kernel}: {np.count_nonzero(got != want)} words differ"
        assert np.array_equal(host(dx), x)
        bc.close()


def switch_case_mma(log_n, sq, sp):
    """the same for one R.SWITCH_CASES_MMA entry"""
    q, p, x, _ = R.switch_case_mma(O, log_n, sq, sp)
    key = ("mma", log_n, sq, sp)
    if key not in _switch_want:
        _switch_want[key] = R.switch_crt_basis(x, q, p)
    return q, p, x, _switch_want[key]


def _switch_kernels(H, sq):
    return [H.BCONV_KERNEL_AUTO, H.BCONV_KERNEL_WIDE] + ([H.BCONV_KERNEL_LIMB] if sq <= 16 else [])


def _check_switch(H, ctx, log_n, q, p, x, want, kernel):
    batch = x.shape[0]
    bc = converter(H, ctx, log_n, q, p, kernel)
    dx, out = dev(x), out_buf(batch, len(p), 1 << log_n)
    bc.switch_exact(dx.data_ptr(), out.data_ptr(), batch, stream())
    got = host(out)
    bad = np.argwhere(got != want)
    assert not len(bad), f"kernel {kernel}: {len(bad)} words differ, first (batch, target, coefficient) {bad[0]}"
    assert np.array_equal(host(dx), x)
    bc.close()


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("log_n,sq,sp", R.SWITCH_CASES_MMA)
def test_switch_crt_basis_mma_steps(hip, log_n, sq, sp, batch):
    """Every K-step count of k_switch_mma that R.SWITCH_CASES leaves out (3, 6, 7, 8 and the WIDE
    combine's 10, 12, 14, 16), with and without the special-prime reduction, two cases with a second
    target chunk; the inputs hold the planted near-Q/2 coefficients, alpha = size_q and the extreme
    digit columns (tests/test_bfv_oracle.py).  The other kernels run on the same inputs."""
    H, ctx = hip
    q, p, x, want = switch_case_mma(log_n, sq, sp)
    for kernel in _switch_kernels(H, sq):
        _check_switch(H, ctx, log_n, q, p, x[:batch], want[:batch], kernel)


def test_switch_crt_basis_past_the_grid_cap(hip):
    """1024 blocks of 256 coefficients against the matrix-core kernel's grid cap of 768: the group
    loop's second, partial trip (batch entry 3, which holds planted coefficients of its own)."""
    H, ctx = hip
    blocks_per_cu = 3  # BCONV_MMA_BLOCKS_PER_CU (csrc/bconv_mma.hpp); the cap is 256 CUs x this / chunks
    log_n, sq, sp = R.SWITCH_CAP_CASE
    tiles, tpc = R.mma_tpc(sq, sp)
    assert R.SWITCH_CAP_BATCH * (1 << log_n) // 256 > 256 * blocks_per_cu // -(-tiles // tpc)
    q, p, x, _ = R.switch_case_cap(O)
    want = R.switch_crt_basis(x, q, p)
    for kernel in (H.BCONV_KERNEL_AUTO, H.BCONV_KERNEL_LIMB, H.BCONV_KERNEL_WIDE):
        _check_switch(H, ctx, log_n, q, p, x, want, kernel)


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("log_n", [3, 5, 12])
def test_switch_known_answer(hip, log_n, batch):
    """The (3, 2, 2) case, UnitTestBFVrnsCRTOperations.cpp:290-376: SwitchCRTBasis(R -> Q) of the
    answer's R towers gives its Q towers (the fixture's expected_ql); the N = 8 vectors as they are
    and tiled to N = 2^5 and 2^12, as test_kat_fast_expand_crt_basis does for the approximate half.
    Batch entry 1 holds the columns reversed, entry 2 rotated by three."""
    H, ctx = hip
    k = REF["kat_fast_expand_crt_basis"]
    q, r = k["q"], k["r"]
    reps = (1 << log_n) // 8
    x0 = np.tile(np.array(k["expected_rl"], np.uint64), (1, reps))
    w0 = np.tile(np.array(k["expected_ql"], np.uint64), (1, reps))
    x = np.stack([x0, x0[:, ::-1], np.roll(x0, 3, axis=1)])[:batch]
    want = np.stack([w0, w0[:, ::-1], np.roll(w0, 3, axis=1)])[:batch]
    for kernel in (H.BCONV_KERNEL_AUTO, H.BCONV_KERNEL_LIMB, H.BCONV_KERNEL_WIDE):
        bc = converter(H, ctx, log_n, r, q, kernel)
        dx, out = dev(x), out_buf(batch, 2, 1 << log_n)
        bc.switch_exact(dx.data_ptr(), out.data_ptr(), batch, stream())
        assert np.array_equal(host(out), want)
        assert np.array_equal(host(dx), x)
        bc.close()


# ---- ExpandCRTBasis ------------------------------------------------------------------------
@pytest.mark.parametrize("eval_form", [False, True])
@pytest.mark.parametrize("log_n,sq,sp,batch", [(3, 2, 3, 2), (10, 4, 5, 2), (13, 3, 4, 1)])
def test_expand_crt_basis(hip, log_n, sq, sp, batch, eval_form):
    H, ctx = hip
    n = 1 << log_n
    q, rq, p, rp = chain(log_n, sq, sp)
    x = O.uniform_dcrt(batch, sq, n, q, 77 + log_n)
    want = R.expand_crt_basis(O, x, q, p, O.Tables(n, q, rq), O.Tables(n, p, rp), eval_form)
    pq, pp = H.NTTPlan(ctx, log_n, q, rq), H.NTTPlan(ctx, log_n, p, rp)
    bc = converter(H, ctx, log_n, q, p)
    dx, out = dev(x), out_buf(batch, sq + sp, n)
    H.expand_crt_basis(pq, pp, bc, eval_form, dx.data_ptr(), out.data_ptr(), batch, stream())
    got = host(out)
    assert np.array_equal(got, want)
    if eval_form:  # the Q towers are the caller's words, not a re-transform
        assert np.array_equal(got[:, :sq], x)
    assert np.array_equal(host(dx), x)
    for h in (bc, pq, pp):
        h.close()


def test_expand_crt_basis_on_caller_stream(hip, delay):  # noqa: F811
    """ExpandCRTBasis ordered on the caller's stream alone (a converter whose exact tables are
    not yet uploaded: the first exact call builds them)."""
    H, ctx = hip
    log_n, sq, sp, batch = 13, 3, 4, 2
    n = 1 << log_n
    q, rq, p, rp = chain(log_n, sq, sp)
    x = O.uniform_dcrt(batch, sq, n, q, 5)
    want = R.expand_crt_basis(O, x, q, p, O.Tables(n, q, rq), O.Tables(n, p, rp), True)
    pq, pp = H.NTTPlan(ctx, log_n, q, rq), H.NTTPlan(ctx, log_n, p, rp)
    bc = converter(H, ctx, log_n, q, p)
    run = OnStream(delay)
    dx, out = run.input(x), run.output(batch, sq + sp, n)
    run.begin()
    H.expand_crt_basis(pq, pp, bc, True, dx.data_ptr(), out.data_ptr(), batch, run.h)
    run.fetch(out)
    (got,) = run.wait()
    assert np.array_equal(got, want)
    import torch

    torch.cuda.synchronize()
    for h in (bc, pq, pp):
        h.close()


# ---- ScaleAndRound ---------------------------------------------------------------------------
SR_CASES = [(False, 1, 2), (False, 2, 3), (False, 4, 5), (False, 16, 17), (True, 2, 2), (True, 4, 4), (True, 17, 17)]


@pytest.mark.parametrize("log_n", [1, 5, 10])
@pytest.mark.parametrize("out_is_q,sq,sp", SR_CASES)
def test_scale_and_round(hip, log_n, out_is_q, sq, sp):
    """real tables of bfv_tables.py, uniform inputs, batch 2"""
    H, ctx = hip
    n, batch = 1 << log_n, 2
    q, _, p, _ = chain(log_n, sq, sp)
    if out_is_q:
        T = BT.BfvTables(q, p, T_PLAIN, BT.HPSPOVERQ)
        table, frac = T.sr_table, T.sr_frac
    else:
        table, frac = BT.scale_round_tables(q, p, T_PLAIN, BT.product(p), BT.product(q) * BT.product(p))
    x = O.uniform_dcrt(batch, sq + sp, n, q + p, 300 + sq)
    want = R.scale_and_round(x, q, p, out_is_q, table, frac)
    sr = H.ScaleRound(ctx, log_n, q, p, out_is_q, table, frac)
    dx, out = dev(x), out_buf(batch, sq if out_is_q else sp, n)
    sr.run(dx.data_ptr(), out.data_ptr(), batch, stream())
    assert np.array_equal(host(out), want)
    assert np.array_equal(host(dx), x)
    sr.close()


@pytest.mark.parametrize("out_is_q", [False, True])
@pytest.mark.parametrize("log_n", [1, 5, 10])
def test_scale_and_round_both_alpha_branches(hip, log_n, out_is_q):
    """the synthetic case with nu > 2^64 on the even and nu < 2^64 on the odd coefficients"""
    H, ctx = hip
    q, p, table, frac, x = R.two_branch_case(O, log_n, 11, out_is_q)
    want, nu = R.scale_and_round(x, q, p, out_is_q, table, frac, want_nu=True)
    assert (nu[0][0::2] > 2.0 ** 64).all() and (nu[0][1::2] < 2.0 ** 64).all()
    sr = H.ScaleRound(ctx, log_n, q, p, out_is_q, table, frac)
    out = out_buf(1, 17, 1 << log_n)
    sr.run(dev(x).data_ptr(), out.data_ptr(), 1, stream())
    assert np.array_equal(host(out), want)
    sr.close()


# ---- EvalMult --------------------------------------------------------------------------------
_mult_cache = {}


def mult_case(tech, log_n):
    """(T, roots, secret, plaintexts, [c0, c1, d0, d1] each [3][Q][n], want): batch entry 0 is a real
    encryption (it decrypts), entries 1 and 2 are uniform towers (parity only)"""
    key = (tech, log_n)
    if key not in _mult_cache:
        sq, sr = (2, 3) if tech == BT.HPS else (2, 2)
        q, rq, r, rr = chain(log_n, sq, sr)
        T = BT.BfvTables(q, r, T_PLAIN, tech)
        ring = R.Ring(O, log_n, q, rq, r, rr)
        rng = np.random.default_rng(40 + log_n + tech)
        n = 1 << log_n
        s = np.array([int(v) for v in rng.integers(-1, 2, size=n)], dtype=object)
        ms = [np.array([int(v) for v in rng.integers(0, T_PLAIN, size=n)], dtype=object) for _ in range(2)]
        cts = list(R.encrypt(O, rng, ms[0], s, q, ring.tb_q, T_PLAIN)) + \
            list(R.encrypt(O, rng, ms[1], s, q, ring.tb_q, T_PLAIN))
        cts = [np.concatenate([c, O.uniform_dcrt(2, sq, n, q, 900 + k)]) for k, c in enumerate(cts)]
        _mult_cache[key] = (T, (rq, rr), s, ms, cts, R.eval_mult(O, T, ring, *cts))
    return _mult_cache[key]


def mult_handles(H, ctx, T, log_n, roots):
    """(BfvMult, every handle it is composed from)"""
    q, r, (rq, rr) = T.q, T.r, roots
    pq, pr, pqr = H.NTTPlan(ctx, log_n, q, rq), H.NTTPlan(ctx, log_n, r, rr), H.NTTPlan(ctx, log_n, q + r, rq + rr)
    q_to_r, r_to_q = converter(H, ctx, log_n, q, r), converter(H, ctx, log_n, r, q)
    neg = None
    if T.technique == BT.HPSPOVERQ:
        neg = H.BaseConverter(ctx, log_n, q, r, T.neg_r_q_hat_inv_modq, T.flat(T.q_inv_modr))
    sr = H.ScaleRound(ctx, log_n, q, r, T.out_is_q, T.sr_table, T.sr_frac)
    tech = H.BFV_HPS if T.technique == BT.HPS else H.BFV_HPSPOVERQ
    mult = H.BfvMult(ctx, tech, pq, pr, pqr, q_to_r, r_to_q, neg, sr)
    return mult, [h for h in (sr, neg, r_to_q, q_to_r, pqr, pr, pq) if h is not None]


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("log_n", [4, 10])
@pytest.mark.parametrize("tech", [BT.HPS, BT.HPSPOVERQ])
def test_bfv_eval_mult(hip, tech, log_n, batch):
    """both techniques against the restated composition; at log_n = 10 batch entry 0 also decrypts
    to the product of the plaintexts"""
    H, ctx = hip
    T, roots, s, ms, cts, want = mult_case(tech, log_n)
    n, q = 1 << log_n, T.q
    mult, parts = mult_handles(H, ctx, T, log_n, roots)
    ins = [dev(c[:batch]) for c in cts]
    outs = [out_buf(batch, len(q), n) for _ in range(3)]
    mult.eval_mult(*[t.data_ptr() for t in ins + outs], batch, stream())
    got = [host(o) for o in outs]
    for g, w in zip(got, want):
        assert np.array_equal(g, w[:batch])
    for t, c in zip(ins, cts):
        assert np.array_equal(host(t), c[:batch])
    if log_n == 10:
        assert (R.decrypt3([g[:1] for g in got], s, q, T_PLAIN) == R.negacyclic(ms[0], ms[1]) % T_PLAIN).all()
    mult.close()
    for h in parts:
        h.close()


@pytest.mark.parametrize("tech", [BT.HPS, BT.HPSPOVERQ])
def test_bfv_eval_mult_on_caller_stream(hip, delay, tech):  # noqa: F811
    """EvalMult (stream-ordered scratch, eleven or more launches) ordered on the caller's stream alone"""
    H, ctx = hip
    log_n, batch = 10, 3
    T, roots, _, _, cts, want = mult_case(tech, log_n)
    mult, parts = mult_handles(H, ctx, T, log_n, roots)
    run = OnStream(delay)
    ins = [run.input(c) for c in cts]
    outs = [run.output(batch, len(T.q), 1 << log_n) for _ in range(3)]
    run.begin()
    mult.eval_mult(*[t.data_ptr() for t in ins + outs], batch, run.h)
    run.fetch(*outs)
    got = run.wait()
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    import torch

    torch.cuda.synchronize()
    mult.close()
    for h in parts:
        h.close()


def test_bfv_argument_checks(hip):
    """Overlapping ExpandCRTBasis buffers, handles of another context, more than 255 summed towers
    and an even output modulus are refused with a status, and the objects stay usable."""
    H, ctx = hip
    log_n, n = 3, 8
    q, rq, p, rp = chain(log_n, 2, 3)
    pq, pp, bc = H.NTTPlan(ctx, log_n, q, rq), H.NTTPlan(ctx, log_n, p, rp), converter(H, ctx, log_n, q, p)
    x = O.uniform_dcrt(1, 2, n, q, 3)
    buf = out_buf(1, 5, n)
    buf[:, :2].copy_(dev(x))
    for xp in (buf.data_ptr(), buf.data_ptr() + 8 * 4 * n):  # x at the head of out, and across its tail
        with pytest.raises(H.MathError, match="overlaps"):
            H.expand_crt_basis(pq, pp, bc, True, xp, buf.data_ptr(), 1, stream())
    other = H.Context(0)
    pq2 = H.NTTPlan(other, log_n, q, rq)
    out = out_buf(1, 5, n)
    with pytest.raises(H.MathError, match="context"):
        H.expand_crt_basis(pq2, pp, bc, True, dev(x).data_ptr(), out.data_ptr(), 1, stream())
    T = BT.BfvTables(q, p, T_PLAIN, BT.HPS)
    sr = H.ScaleRound(ctx, log_n, q, p, False, T.sr_table, T.sr_frac)
    pqr = H.NTTPlan(ctx, log_n, q + p, rq + rp)
    r_to_q = converter(H, ctx, log_n, p, q)
    with pytest.raises(H.MathError, match="belong to ctx"):
        H.BfvMult(ctx, H.BFV_HPS, pq2, pp, pqr, bc, r_to_q, None, sr)
    with pytest.raises(H.MathError, match="255"):
        H.ScaleRound(ctx, log_n, [3] * 256, [5], False, [[0] * 257], [0.0] * 256)
    with pytest.raises(H.MathError, match="odd"):
        H.ScaleRound(ctx, log_n, [3], [4], False, [[0, 0]], [0.5])
    dx = dev(x)
    H.expand_crt_basis(pq, pp, bc, True, dx.data_ptr(), out.data_ptr(), 1, stream())
    want = R.expand_crt_basis(O, x, q, p, O.Tables(n, q, rq), O.Tables(n, p, rp), True)
    assert np.array_equal(host(out), want)
    for h in (sr, r_to_q, pqr, pq2, bc, pp, pq):
        h.close()
    other.close()
