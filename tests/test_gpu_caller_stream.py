"""The caller's stream is the only thing the host waits on.

include/ofhe_hip.h: "calls are asynchronous on that stream; nothing here
synchronises".  Nearly every other GPU test passes torch's current stream --
the legacy null stream -- and fetches results after torch.cuda.synchronize(),
which hides a launch that lost its stream argument, a side stream (KsFork,
ofhe_hip_plan_tune(.., 2)) that was not forked behind the caller's stream or
not joined back into it, and stream-ordered scratch freed on another stream.

Here every op runs on a torch.cuda.Stream of its own (non-blocking: it does
not synchronise with the null stream).  The device inputs start as zeros; on
the stream, unrelated library work comes first (forward NTTs of a throwaway
buffer, repeated until they fill about DELAY_MS: one such NTT took 0.065 ms
on an MI355X, so the fixture times one and sizes the repeat count from that), then the real
inputs arrive by asynchronous copies from pinned memory -- which by themselves
also keep the inputs zero for a while after the host has moved on -- then the
op, then the copies of its outputs to pinned memory.  The host waits for that
stream alone and compares with the oracle.  Work that is not ordered behind
the stream reads zeros; work the stream does not wait for leaves the outputs
unfinished.  These tests only order work: nothing in them can fault."""
import numpy as np
import pytest

import keyswitch as K
import oracle as O
from test_mixed_moduli_oracle import mixed_chain, rescale_chain, bv_chain, uniform

pytestmark = pytest.mark.gpu

Q_BITS, P_BITS = [60, 50, 45, 55, 40, 58], [60, 59]  # 6 + 2 towers of mixed size
DELAY_MS, DELAY_MAX_REPEATS = 3.0, 256  # the work queued ahead of every op, and a bound on its launches


@pytest.fixture(scope="module")
def delay(hip):
    """delay(stream, which): forward NTTs of a 2^16 x 16-tower x batch-8
    throwaway buffer (64 MiB) on `stream`, as many as take about DELAY_MS by
    one timing of a single transform made here; two buffers for two streams."""
    import torch

    H, ctx = hip
    q, r = O.moduli_chain(16, 16)
    plan = H.NTTPlan(ctx, 16, q, r)
    bufs = [torch.zeros((8, 16, 1 << 16), dtype=torch.int64, device="cuda") for _ in range(2)]
    cur = torch.cuda.current_stream().cuda_stream
    plan.forward(bufs[0].data_ptr(), 8, cur)  # warm: the first launch also loads the code object
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    plan.forward(bufs[0].data_ptr(), 8, cur)
    t1.record()
    torch.cuda.synchronize()
    one_ms = max(t0.elapsed_time(t1), 1e-3)
    repeats = int(min(DELAY_MAX_REPEATS, max(1, -(-DELAY_MS // one_ms))))

    def run(stream, which=0):
        for _ in range(repeats):
            plan.forward(bufs[which].data_ptr(), 8, stream.cuda_stream)

    run.one_ms, run.repeats = one_ms, repeats

    yield run
    torch.cuda.synchronize()
    plan.close()


class OnStream:
    """Buffers and copies of one op on one caller stream."""

    def __init__(self, delay, which=0):
        import torch

        self.torch, self.delay, self.which = torch, delay, which
        self.s = torch.cuda.Stream()
        self.h = self.s.cuda_stream
        assert self.h != 0, "a stream of its own, not the null stream"
        self.pending, self.fetched = [], []

    def input(self, x):
        """A zeroed device buffer that receives x on the stream in begin()."""
        t = self.torch
        src = t.from_numpy(np.ascontiguousarray(x, dtype=np.uint64).view(np.int64)).pin_memory()
        d = t.zeros(src.shape, dtype=t.int64, device="cuda")
        self.pending.append((d, src))
        return d

    def output(self, *shape):
        return self.torch.zeros(shape, dtype=self.torch.int64, device="cuda")

    def begin(self, sync=True):
        if sync:  # the zeros are in place before anything is queued on the stream
            self.torch.cuda.synchronize()
        self.delay(self.s, self.which)
        with self.torch.cuda.stream(self.s):
            for d, src in self.pending:
                d.copy_(src, non_blocking=True)

    def fetch(self, *outs):
        """Queue copies of outs to pinned memory on the stream; valid after wait()."""
        t = self.torch
        with t.cuda.stream(self.s):
            for o in outs:
                h = t.empty(o.shape, dtype=t.int64, pin_memory=True)
                h.copy_(o, non_blocking=True)
                self.fetched.append(h)

    def wait(self):
        self.s.synchronize()  # this stream only: never the device
        return [h.numpy().view(np.uint64) for h in self.fetched]


def _ks_bases(log_n):
    m, r = mixed_chain(log_n, Q_BITS + P_BITS)
    return m[:6], r[:6], m[6:], r[6:]


@pytest.mark.parametrize("alias", [False, True])
def test_pipeline_two_streams_on_caller_stream(hip, delay, alias):
    """ntt_mul_intt at N = 2^13, batch 5, after tune(2, 2): chunks of two
    polynomials alternate between the plan's two streams."""
    H, ctx = hip
    log_n, T, B = 13, 3, 5
    n = 1 << log_n
    q, r = mixed_chain(log_n, [60, 45, 52])
    a, b = O.uniform_dcrt(B, T, n, q, 31), O.uniform_dcrt(B, T, n, q, 32)
    want = O.ntt_mul_intt(a, b, O.Tables(n, q, r))
    plan = H.NTTPlan(ctx, log_n, q, r)
    plan.tune(2, 2)
    try:
        run = OnStream(delay)
        da, db = run.input(a), run.input(b)
        dc = da if alias else run.output(B, T, n)
        run.begin()
        plan.ntt_mul_intt(da.data_ptr(), db.data_ptr(), dc.data_ptr(), B, run.h)
        run.fetch(dc)
        (got,) = run.wait()
        assert np.array_equal(got, want)
    finally:
        plan.tune(0, 1)
    import torch

    torch.cuda.synchronize()
    plan.close()


def _core_case(log_n, t, B=2):
    n = 1 << log_n
    q, rq, p, rp = _ks_bases(log_n)
    kp = K.KeySwitchParams(n, q, rq, p, rp, 3)
    rng = np.random.default_rng(log_n + t)
    c = uniform(rng, B, q, n)
    kb, ka = uniform(rng, 3, q + p, n), uniform(rng, 3, q + p, n)
    return kp, c, kb, ka


@pytest.mark.parametrize("log_n,t", [(13, 0), (17, 0), (13, 65537)])
@pytest.mark.parametrize("single_stream", [0, 1])
def test_keyswitch_core_on_caller_stream(hip, delay, log_n, t, single_stream):
    H, ctx = hip
    kp, c, kb, ka = _core_case(log_n, t)
    B, n = c.shape[0], c.shape[2]
    want = K.ks_core(kp, c, kb, ka, t)
    opt = H.KsOptions()
    opt.single_stream = single_stream
    ks = H.KeySwitch(ctx, log_n, kp.q, kp.rq, kp.p, kp.rp, 3, opt)
    run = OnStream(delay)
    dc, dkb, dka = run.input(c), run.input(kb), run.input(ka)
    o0, o1 = run.output(B, 6, n), run.output(B, 6, n)
    run.begin()
    ks.core(6, dc.data_ptr(), dkb.data_ptr(), dka.data_ptr(), o0.data_ptr(), o1.data_ptr(), t, B, run.h)
    run.fetch(o0, o1)
    g0, g1 = run.wait()
    assert np.array_equal(g0, want[0]) and np.array_equal(g1, want[1])
    ks.close()


def test_keyswitch_steps_on_caller_stream(hip, delay):
    """precompute, fast_core_ext and mod_down as three calls on the stream:
    each one's side streams join before the next one reads its result."""
    H, ctx = hip
    log_n, t = 13, 0
    kp, c, kb, ka = _core_case(log_n, 7)
    B, n = c.shape[0], c.shape[2]
    wd = K.ks_precompute(kp, c)
    w0, w1 = K.ks_fast_core_ext(kp, wd, kb, ka)
    r0 = K.ks_mod_down(kp, w0, t)
    ks = H.KeySwitch(ctx, log_n, kp.q, kp.rq, kp.p, kp.rp, 3)
    run = OnStream(delay)
    dc, dkb, dka = run.input(c), run.input(kb), run.input(ka)
    d = run.output(B, 3, 8, n)
    c0, c1, o0 = run.output(B, 8, n), run.output(B, 8, n), run.output(B, 6, n)
    run.begin()
    ks.precompute(6, dc.data_ptr(), d.data_ptr(), B, run.h)
    ks.fast_core_ext(6, d.data_ptr(), dkb.data_ptr(), dka.data_ptr(), c0.data_ptr(), c1.data_ptr(), B, run.h)
    ks.mod_down(6, c0.data_ptr(), o0.data_ptr(), t, B, run.h)
    run.fetch(d, c0, c1, o0)
    gd, g0, g1, go = run.wait()
    assert np.array_equal(gd, wd)
    assert np.array_equal(g0, w0) and np.array_equal(g1, w1)
    assert np.array_equal(go, r0)
    ks.close()


def test_approx_mod_up_down_on_caller_stream(hip, delay):
    H, ctx = hip
    log_n, B = 13, 2
    n = 1 << log_n
    q, rq, p, rp = _ks_bases(log_n)
    pq, pp = H.NTTPlan(ctx, log_n, q, rq), H.NTTPlan(ctx, log_n, p, rp)
    qhinv, qhmodp = K.switch_tables(q, p)
    up = H.BaseConverter(ctx, log_n, q, p, qhinv, [v for row in qhmodp for v in row])
    phinv, phmodq = K.switch_tables(p, q)
    down = H.BaseConverter(ctx, log_n, p, q, phinv, [v for row in phmodq for v in row])
    rng = np.random.default_rng(5)
    x, y = uniform(rng, B, q, n), uniform(rng, B, q + p, n)
    T = K.moddown_tables(q, p, 0)
    run = OnStream(delay)
    dx, dy = run.input(x), run.input(y)
    oup, odown = run.output(B, 8, n), run.output(B, 6, n)
    run.begin()
    H.approx_mod_up(pq, pp, up, True, dx.data_ptr(), oup.data_ptr(), B, run.h)
    H.approx_mod_down(pq, pp, down, T["pinv_modq"], 0, dy.data_ptr(), odown.data_ptr(), B, run.h)
    run.fetch(oup, odown)
    gup, gdown = run.wait()
    assert np.array_equal(gup, K.approx_mod_up(x, q, rq, p, rp, True))
    assert np.array_equal(gdown, K.approx_mod_down(y, q, rq, p, rp, 0))
    for o in (up, down, pq, pp):
        o.close()


@pytest.mark.parametrize("log_n", [13, 16])
def test_rescale_on_caller_stream(hip, delay, log_n):
    """Evaluation form: the dropped tower's coefficient form and the switched
    towers live in stream-ordered scratch that is freed when the call returns."""
    H, ctx = hip
    B, T, t = 2, 5, 65537
    n = 1 << log_n
    q, r = rescale_chain(log_n, small_bits=34)  # every tower of the special form: the default kernels
    x = uniform(np.random.default_rng(log_n), B, q, n)
    c, a = K.rescale_tables(q)
    negtinv = (-pow(t, -1, q[-1])) % q[-1]
    plan = H.NTTPlan(ctx, log_n, q, r)
    run = OnStream(delay)
    dx = run.input(x)
    o1, o2 = run.output(B, T - 1, n), run.output(B, T - 1, n)
    run.begin()
    plan.drop_last_and_scale(T, dx.data_ptr(), T * n, o1.data_ptr(), (T - 1) * n, True, c, a, B, run.h)
    plan.mod_reduce(T, dx.data_ptr(), T * n, o2.data_ptr(), (T - 1) * n, True, t, negtinv, a, B, run.h)
    run.fetch(o1, o2)
    g1, g2 = run.wait()
    assert np.array_equal(g1, K.drop_last_and_scale(x, q, r, True, c, a))
    assert np.array_equal(g2, K.mod_reduce(x, q, r, True, t, negtinv, a))
    plan.close()


def test_bv_precompute_on_caller_stream(hip, delay):
    H, ctx = hip
    log_n, B, T = 13, 2, 4
    n = 1 << log_n
    q, r = bv_chain(log_n, small_bits=34)
    x = uniform(np.random.default_rng(9), B, q, n)
    plan = H.NTTPlan(ctx, log_n, q, r)
    run = OnStream(delay)
    dx = run.input(x)
    dd = run.output(B, T, T, n)
    run.begin()
    plan.bv_precompute(T, dx.data_ptr(), dd.data_ptr(), B, run.h)
    run.fetch(dd)
    (got,) = run.wait()
    assert np.array_equal(got, K.crt_decompose0(x, q, r))
    plan.close()


def test_one_engine_two_caller_streams(hip, delay):
    """One KeySwitch engine driven from two caller streams back to back: its
    side streams are shared, and each result is waited on through its own
    stream only."""
    H, ctx = hip
    log_n = 13
    kp, c, kb, ka = _core_case(log_n, 0)
    B, n = c.shape[0], c.shape[2]
    c2 = uniform(np.random.default_rng(77), B, kp.q, n)
    want_a, want_b = K.ks_core(kp, c, kb, ka, 0), K.ks_core(kp, c2, kb, ka, 65537)
    ks = H.KeySwitch(ctx, log_n, kp.q, kp.rq, kp.p, kp.rp, 3)
    ra, rb = OnStream(delay, 0), OnStream(delay, 1)
    runs = []
    for run, x in ((ra, c), (rb, c2)):
        runs.append((run, run.input(x), run.input(kb), run.input(ka), run.output(B, 6, n), run.output(B, 6, n)))
    ra.begin()
    rb.begin(sync=False)
    for (run, dc, dkb, dka, o0, o1), t in zip(runs, (0, 65537)):
        ks.core(6, dc.data_ptr(), dkb.data_ptr(), dka.data_ptr(), o0.data_ptr(), o1.data_ptr(), t, B, run.h)
        run.fetch(o0, o1)
    gb = rb.wait()
    ga = ra.wait()
    assert np.array_equal(ga[0], want_a[0]) and np.array_equal(ga[1], want_a[1])
    assert np.array_equal(gb[0], want_b[0]) and np.array_equal(gb[1], want_b[1])
    import torch

    torch.cuda.synchronize()
    ks.close()
