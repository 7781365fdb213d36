"""GPU parity of the BSGS linear transform (ofhe_hip_ks_bsgs_transform and its stage calls
ofhe_hip_ks_ext / _mult_ext_sum / _fast_rotation_ext_sum) against tests/linear_transform_ref.py,
bit for bit.

Uniform random ciphertexts, diagonals and distinct keys per step, as tests/test_gpu_rotation.py.
One reference per (shape, level, configuration) at batch 3; the batch-1 call is compared with its
slice, batch entries being independent.
"""
import numpy as np
import pytest

import keyswitch as K
import linear_transform_ref as LT
from test_gpu_caller_stream import OnStream, delay  # noqa: F401  (delay is a fixture)
from test_gpu_keyswitch import _ks_case, _uniform
from test_gpu_parity import dev, host, stream
from test_gpu_rotation import _levels
from test_linear_transform_oracle import _real_key_case, check_decrypts
from test_mixed_moduli_oracle import mixed_chain

pytestmark = pytest.mark.gpu

SHAPES = [
    (1, 2, 1, 1, False),    # N = 2: below a wave
    (3, 4, 2, 2, False),    # small ring
    (6, 5, 3, 2, False),    # partial last digit
    (12, 6, 2, 3, True),    # generic moduli
    (5, 8, 2, 4, False),    # beta = 4
    (5, 10, 2, 5, False),   # beta = 5: the runtime digit count
    (13, 8, 3, 3, False),   # several blocks per row
]
CASES = [s + (l,) for s in SHAPES for l in _levels(s[1], s[3])]


def nonid(n, r):
    """A non-identity automorphism index: 5^(r+1) mod 2N, or 2N - 1 where that is 1."""
    k = pow(5, r + 1, 2 * n)
    return k if k != 1 else 2 * n - 1


def zeros(*shape):
    import torch

    return torch.zeros(shape, dtype=torch.int64, device="cuda")


def ptr(x):
    return 0 if x is None else x.data_ptr()


class Bsgs:
    """Host and device copies of one transform's inputs, the fused call and its reference."""

    def __init__(self, rng, ks, kp, q, p, l, n, dnum, B, baby, giant, present=None, pad=0):
        self.ks, self.kp, self.l, self.n, self.B = ks, kp, l, n, B
        self.sp = len(p)
        self.baby, self.giant, self.present = list(baby), list(giant), present
        mods = q[:l] + p
        self.c0, self.c1 = _uniform(rng, B, q[:l], n), _uniform(rng, B, q[:l], n)

        def key(k):
            if LT.is_identity(k, n):
                return None
            return _uniform(rng, dnum, q + p, n), _uniform(rng, dnum, q + p, n)

        self.bkeys, self.gkeys = [key(k) for k in baby], [key(k) for k in giant]
        nd = len(baby) * len(giant)
        self.diag = _uniform(rng, nd, mods, n)
        # pad: extra words between diagonals (diag_stride > (l + P) N), filled with a value no modulus admits
        store = np.full((nd, (l + self.sp) * n + pad), np.uint64((1 << 64) - 1))
        store[:, :(l + self.sp) * n] = self.diag.reshape(nd, -1)
        if present is not None:  # absent diagonals are never read: poison them
            for d, pr in enumerate(present):
                if not pr:
                    store[d] = np.uint64((1 << 64) - 1)
        self.store, self.diag_stride = store, store.shape[1]
        self.d_c0, self.d_c1, self.d_diag = dev(self.c0), dev(self.c1), dev(store)
        self.d_bkeys = [None if k is None else (dev(k[0]), dev(k[1])) for k in self.bkeys]
        self.d_gkeys = [None if k is None else (dev(k[0]), dev(k[1])) for k in self.gkeys]

    @staticmethod
    def _ptrs(keys, e):
        return [0 if k is None else k[e].data_ptr() for k in keys]

    def run(self, batch=None, t=0, s=None, out=None, **over):
        batch = self.B if batch is None else batch
        o0, o1 = out or (zeros(batch, self.l, self.n), zeros(batch, self.l, self.n))
        a = dict(baby_indices=self.baby, giant_indices=self.giant, baby_key_b=self._ptrs(self.d_bkeys, 0),
                 baby_key_a=self._ptrs(self.d_bkeys, 1), giant_key_b=self._ptrs(self.d_gkeys, 0),
                 giant_key_a=self._ptrs(self.d_gkeys, 1), diag=self.d_diag.data_ptr(), diag_stride=self.diag_stride,
                 present=self.present, c0=self.d_c0.data_ptr(), c1=self.d_c1.data_ptr(), out0=o0.data_ptr(),
                 out1=o1.data_ptr(), t=t, batch=batch, stream=stream() if s is None else s)
        a.update(over)
        self.ks.bsgs_transform(self.l, **a)
        return o0, o1

    def ref(self, t=0):
        return LT.bsgs_ref(self.kp, self.c0, self.c1, self.baby, self.giant, self.bkeys, self.gkeys, self.diag,
                           self.present, t)

    def inputs_unchanged(self):
        ok = np.array_equal(host(self.d_c0), self.c0) and np.array_equal(host(self.d_c1), self.c1)
        ok = ok and np.array_equal(host(self.d_diag), self.store)
        for dk, hk in zip(self.d_bkeys + self.d_gkeys, self.bkeys + self.gkeys):
            if hk is not None:
                ok = ok and np.array_equal(host(dk[0]), hk[0]) and np.array_equal(host(dk[1]), hk[1])
        return ok


def _same(got, want):
    return all(np.array_equal(host(g), w) for g, w in zip(got, want))


def _check(bs, t=0):
    """the batch-3 call against the reference, the batch-1 call against its slice, inputs intact"""
    want = bs.ref(t)
    assert _same(bs.run(t=t), want), (bs.baby, bs.giant, t)
    if bs.B > 1:
        assert _same(bs.run(batch=1, t=t), [w[:1] for w in want]), (bs.baby, bs.giant, t, "batch 1")
    assert bs.inputs_unchanged()


@pytest.mark.parametrize("log_n,sq,sp,dnum,generic,l", CASES)
def test_bsgs_transform_parity(hip, log_n, sq, sp, dnum, generic, l):
    """(nbaby, ngiant) = (1, 1): identities only (all giants identity); (2, 3): identity babies and
    giants past position 0, given as 2N + 1, a ragged tail, t = 65537; (3, 2): no identity at all and
    one giant with no diagonal present.  At N = 2^13 the last two shrink to (2, 2)."""
    H, ctx = hip
    n, q, rq, p, rp, kp, ks = _ks_case(H, ctx, log_n, sq, sp, dnum, generic)
    rng = np.random.default_rng(2000 * log_n + l)
    k = [nonid(n, r) for r in range(5)]
    if log_n >= 13:
        configs = [([1], [1], None, 0), ([k[0], 2 * n + 1], [k[1], 1], [1, 1, 1, 0], 65537),
                   ([k[0], k[1]], [k[3], k[4]], [1, 1, 0, 0], 0)]
    else:
        configs = [([1], [1], None, 0), ([k[0], 2 * n + 1], [k[1], 1, k[2]], [1, 1, 1, 1, 1, 0], 65537),
                   ([k[0], k[1], k[2]], [k[3], k[4]], [1, 1, 1, 0, 0, 0], 0)]
    for baby, giant, present, t in configs:
        _check(Bsgs(rng, ks, kp, q, p, l, n, dnum, 3, baby, giant, present), t)
    ks.close()


@pytest.mark.parametrize("log_n,sq,sp,dnum", [(3, 4, 2, 2), (6, 5, 3, 2)])
def test_bsgs_identity_placements(hip, log_n, sq, sp, dnum):
    """Identity at position 0 of both lists, in the middle of both, nowhere, and on every giant;
    all diagonals present; diagonals stored with a stride wider than a diagonal."""
    H, ctx = hip
    n, q, rq, p, rp, kp, ks = _ks_case(H, ctx, log_n, sq, sp, dnum)
    rng = np.random.default_rng(70 + log_n)
    k = [nonid(n, r) for r in range(6)]
    for baby, giant in [([1, k[0], k[1]], [1, k[2]]),
                        ([k[0], 1, k[1]], [k[2], 2 * n + 1, k[3]]),
                        ([k[0], k[1]], [k[2], k[3]]),
                        ([k[0], 1], [1, 2 * n + 1, 4 * n + 1])]:
        _check(Bsgs(rng, ks, kp, q, p, sq, n, dnum, 2, baby, giant, None, pad=6), 0)
    ks.close()


@pytest.mark.parametrize("log_n,sq,sp,dnum", [(3, 4, 2, 2), (6, 5, 3, 2)])
def test_bsgs_past_the_per_launch_caps(hip, log_n, sq, sp, dnum):
    """17 babies (two term chunks of k_lt_inner) and KS_ROT_CAP + 1 giants (two launches of
    k_lt_outer and k_lt_first), with a ragged tail each."""
    H, ctx = hip
    n, q, rq, p, rp, kp, ks = _ks_case(H, ctx, log_n, sq, sp, dnum)
    rng = np.random.default_rng(80 + log_n)
    cap = H.KS_ROT_CAP
    baby = [1] + [nonid(n, r) for r in range(16)]
    _check(Bsgs(rng, ks, kp, q, p, sq, n, dnum, 2, baby, [1, nonid(n, 2)], [1] * 17 + [1] * 16 + [0]), 0)
    giant = [nonid(n, r) for r in range(cap + 1)]  # every one rotated: cap + 1 digit sets
    _check(Bsgs(rng, ks, kp, q, p, sq, n, dnum, 2, [1, nonid(n, 1)], giant, [1] * (2 * cap) + [1, 0]), 65537)
    ks.close()


# ---- the stage calls, each alone -------------------------------------------------
def _stage_inputs(rng, kp, q, p, l, n, dnum, B, nterm, nsum, nset):
    mods = q[:l] + p
    x0 = np.stack([_uniform(rng, B, mods, n) for _ in range(nterm)])
    x1 = np.stack([_uniform(rng, B, mods, n) for _ in range(nterm)])
    diag = _uniform(rng, nsum * nterm, mods, n)
    digits = np.stack([np.stack([_uniform(rng, kp.beta(l), mods, n) for _ in range(B)]) for _ in range(nset)])
    keys = [(_uniform(rng, dnum, q + p, n), _uniform(rng, dnum, q + p, n)) for _ in range(nset)]
    return x0, x1, diag, digits, keys


def _mult_ext_sum(ks, l, sp, n, x0, x1, diag, present, nsum, batch):
    nterm, B = x0.shape[:2]
    d0, d1, dd = dev(x0), dev(x1), dev(diag)
    o0, o1 = zeros(nsum, batch, l + sp, n), zeros(nsum, batch, l + sp, n)
    ks.mult_ext_sum(l, nterm, d0.data_ptr(), d1.data_ptr(), B * (l + sp) * n, dd.data_ptr(), (l + sp) * n, present,
                    nsum, o0.data_ptr(), o1.data_ptr(), batch, stream())
    assert np.array_equal(host(d0), x0) and np.array_equal(host(d1), x1) and np.array_equal(host(dd), diag)
    return o0, o1


def _rot_sum(ks, l, sp, n, digits, indices, keys, addend, batch):
    dd, da = dev(digits), None if addend is None else dev(addend)
    dk = [(dev(b), dev(a)) for b, a in keys]
    o0, o1 = zeros(batch, l + sp, n), zeros(batch, l + sp, n)
    ks.fast_rotation_ext_sum(l, dd.data_ptr(), indices, [b.data_ptr() for b, _ in dk], [a.data_ptr() for _, a in dk],
                             ptr(da), 0 if addend is None else len(addend), o0.data_ptr(), o1.data_ptr(), batch,
                             stream())
    assert np.array_equal(host(dd), digits)
    return o0, o1


@pytest.mark.parametrize("log_n,sq,sp,dnum,generic,l", CASES)
def test_stage_calls_parity(hip, log_n, sq, sp, dnum, generic, l):
    H, ctx = hip
    n, q, rq, p, rp, kp, ks = _ks_case(H, ctx, log_n, sq, sp, dnum, generic)
    rng = np.random.default_rng(3000 * log_n + l)
    B, nterm, nsum, nset = 2, 3, 2, 3
    x0, x1, diag, digits, keys = _stage_inputs(rng, kp, q, p, l, n, dnum, B, nterm, nsum, nset)
    # KeySwitchExt
    c = _uniform(rng, B, q[:l], n)
    dc, out = dev(c), zeros(B, l + sp, n) + 7
    ks.ext(l, dc.data_ptr(), out.data_ptr(), B, stream())
    assert np.array_equal(host(out), LT.ext_ref(kp, c)) and np.array_equal(host(dc), c)
    # the multiply-accumulate, all present and with one absent diagonal per sum
    for present in (None, [1, 0, 1, 0, 1, 1]):
        want = LT.mult_ext_sum_ref(kp, l, x0, x1, diag, present, nsum)
        assert _same(_mult_ext_sum(ks, l, sp, n, x0, x1, diag, present, nsum, B), want), present
    # batch 1 reads entry 0 of every term (x_stride stays the batch-2 stride)
    got = _mult_ext_sum(ks, l, sp, n, x0, x1, diag, None, nsum, 1)
    assert _same(got, [w[:, :1] for w in LT.mult_ext_sum_ref(kp, l, x0, x1, diag, None, nsum)])
    # the rotated sum, with and without addends; index 1 is the plain inner product
    idx = [nonid(n, 0), 1, nonid(n, 1) + 2 * n]
    add = np.stack([_uniform(rng, B, q[:l] + p, n) for _ in range(2)])
    assert _same(_rot_sum(ks, l, sp, n, digits, idx, keys, None, B),
                 LT.fast_rotation_ext_sum_ref(kp, digits, idx, keys))
    assert _same(_rot_sum(ks, l, sp, n, digits, idx, keys, add, B),
                 LT.fast_rotation_ext_sum_ref(kp, digits, idx, keys, add))
    ks.close()


def _top(shape, mods):
    """every word q_t - 1; towers on axis -2"""
    return np.broadcast_to((np.array(mods, np.uint64) - np.uint64(1))[:, None], shape).copy()


EXTREME_CHAINS = {
    "60-bit": lambda log_n: _named_chain(log_n, [60, 60, 59, 59, 60, 59], [60, 59]),
    "smallest": lambda log_n: _named_chain(log_n, [22] * 6, [22, 22]),
}


def _named_chain(log_n, qbits, pbits):
    m, r = mixed_chain(log_n, qbits + pbits)
    sq = len(qbits)
    return m[:sq], r[:sq], m[sq:], r[sq:]


@pytest.mark.parametrize("chain", sorted(EXTREME_CHAINS))
def test_mult_ext_sum_at_the_largest_limb_sums(hip, chain):
    """16 and 17 terms whose words and diagonals are all q_t - 1: every limb sum of a 16-term launch
    at its maximum, and the second term chunk added to it."""
    H, ctx = hip
    log_n, dnum = 4, 2
    n = 1 << log_n
    q, rq, p, rp = EXTREME_CHAINS[chain](log_n)
    kp = K.KeySwitchParams(n, q, rq, p, rp, dnum)
    ks = H.KeySwitch(ctx, log_n, q, rq, p, rp, dnum)
    l, sp, B, nsum = len(q), len(p), 2, 2
    mods = q + p
    for nterm in (16, 17):
        x = _top((nterm, B, l + sp, n), mods)
        diag = _top((nsum * nterm, l + sp, n), mods)
        want = LT.mult_ext_sum_ref(kp, l, x, x, diag, None, nsum)
        for b in range(B):
            for t, m in enumerate(mods):  # nterm (m - 1)^2 = nterm mod m
                assert int(want[0][0, b, t, 0]) == nterm % m
        assert _same(_mult_ext_sum(ks, l, sp, n, x, x, diag, None, nsum, B), want), nterm
    # uniform words on the same towers
    rng = np.random.default_rng(90)
    x0, x1, diag, _, _ = _stage_inputs(rng, kp, q, p, l, n, dnum, B, 17, nsum, 1)
    assert _same(_mult_ext_sum(ks, l, sp, n, x0, x1, diag, None, nsum, B),
                 LT.mult_ext_sum_ref(kp, l, x0, x1, diag, None, nsum))
    ks.close()


@pytest.mark.parametrize("chain", sorted(EXTREME_CHAINS))
def test_fast_rotation_ext_sum_at_the_largest_limb_sums(hip, chain):
    """Digits and keys all q_t - 1 with sets x beta = 16, 17 and 33 (beta = 1: one, two and three
    reductions of the limb sums), 8 and 9 sets x beta = 2, and 6 sets x beta = 3, where the
    reduction after 16 products falls inside a set."""
    H, ctx = hip
    log_n = 4
    n = 1 << log_n
    q, rq, p, rp = EXTREME_CHAINS[chain](log_n)
    l, sp, B = len(q), len(p), 2
    mods = q + p
    for dnum, sets in ((1, (16, 17, 33)), (2, (8, 9)), (3, (6,))):
        kp = K.KeySwitchParams(n, q, rq, p, rp, dnum)
        ks = H.KeySwitch(ctx, log_n, q, rq, p, rp, dnum)
        beta = kp.beta(l)
        for nset in sets:
            digits = _top((nset, B, beta, l + sp, n), mods)
            keys = [(_top((dnum, l + sp, n), mods), _top((dnum, l + sp, n), mods)) for _ in range(nset)]
            idx = [nonid(n, r) for r in range(nset)]
            want = LT.fast_rotation_ext_sum_ref(kp, digits, idx, keys)
            assert int(want[0][0, 0, 0]) == (nset * beta) % mods[0]
            assert _same(_rot_sum(ks, l, sp, n, digits, idx, keys, None, B), want), (dnum, nset)
        rng = np.random.default_rng(91)
        _, _, _, digits, keys = _stage_inputs(rng, kp, q, p, l, n, dnum, B, 1, 1, 17)
        idx = [nonid(n, r) for r in range(17)]
        assert _same(_rot_sum(ks, l, sp, n, digits, idx, keys, None, B),
                     LT.fast_rotation_ext_sum_ref(kp, digits, idx, keys))
        ks.close()


@pytest.mark.parametrize("chain", sorted(EXTREME_CHAINS))
def test_bsgs_on_extreme_towers(hip, chain):
    H, ctx = hip
    log_n, dnum = 4, 2
    n = 1 << log_n
    q, rq, p, rp = EXTREME_CHAINS[chain](log_n)
    kp = K.KeySwitchParams(n, q, rq, p, rp, dnum)
    ks = H.KeySwitch(ctx, log_n, q, rq, p, rp, dnum)
    rng = np.random.default_rng(92)
    _check(Bsgs(rng, ks, kp, q, p, len(q), n, dnum, 2, [1, nonid(n, 0), nonid(n, 1)], [1, nonid(n, 2)],
                [1, 1, 1, 1, 1, 0]), 0)
    ks.close()


# ---- engine options and streams ----------------------------------------------------
@pytest.mark.parametrize("opt", ["single_stream", "chunk"])
def test_bsgs_engine_options_small(hip, opt):
    H, ctx = hip
    log_n, sq, sp, dnum = 6, 5, 3, 2
    o = H.KsOptions(single_stream=1) if opt == "single_stream" else H.KsOptions(chunk=2)
    n, q, rq, p, rp, kp, ks = _ks_case(H, ctx, log_n, sq, sp, dnum, options=o)
    rng = np.random.default_rng(93)
    _check(Bsgs(rng, ks, kp, q, p, sq, n, dnum, 3, [1, nonid(n, 0)], [1, nonid(n, 1), nonid(n, 2)],
                [1, 1, 1, 1, 1, 0]), 65537)
    ks.close()


def test_bsgs_separate_cols_and_icol(hip):
    """options.separate_cols / separate_icol change the ModUp / ModDown kernels at N = 2^17 only:
    one reference there, the default engine and one engine per option against it."""
    H, ctx = hip
    log_n, sq, sp, dnum = 17, 3, 2, 2
    n = 1 << log_n
    rng = np.random.default_rng(94)
    want = None
    for o in (None, H.KsOptions(separate_cols=1), H.KsOptions(separate_icol=1)):
        n, q, rq, p, rp, kp, ks = _ks_case(H, ctx, log_n, sq, sp, dnum, options=o)
        if want is None:
            first = Bsgs(rng, ks, kp, q, p, sq, n, dnum, 1, [1, nonid(n, 0)], [1, nonid(n, 1)])
            want = first.ref(0)
        first.ks = ks
        assert _same(first.run(), want), o
        ks.close()


def test_bsgs_on_caller_stream(hip, delay):  # noqa: F811
    """The fused call from a non-default stream, waited on through that stream alone."""
    H, ctx = hip
    log_n, sq, sp, dnum, B = 10, 6, 2, 3, 2
    n, q, rq, p, rp, kp, ks = _ks_case(H, ctx, log_n, sq, sp, dnum)
    rng = np.random.default_rng(95)
    bs = Bsgs(rng, ks, kp, q, p, sq, n, dnum, B, [1, nonid(n, 0)], [1, nonid(n, 1)], [1, 1, 1, 0])
    st = OnStream(delay)
    bs.d_c0, bs.d_c1 = st.input(bs.c0), st.input(bs.c1)
    bs.d_diag = st.input(host(bs.d_diag))
    bs.d_bkeys = [None if k is None else (st.input(k[0]), st.input(k[1])) for k in bs.bkeys]
    bs.d_gkeys = [None if k is None else (st.input(k[0]), st.input(k[1])) for k in bs.gkeys]
    o0, o1 = st.output(B, sq, n), st.output(B, sq, n)
    st.begin()
    bs.run(s=st.h, out=(o0, o1))
    st.fetch(o0, o1)
    got = st.wait()
    assert all(np.array_equal(a, b) for a, b in zip(got, bs.ref(0)))
    import torch

    torch.cuda.synchronize()
    ks.close()


def test_bsgs_semantics_with_real_keys(hip):
    """The CPU semantic test's case (tests/test_linear_transform_oracle.py) with bsgs_transform in
    place of the reference: the device's output decrypts to the linear transform within the same bound."""
    H, ctx = hip
    case = _real_key_case()
    ks = H.KeySwitch(ctx, case["log_n"], case["q"], case["rq"], case["p"], case["rp"], case["dnum"])
    bs = Bsgs(np.random.default_rng(0), ks, case["kp"], case["q"], case["p"], case["sq"], case["n"], case["dnum"], 1,
              case["baby"], case["giant"], case["present"])
    bs.c0, bs.c1, bs.diag, bs.bkeys, bs.gkeys = case["c0"], case["c1"], case["diag"], case["bkeys"], case["gkeys"]
    bs.store = bs.diag.reshape(len(bs.diag), -1)
    bs.d_c0, bs.d_c1, bs.d_diag = dev(bs.c0), dev(bs.c1), dev(bs.store)
    bs.d_bkeys = [None if k is None else (dev(k[0]), dev(k[1])) for k in bs.bkeys]
    bs.d_gkeys = [None if k is None else (dev(k[0]), dev(k[1])) for k in bs.gkeys]
    o0, o1 = bs.run()
    check_decrypts(case, host(o0), host(o1))
    ks.close()


def test_argument_errors(hip):
    H, ctx = hip
    log_n, sq, sp, dnum, l, B = 3, 4, 2, 2, 4, 1
    n, q, rq, p, rp, kp, ks = _ks_case(H, ctx, log_n, sq, sp, dnum)
    rng = np.random.default_rng(96)
    bs = Bsgs(rng, ks, kp, q, p, l, n, dnum, B, [1, nonid(n, 0)], [1, nonid(n, 1)])
    want = bs.ref(0)
    o0, o1 = bs.run()
    kb, ka = bs._ptrs(bs.d_bkeys, 0), bs._ptrs(bs.d_bkeys, 1)
    gb, ga = bs._ptrs(bs.d_gkeys, 0), bs._ptrs(bs.d_gkeys, 1)
    bad = [
        dict(c0=0), dict(c1=0), dict(out0=0), dict(out1=0), dict(diag=0),          # NULL data
        dict(baby_indices=None), dict(giant_indices=None),                         # NULL index arrays
        dict(baby_key_b=None), dict(baby_key_a=None), dict(giant_key_b=None), dict(giant_key_a=None),
        dict(baby_key_b=[0, 0]), dict(baby_key_a=[0, 0]),                          # NULL key, non-identity step
        dict(giant_key_b=[0, 0]), dict(giant_key_a=[0, 0]),
        dict(baby_indices=[1, 6]), dict(giant_indices=[2, 5]),                     # even indices
        dict(baby_indices=[], baby_key_b=[], baby_key_a=[], present=None),         # nbaby = 0
        dict(giant_indices=[], giant_key_b=[], giant_key_a=[], present=None),      # ngiant = 0
        dict(batch=0),
        dict(diag_stride=(l + sp) * n - 1),
        dict(out1=o0.data_ptr()),                                                  # out0 == out1
        dict(out1=o0.data_ptr() + 8),                                              # out1 one word into out0
        dict(out0=bs.d_c0.data_ptr()), dict(out1=bs.d_c1.data_ptr()),              # outputs aliasing inputs
        dict(out0=bs.d_diag.data_ptr()),
    ]
    for over in bad:
        with pytest.raises(H.MathError):
            bs.run(out=(o0, o1), **over)
    # identity steps ignore their (NULL) keys: the good call's pointers are 0 there
    assert kb[0] == 0 and ka[0] == 0 and gb[0] == 0 and ga[0] == 0
    # the stage calls
    x0, x1, diag, digits, keys = _stage_inputs(rng, kp, q, p, l, n, dnum, B, 2, 2, 2)
    d0, d1, dd, dg = dev(x0), dev(x1), dev(diag), dev(digits)
    dk = [(dev(b), dev(a)) for b, a in keys]
    e0, e1 = zeros(2, B, l + sp, n), zeros(2, B, l + sp, n)
    per, poly = B * (l + sp) * n, (l + sp) * n
    good = dict(size_ql=l, nterm=2, x0=d0.data_ptr(), x1=d1.data_ptr(), x_stride=per, diag=dd.data_ptr(),
                diag_stride=poly, present=None, nsum=2, out0=e0.data_ptr(), out1=e1.data_ptr(), batch=B,
                stream=stream())
    for over in (dict(x0=0), dict(x1=0), dict(diag=0), dict(out0=0), dict(out1=0), dict(nterm=0), dict(nsum=0),
                 dict(batch=0), dict(diag_stride=poly - 1), dict(x_stride=per - 1), dict(out1=e0.data_ptr()),
                 dict(out1=e0.data_ptr() + 8), dict(out0=d0.data_ptr()), dict(out1=dd.data_ptr()),
                 dict(size_ql=sq + 1)):
        with pytest.raises(H.MathError):
            ks.mult_ext_sum(**{**good, **over})
    f0, f1 = zeros(B, l + sp, n), zeros(B, l + sp, n)
    good = dict(size_ql=l, digits=dg.data_ptr(), auto_indices=[5, 3], key_b_ptrs=[b.data_ptr() for b, _ in dk],
                key_a_ptrs=[a.data_ptr() for _, a in dk], addend1=0, nadd=0, out0=f0.data_ptr(), out1=f1.data_ptr(),
                batch=B, stream=stream())
    for over in (dict(digits=0), dict(out0=0), dict(out1=0), dict(auto_indices=None), dict(key_b_ptrs=None),
                 dict(key_a_ptrs=None), dict(auto_indices=[5, 4]), dict(key_b_ptrs=[0, 0]), dict(batch=0),
                 dict(auto_indices=[], key_b_ptrs=[], key_a_ptrs=[]), dict(out1=f0.data_ptr()),
                 dict(out1=f0.data_ptr() + 8), dict(out0=dg.data_ptr()), dict(nadd=1), dict(addend1=e0.data_ptr())):
        with pytest.raises(H.MathError):
            ks.fast_rotation_ext_sum(**{**good, **over})
    for c, out, batch in ((0, f0.data_ptr(), B), (bs.d_c0.data_ptr(), 0, B), (bs.d_c0.data_ptr(), f0.data_ptr(), 0),
                          (bs.d_c0.data_ptr(), bs.d_c0.data_ptr(), B)):
        with pytest.raises(H.MathError):
            ks.ext(l, c, out, batch, stream())
    # the engine is still usable and a good call gives the reference's words
    assert _same(bs.run(), want) and _same((o0, o1), want)
    assert _same(_mult_ext_sum(ks, l, sp, n, x0, x1, diag, None, 2, B),
                 LT.mult_ext_sum_ref(kp, l, x0, x1, diag, None, 2))
    assert _same(_rot_sum(ks, l, sp, n, digits, [5, 3], keys, None, B),
                 LT.fast_rotation_ext_sum_ref(kp, digits, [5, 3], keys))
    ks.close()
