"""GPU parity of the hoisted rotations (ofhe_hip_ks_fast_rotation_ext /
ofhe_hip_ks_fast_rotation) against tests/rotation_ref.py, bit for bit.

Every case uses distinct random keys per rotation and indices drawn from
{1, 5^r mod 2N, 2N - 1, an odd value >= 2N}.  The reference of one (shape,
level) is computed once for batch 3 and cap + 1 rotations; the smaller calls
(batch 1, nrot 1 and 3) are compared with its slices, the per-rotation and
per-entry results being independent.
"""
import numpy as np
import pytest

import keyswitch as K
import oracle as O
import rotation_ref as R
from test_gpu_caller_stream import OnStream, delay  # noqa: F401  (delay is a fixture)
from test_gpu_keyswitch import _ks_case, _uniform
from test_gpu_parity import dev, host, stream
from test_rotation_oracle import coeff_automorphism_signed

pytestmark = pytest.mark.gpu

SHAPES = [
    (1, 2, 1, 1, False),    # N = 2: below a wave
    (3, 4, 2, 2, False),    # N = 8: below a workgroup block
    (6, 5, 3, 2, False),    # partial last digit
    (12, 6, 2, 3, True),    # generic moduli
    (5, 8, 2, 4, False),    # beta = 4
    (5, 10, 2, 5, False),   # beta = 5: the 128-bit variant
    (13, 8, 3, 3, False),   # several blocks per row
    (16, 6, 2, 3, False),   # batch 1, nrot 2
]


def _levels(sq, dnum):
    alpha = -(-sq // dnum)
    return sorted({sq, max(1, sq - 1), max(1, alpha - 1)}, reverse=True)


CASES = [s + (l,) for s in SHAPES for l in _levels(s[1], s[3])]


def indices_for(n, nrot):
    """1, 5, 2N - 1, an odd value >= 2N, then 5^r mod 2N."""
    head = [1, 5 % (2 * n), 2 * n - 1, 2 * n + 3]
    return (head + [pow(5, r, 2 * n) for r in range(2, nrot)])[:nrot]


class Rot:
    """Device copies of one digit set, c0 and nrot keys, and the calls on them."""

    def __init__(self, ks, l, sp, n, digits, c0, keys, indices):
        self.ks, self.l, self.sp, self.n = ks, l, sp, n
        self.h_digits, self.h_c0, self.h_keys, self.indices = digits, c0, keys, indices
        self.d_digits, self.d_c0 = dev(digits), dev(c0)
        self.d_keys = [(dev(kb), dev(ka)) for kb, ka in keys]

    def _args(self, nrot):
        return (self.indices[:nrot], [b.data_ptr() for b, _ in self.d_keys[:nrot]],
                [a.data_ptr() for _, a in self.d_keys[:nrot]])

    def ext(self, nrot, batch, add_first, s=None):
        import torch

        o0 = torch.zeros((nrot, batch, self.l + self.sp, self.n), dtype=torch.int64, device="cuda")
        o1 = torch.zeros_like(o0)
        idx, kb, ka = self._args(nrot)
        self.ks.fast_rotation_ext(self.l, self.d_digits.data_ptr(), self.d_c0.data_ptr() if add_first else 0, idx,
                                  kb, ka, o0.data_ptr(), o1.data_ptr(), batch, stream() if s is None else s)
        return o0, o1

    def plain(self, nrot, batch, t, s=None):
        import torch

        o0 = torch.zeros((nrot, batch, self.l, self.n), dtype=torch.int64, device="cuda")
        o1 = torch.zeros_like(o0)
        idx, kb, ka = self._args(nrot)
        self.ks.fast_rotation(self.l, self.d_digits.data_ptr(), self.d_c0.data_ptr(), idx, kb, ka, o0.data_ptr(),
                              o1.data_ptr(), t, batch, stream() if s is None else s)
        return o0, o1

    def inputs_unchanged(self):
        ok = np.array_equal(host(self.d_digits), self.h_digits) and np.array_equal(host(self.d_c0), self.h_c0)
        return ok and all(np.array_equal(host(b), kb) and np.array_equal(host(a), ka)
                          for (b, a), (kb, ka) in zip(self.d_keys, self.h_keys))


def _inputs(rng, kp, q, p, l, n, batch, nrot, dnum):
    beta = kp.beta(l)
    digits = np.stack([_uniform(rng, beta, q[:l] + p, n) for _ in range(batch)])
    c0 = _uniform(rng, batch, q[:l], n)
    keys = [(_uniform(rng, dnum, q + p, n), _uniform(rng, dnum, q + p, n)) for _ in range(nrot)]
    return digits, c0, keys


def _same(got, want):
    return all(np.array_equal(host(g), w) for g, w in zip(got, want))


@pytest.mark.parametrize("log_n,sq,sp,dnum,generic,l", CASES)
def test_fast_rotation_parity(hip, log_n, sq, sp, dnum, generic, l):
    H, ctx = hip
    n, q, rq, p, rp, kp, ks = _ks_case(H, ctx, log_n, sq, sp, dnum, generic)
    big = log_n >= 16
    B, nmax = (1, 2) if big else (3, H.KS_ROT_CAP + 1)
    rng = np.random.default_rng(1000 * log_n + l)
    digits, c0, keys = _inputs(rng, kp, q, p, l, n, B, nmax, dnum)
    idx = indices_for(n, nmax)
    rot = Rot(ks, l, sp, n, digits, c0, keys, idx)
    cts = R.inner_products(kp, digits, keys)
    ext_add = R.fast_rotation_ext_ref(kp, digits, c0, idx, keys, cts=cts)
    ext_no = R.fast_rotation_ext_ref(kp, digits, None, idx, keys, cts=cts)
    nt = min(nmax, 3)  # t = 65537 on the first rotations: ModDown's t path is per polynomial
    plain0 = R.fast_rotation_ref(kp, digits, c0, idx, keys, 0, cts=cts)
    plain_t = R.fast_rotation_ref(kp, digits, c0, idx[:nt], keys[:nt], 65537, cts=cts[:nt])
    # the largest call of each kind
    assert _same(rot.ext(nmax, B, True), ext_add), "Ext, addFirst"
    assert _same(rot.ext(nmax, B, False), ext_no), "Ext"
    assert _same(rot.plain(nmax, B, 0), plain0), "non-Ext, t = 0"
    assert _same(rot.plain(nt, B, 65537), plain_t), "non-Ext, t = 65537"
    assert rot.inputs_unchanged()
    # batch 1 and nrot 1, 3: slices of the same reference
    for nrot, batch in sorted({(1, 1), (min(3, nmax), 1), (1, B)}):
        cut = lambda w: [x[:nrot, :batch] for x in w]  # noqa: E731
        assert _same(rot.ext(nrot, batch, True), cut(ext_add)), (nrot, batch)
        assert _same(rot.ext(nrot, batch, False), cut(ext_no)), (nrot, batch)
        assert _same(rot.plain(nrot, batch, 0), cut(plain0)), (nrot, batch)
        assert _same(rot.plain(min(nrot, nt), batch, 65537), [x[:min(nrot, nt), :batch] for x in plain_t]), (nrot, batch)
    ks.close()


def test_fast_rotation_single_stream_engine(hip):
    H, ctx = hip
    log_n, sq, sp, dnum, l, B, nrot = 6, 5, 3, 2, 5, 2, 3
    n, q, rq, p, rp, kp, ks = _ks_case(H, ctx, log_n, sq, sp, dnum, options=H.KsOptions(single_stream=1))
    rng = np.random.default_rng(61)
    digits, c0, keys = _inputs(rng, kp, q, p, l, n, B, nrot, dnum)
    idx = indices_for(n, nrot)
    rot = Rot(ks, l, sp, n, digits, c0, keys, idx)
    assert _same(rot.ext(nrot, B, True), R.fast_rotation_ext_ref(kp, digits, c0, idx, keys))
    assert _same(rot.plain(nrot, B, 65537), R.fast_rotation_ref(kp, digits, c0, idx, keys, 65537))
    ks.close()


def test_fast_rotation_on_caller_stream(hip, delay):  # noqa: F811
    """Both calls from a non-default stream, waited on through that stream alone."""
    H, ctx = hip
    log_n, sq, sp, dnum, l, B, nrot = 10, 6, 2, 3, 6, 2, 3
    n, q, rq, p, rp, kp, ks = _ks_case(H, ctx, log_n, sq, sp, dnum)
    rng = np.random.default_rng(62)
    digits, c0, keys = _inputs(rng, kp, q, p, l, n, B, nrot, dnum)
    idx = indices_for(n, nrot)
    st = OnStream(delay)
    dd, dc = st.input(digits), st.input(c0)
    dk = [(st.input(kb), st.input(ka)) for kb, ka in keys]
    e0, e1 = st.output(nrot, B, l + sp, n), st.output(nrot, B, l + sp, n)
    o0, o1 = st.output(nrot, B, l, n), st.output(nrot, B, l, n)
    kb, ka = [b.data_ptr() for b, _ in dk], [a.data_ptr() for _, a in dk]
    st.begin()
    ks.fast_rotation_ext(l, dd.data_ptr(), dc.data_ptr(), idx, kb, ka, e0.data_ptr(), e1.data_ptr(), B, st.h)
    ks.fast_rotation(l, dd.data_ptr(), dc.data_ptr(), idx, kb, ka, o0.data_ptr(), o1.data_ptr(), 0, B, st.h)
    st.fetch(e0, e1, o0, o1)
    g = st.wait()
    cts = R.inner_products(kp, digits, keys)
    w = R.fast_rotation_ext_ref(kp, digits, c0, idx, keys, cts=cts) + R.fast_rotation_ref(kp, digits, c0, idx, keys, 0,
                                                                                           cts=cts)
    assert all(np.array_equal(a, b) for a, b in zip(g, w))
    import torch

    torch.cuda.synchronize()
    ks.close()


def test_fast_rotation_semantics_with_real_keys(hip):
    """precompute -> fast_rotation / fast_rotation_ext + mod_down on the GPU
    decrypt under s to sigma_5(c0 + c1 s) (keys: KeySwitchGen(s, sigma_{5^-1}(s)))."""
    H, ctx = hip
    import torch

    log_n, sq, sp, dnum, k = 6, 5, 3, 2, 5
    n, q, rq, p, rp, kp, ks = _ks_case(H, ctx, log_n, sq, sp, dnum)
    rng = np.random.default_rng(7)
    s = K.ternary(n, rng)
    s_eval = K.small_poly_eval(s, q, rq)
    c0 = K.set_format(_uniform(rng, 1, q, n), q, rq, True)
    c1 = K.set_format(_uniform(rng, 1, q, n), q, rq, True)
    kb, ka = K.keyswitch_gen(kp, s, coeff_automorphism_signed(s, R.inverse_index(k, n)), rng)
    dc0, dc1, dkb, dka = dev(c0), dev(c1), dev(kb), dev(ka)
    dg = torch.empty((1, kp.beta(sq), sq + sp, n), dtype=torch.int64, device="cuda")
    ks.precompute(sq, dc1.data_ptr(), dg.data_ptr(), 1, stream())
    o0 = torch.empty((1, 1, sq, n), dtype=torch.int64, device="cuda")
    o1, m0, m1 = torch.empty_like(o0), torch.empty_like(o0), torch.empty_like(o0)
    e0 = torch.empty((1, 1, sq + sp, n), dtype=torch.int64, device="cuda")
    e1 = torch.empty_like(e0)
    ks.fast_rotation(sq, dg.data_ptr(), dc0.data_ptr(), [k], [dkb.data_ptr()], [dka.data_ptr()], o0.data_ptr(),
                     o1.data_ptr(), 0, 1, stream())
    ks.fast_rotation_ext(sq, dg.data_ptr(), dc0.data_ptr(), [k], [dkb.data_ptr()], [dka.data_ptr()], e0.data_ptr(),
                         e1.data_ptr(), 1, stream())
    ks.mod_down(sq, e0.data_ptr(), m0.data_ptr(), 0, 1, stream())
    ks.mod_down(sq, e1.data_ptr(), m1.data_ptr(), 0, 1, stream())
    msg = R.sigma(O.eltwise("add", c0, O.eltwise("mul", c1, s_eval, q), q), k)
    for a, b in ((o0, o1), (m0, m1)):
        lhs = O.eltwise("add", host(a)[0], O.eltwise("mul", host(b)[0], s_eval, q), q)
        d = K.set_format(O.eltwise("sub", lhs, msg, q), q, rq, False)
        err = max(abs(e) for e in K.crt_centered(d[0], q))
        assert err < 1 << 20, err.bit_length()
    ks.close()


def test_fast_rotation_argument_errors(hip):
    H, ctx = hip
    log_n, sq, sp, dnum, l, B, nrot = 3, 4, 2, 2, 4, 1, 2
    n, q, rq, p, rp, kp, ks = _ks_case(H, ctx, log_n, sq, sp, dnum)
    rng = np.random.default_rng(63)
    digits, c0, keys = _inputs(rng, kp, q, p, l, n, B, nrot, dnum)
    idx = indices_for(n, nrot)
    rot = Rot(ks, l, sp, n, digits, c0, keys, idx)
    e0, e1 = rot.ext(nrot, B, True)
    o0, o1 = rot.plain(nrot, B, 0)
    _, kb, ka = rot._args(nrot)
    dg, dc = rot.d_digits.data_ptr(), rot.d_c0.data_ptr()
    bad = [
        ([5, 6], kb, ka, e0.data_ptr(), e1.data_ptr()),   # even index
        ([], [], [], e0.data_ptr(), e1.data_ptr()),       # nrot = 0
        (idx, kb, ka, e0.data_ptr(), e0.data_ptr()),      # out0 == out1
        (idx, None, ka, e0.data_ptr(), e1.data_ptr()),    # NULL pointer arrays
        (idx, kb, None, e0.data_ptr(), e1.data_ptr()),
        (None, kb, ka, e0.data_ptr(), e1.data_ptr()),
    ]
    for i, b, a, x0, x1 in bad:
        with pytest.raises(H.MathError):
            ks.fast_rotation_ext(l, dg, dc, i, b, a, x0, x1, B, stream())
        with pytest.raises(H.MathError):
            ks.fast_rotation(l, dg, dc, i, b, a, x0, x1, 0, B, stream())
    with pytest.raises(H.MathError):  # the non-Ext call needs c0
        ks.fast_rotation(l, dg, 0, idx, kb, ka, o0.data_ptr(), o1.data_ptr(), 0, B, stream())
    with pytest.raises(H.MathError):
        ks.fast_rotation_ext(l, dg, dc, idx, kb, ka, e0.data_ptr(), e1.data_ptr(), 0, stream())  # batch = 0
    # the engine is still usable
    assert _same(rot.ext(nrot, B, True), R.fast_rotation_ext_ref(kp, digits, c0, idx, keys))
    assert _same(rot.plain(nrot, B, 0), R.fast_rotation_ref(kp, digits, c0, idx, keys))
    ks.close()
