"""CPU: the restatement of BV key switching with a digit size (tests/bv_digits_ref.py) against the algebra
the reference's decomposition and key generation make exact -- "parity unpinned" against reference-run data
(none exists for this path), pinned by identities instead:
  (a) sum_j win_{i,j} 2^{j r} = coef_i exactly, every window below 2^r;
  (b) tower i of digit (i, j) in coefficient form is the window, tower k SwitchModulus of it;
  (c) with keys bv = filtered - (a s_new + e), filtered_{i,j} = s_old_i 2^{j r} in tower i only:
      ct0 + ct1 s_new = c s_old - sum_d digit_d e_d, exactly, tower by tower;
  (d) when no window is re-centred or reduced, the CRT-centred c s_old - (ct0 + ct1 s_new) is the integer
      polynomial sum_d D_d e_d, bounded by nWindows N (2^r - 1) E; the same chain at digitSize = 0 exceeds
      that bound -- the reason a digit size exists;
  (e) with r at least every tower's bit length the digits are CRTDecompose(0)'s;
  (f) a lower level uses a prefix of the key."""
import numpy as np
import pytest

import bv_digits_ref as R
import keyswitch as K
import oracle as O
from test_mixed_moduli_oracle import bv_chain, mixed_chain, uniform


def _negacyclic(a, b):
    """Product of two integer polynomials modulo x^n + 1 (Python integers)."""
    n = len(a)
    out = [0] * n
    for i, x in enumerate(a):
        if x:
            for j, y in enumerate(b):
                k = i + j
                if k < n:
                    out[k] += x * y
                else:
                    out[k - n] -= x * y
    return out


@pytest.mark.parametrize("r", [1, 7, 13, 29, 30])
@pytest.mark.parametrize("generic", [False, True])
def test_windows_and_digits(r, generic):
    log_n = 6
    n = 1 << log_n
    q, rq = bv_chain(log_n, generic)
    rng = np.random.default_rng(40 + r)
    c = uniform(rng, 2, q, n)
    coef = K.set_format(c, q, rq, False)
    d = R.crt_decompose(c, q, rq, r)
    idx = R.digit_index(q, r)
    assert d.shape[1] == len(idx) == R.digit_count(q, r) == sum(-(-m.bit_length() // r) for m in q)
    dcoef = np.stack([K.set_format(np.ascontiguousarray(d[:, k]), q, rq, False) for k in range(len(idx))], axis=1)
    for i in range(len(q)):
        acc = np.zeros_like(coef[:, i])
        for dd, (ii, j) in enumerate(idx):
            if ii != i:
                continue
            win = dcoef[:, dd, i]                                        # (b): tower i is the window itself
            assert np.array_equal(win, R.window(coef[:, i], j, r)) and int(win.max()) < (1 << r)
            acc += win << np.uint64(j * r)                               # (a)
            for k in range(len(q)):
                assert np.array_equal(dcoef[:, dd, k], K.switch_modulus(win, q[i], q[k]))
        assert np.array_equal(acc, coef[:, i])


@pytest.mark.parametrize("r,generic", [(7, False), (29, False), (30, True), (13, True)])
def test_key_identity(r, generic):
    """(c), (f) and KeySwitchInPlace on two and three elements."""
    log_n = 6
    n = 1 << log_n
    q, rq = bv_chain(log_n, generic)
    T = len(q)
    rng = np.random.default_rng(60 + r)
    s_old = K.small_poly_eval(rng.integers(-1, 2, size=n), q, rq)[0]
    s_new = K.small_poly_eval(rng.integers(-1, 2, size=n), q, rq)[0]
    kb, ka, es, _ = R.bv_keygen_digits(q, rq, s_old, s_new, r, rng)
    for L in (T, T - 1):                                                 # (f): the level's digits meet a key prefix
        ql, rl = q[:L], rq[:L]
        c = uniform(rng, 1, ql, n)
        d = R.crt_decompose(c, ql, rl, r)
        nd = d.shape[1]
        assert R.digit_index(ql, r) == R.digit_index(q, r)[:nd]
        o0, o1 = R.bv_fast_core_digits(d, kb, ka, ql)
        lhs = O.eltwise("add", o0, O.eltwise("mul", o1, s_new[None, :L], ql), ql)
        noise = O.eltwise("mul", d[:, 0], np.ascontiguousarray(es[0:1, :L]), ql)
        for k in range(1, nd):
            noise = O.eltwise("add", noise, O.eltwise("mul", d[:, k], np.ascontiguousarray(es[k:k + 1, :L]), ql), ql)
        cs = O.eltwise("mul", c, np.ascontiguousarray(s_old[None, :L]), ql)
        assert np.array_equal(lhs, O.eltwise("sub", cs, noise, ql))
        a0, a1 = uniform(rng, 1, ql, n), uniform(rng, 1, ql, n)
        c0, c1 = R.key_switch_in_place([a0, c], kb, ka, ql, rl, r)
        assert np.array_equal(c0, O.eltwise("add", a0, o0, ql)) and np.array_equal(c1, o1)
        c0, c1 = R.key_switch_in_place([a0, a1, c], kb, ka, ql, rl, r)
        assert np.array_equal(c0, O.eltwise("add", a0, o0, ql)) and np.array_equal(c1, O.eltwise("add", a1, o1, ql))


def test_noise_is_bounded_by_the_digit_size():
    """(d): r = 10 on towers of 45 and 40 bits (r <= min bitlen - 2, so every window is at most q_i / 2 and
    below every q_k: no lift re-centres or reduces)."""
    log_n, r, E = 5, 10, 3
    n = 1 << log_n
    q, rq = mixed_chain(log_n, [45, 40, 40])
    assert r <= min(m.bit_length() for m in q) - 2
    rng = np.random.default_rng(8)
    c = uniform(rng, 1, q, n)
    so, sn = rng.integers(-1, 2, size=n), rng.integers(-1, 2, size=n)
    s_old, s_new = K.small_poly_eval(so, q, rq)[0], K.small_poly_eval(sn, q, rq)[0]
    kb, ka, es, ec = R.bv_keygen_digits(q, rq, s_old, s_new, r, rng, E)
    coef = K.set_format(c, q, rq, False)
    idx = R.digit_index(q, r)
    wins = [R.window(coef[0, i], j, r) for i, j in idx]
    assert all(int(w.max()) <= min(q) // 2 for w in wins)
    o0, o1 = R.bv_fast_core_digits(R.crt_decompose(c, q, rq, r), kb, ka, q)

    def centred_error(o0, o1):
        lhs = O.eltwise("add", o0, O.eltwise("mul", o1, s_new[None], q), q)
        diff = O.eltwise("sub", O.eltwise("mul", c, s_old[None], q), lhs, q)
        return K.crt_centered(K.set_format(diff, q, rq, False)[0], q)

    want = [0] * n
    for w, e in zip(wins, ec):
        want = [x + y for x, y in zip(want, _negacyclic([int(v) for v in w], [int(v) for v in e]))]
    err = centred_error(o0, o1)
    assert err == want
    bound = len(idx) * n * ((1 << r) - 1) * E
    assert max(abs(v) for v in err) <= bound
    # digitSize = 0 on the same chain, the same c and secrets: the error grows with q_i, past that bound
    kb0, ka0, _ = K.bv_keygen(q, rq, s_old, s_new, rng, E)
    z0, z1 = K.bv_fast_core(K.crt_decompose0(c, q, rq), kb0, ka0, q)
    assert max(abs(v) for v in centred_error(z0, z1)) > bound


@pytest.mark.parametrize("generic", [False, True])
def test_one_window_per_tower_is_digit_size_zero(generic):
    """(e), on a chain of at most 30 bits (r = 30 is the largest digit size), and tower by tower on bv_chain,
    whose 30-bit tower has one window at r = 30."""
    log_n = 6
    n = 1 << log_n
    q, rq = mixed_chain(log_n, [30, 28, 22], generic)
    rng = np.random.default_rng(2)
    c = uniform(rng, 2, q, n)
    assert R.windows(q, 30) == [1, 1, 1]
    assert np.array_equal(R.crt_decompose(c, q, rq, 30), K.crt_decompose0(c, q, rq))
    assert np.array_equal(R.crt_decompose(c, q, rq, 0), K.crt_decompose0(c, q, rq))
    q, rq = bv_chain(log_n, generic)
    c = uniform(rng, 1, q, n)
    d, d0 = R.crt_decompose(c, q, rq, 30), K.crt_decompose0(c, q, rq)
    assert R.windows(q, 30) == [2, 2, 2, 1]
    assert np.array_equal(d[:, 6], d0[:, 3])
