"""CPU checks of the CKKS / BGV multiplication's reference composition (tests/she_mult_ref.py), the yardstick
of tests/test_gpu_she_mult.py, and of the identity the engine builds its CKKS rescaling table from.

1. QlQlInvModqlDivqlModq[i] = q_i - qlInvModq[i], against rescale_tables (Python integers).
2. EvalSquare is EvalMult(c, c); the order of a relinearisation's key switches does not show in the words.
3. Semantics with real keys: CKKS decrypts to m1 m2 / prod(q_dropped) within a derived bound, BGV to
   m1 m2 prod(q_dropped)^-1 mod t exactly; a 4-element ciphertext relinearises under keys for s^2 and s^3.
"""
import math
from fractions import Fraction

import numpy as np
import pytest

import keyswitch as K
import oracle as O
import she_mult_ref as S
from test_keyswitch_oracle import _bases, _uniform
from tier2_cases import _moduli

KEY_ERR = 3   # |e| of keyswitch_gen's error polynomials
ENC_ERR = 3   # |e| of the encryptions below


# ---------------------------------------------------------------------------
# 1. the table identity
# ---------------------------------------------------------------------------
def _check_identity(q):
    for l in range(1, len(q)):           # dropping tower l, towers 0..l present
        c, a = K.rescale_tables(q[:l + 1])
        for i in range(l):
            assert a[i] == pow(q[l], -1, q[i])
            assert c[i] == q[i] - a[i], (l, i)


def test_ckks_table_is_minus_ql_inverse_on_a_mixed_chain():
    """Q = prod_{j<l} q_j, b = Q^-1 mod q_l: b Q = 1 + k q_l, floor(b Q / q_l) = k, and Q = 0 (mod q_i) gives
    k q_l = -1 (mod q_i): the table is q_i - q_l^-1 mod q_i.  Towers of 22 to 60 bits in one chain."""
    spans = []
    for seed in range(6):
        q, _, _ = _moduli(np.random.default_rng([77, seed]), 6, 7, 22)
        spans.append((min(q).bit_length(), max(q).bit_length()))
        _check_identity(q)
    assert min(lo for lo, _ in spans) <= 26 and max(hi for _, hi in spans) >= 58 and any(hi - lo >= 24 for lo, hi in spans)


@pytest.mark.parametrize("log_n,towers", [(4, 3), (10, 8), (16, 6)])
def test_ckks_table_is_minus_ql_inverse_on_moduli_chain(log_n, towers):
    _check_identity(O.moduli_chain(log_n, towers)[0])


# ---------------------------------------------------------------------------
# 2. identities of the restatement
# ---------------------------------------------------------------------------
def _params(log_n, sq, sp, dnum):
    n = 1 << log_n
    q, rq, p, rp = _bases(log_n, sq, sp)
    return n, q, rq, p, rp, K.KeySwitchParams(n, q, rq, p, rp, dnum)


@pytest.mark.parametrize("scheme,t", [(S.CKKS, 0), (S.BGV, 65537)])
def test_square_is_mult_by_itself(scheme, t):
    n, q, rq, p, rp, kp = _params(4, 4, 2, 2)
    rng = np.random.default_rng(3)
    for l in (4, 3):
        c0, c1 = _uniform(rng, 2, q[:l], n), _uniform(rng, 2, q[:l], n)
        kb, ka = _uniform(rng, 2, q + p, n), _uniform(rng, 2, q + p, n)
        for levels in (0, 1, 2):
            a = S.eval_mult(kp, c0, c1, None, None, kb, ka, scheme, t, levels)
            b = S.eval_mult(kp, c0, c1, c0, c1, kb, ka, scheme, t, levels)
            assert a[0].shape == (2, l - levels, n)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_relinearisation_order_does_not_show():
    n, q, rq, p, rp, kp = _params(4, 3, 1, 3)
    rng = np.random.default_rng(4)
    cv = [_uniform(rng, 2, q, n) for _ in range(4)]
    k2 = (_uniform(rng, 3, q + p, n), _uniform(rng, 3, q + p, n))
    k3 = (_uniform(rng, 3, q + p, n), _uniform(rng, 3, q + p, n))
    a = S.relinearize(kp, cv, [k2, k3])
    b = S.relinearize(kp, [cv[0], cv[1], cv[3], cv[2]], [k3, k2])
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    only2 = S.relinearize(kp, cv[:3], [k2])
    assert not np.array_equal(a[0], only2[0])


# ---------------------------------------------------------------------------
# 3. semantics with real keys
# ---------------------------------------------------------------------------
def negacyclic(a, b):
    """a b mod X^N + 1 over the integers (Python integers)."""
    n = len(a)
    out = [0] * n
    for i, x in enumerate(a):
        x = int(x)
        if x:
            for j, y in enumerate(b):
                k = i + j
                if k < n:
                    out[k] += x * int(y)
                else:
                    out[k - n] -= x * int(y)
    return out


def encrypt(kp, s, value, rng):
    """(c0, c1) over q with c0 + c1 s = value exactly (the caller puts the noise into value)."""
    q, rq = kp.q, kp.rq
    c1 = K.set_format(_uniform(rng, 1, q, kp.n), q, rq, True)
    s_eval = K.small_poly_eval(s, q, rq)
    v = K.small_poly_eval(np.asarray(value, dtype=np.int64), q, rq)
    return O.eltwise("sub", v, O.eltwise("mul", c1, s_eval, q), q), c1


def decrypt(kp, s, elements):
    """Centred integers of sum_j elements[j] s^j over the towers the elements have."""
    l = elements[0].shape[1]
    q, rq = kp.q[:l], kp.rq[:l]
    acc = np.zeros_like(elements[0])
    spow = [1] + [0] * (kp.n - 1)
    for e in elements:
        acc = O.eltwise("add", acc, O.eltwise("mul", e, K.small_poly_eval(np.asarray(spow, dtype=np.int64), q, rq), q), q)
        spow = negacyclic(spow, s)
    return K.crt_centered(K.set_format(acc, q, rq, False)[0], q)


def key_switch_noise(kp, l, h, key_err=KEY_ERR):
    """Bound on |ab0 + ab1 s - c s_old| of one KeySwitchCore at level l, for a secret of h non-zero ternary
    coefficients.  At scale P the key errors contribute sum_d digit_d e_d with digit_d in [0, alpha Q_d)
    (ApproxSwitchCRTBasis without its correction) over beta digits: key_err beta alpha N max(Q_d), divided by
    P; the two ApproxModDowns subtract (x0 + x1 s) / P with x in [0, sp P): sp (1 + h)."""
    beta, alpha, n = kp.beta(l), kp.alpha, kp.n
    qd = max(math.prod(kp.q[kp.digit(l, j)[0]:sum(kp.digit(l, j))]) for j in range(beta))
    return Fraction(key_err * beta * alpha * n * qd, math.prod(kp.p)) + len(kp.p) * (1 + h)


CASES = [(4, 3, 1, 3), (5, 4, 2, 2), (6, 4, 1, 4), (6, 3, 2, 3)]  # log_n, Q, P, dnum


@pytest.mark.parametrize("log_n,sq,sp,dnum", CASES)
@pytest.mark.parametrize("square", [False, True])
def test_ckks_decrypts_to_the_scaled_product(log_n, sq, sp, dnum, square):
    """Dec(out) D = m1 m2 + residual, D = prod(q_dropped).  With Dec(ct_i) = M_i = m_i + e_i (|e_i| <= 3):
    the tensor product decrypts to M1 M2 exactly; |M1 M2 - m1 m2| <= N (|m1| + |m2| + 3) 3; the key switch of
    the third element under KeySwitchGen(s^2 -> s) adds key_switch_noise; each DropLastElementAndScale divides
    by q_l and adds at most 1 per element, 1 + h on the decryption, and the later levels only shrink that:
        |Dec(out) D - m1 m2| <= N (|m1| + |m2| + 3) 3 + key_switch_noise + D levels (1 + h)."""
    n, q, rq, p, rp, kp = _params(log_n, sq, sp, dnum)
    rng = np.random.default_rng([log_n, sq, sp, dnum, int(square)])
    s = K.ternary(n, rng)
    h = int(np.count_nonzero(s))
    bm = 1 << 40
    kb, ka = K.keyswitch_gen(kp, negacyclic(s, s), s, rng, KEY_ERR)
    m = [rng.integers(-bm, bm + 1, size=n) for _ in range(2)]
    if square:
        m[1] = m[0]
    cts = [encrypt(kp, s, mi + rng.integers(-ENC_ERR, ENC_ERR + 1, size=n), rng) for mi in m]
    if square:
        cts[1] = (None, None)
    want = negacyclic(m[0], m[1])
    for levels in range(0, min(sq, 3)):
        o0, o1 = S.eval_mult(kp, cts[0][0], cts[0][1], cts[1][0], cts[1][1], kb, ka, S.CKKS, 0, levels)
        D = math.prod(q[sq - levels:])
        dec = decrypt(kp, s, [o0, o1])
        err = max(abs(d * D - w) for d, w in zip(dec, want))
        bound = math.ceil(n * (2 * bm + ENC_ERR) * ENC_ERR + key_switch_noise(kp, sq, h) + D * levels * (1 + h))
        print(f"levels {levels}: residual {err.bit_length()} bits, bound {bound.bit_length()} bits, "
              f"product {max(abs(w) for w in want).bit_length()} bits")
        assert err <= bound, (levels, err, bound)
        # a wrong word, uniform mod Q_l, cannot pass; and the product is far above the bound
        assert bound << 40 < math.prod(q)
        if levels <= 1:
            assert max(abs(w) for w in want) > bound << 6


@pytest.mark.parametrize("log_n,sq,sp,dnum", CASES)
@pytest.mark.parametrize("t", [2, 65537])
def test_bgv_decrypts_to_the_product_mod_t(log_n, sq, sp, dnum, t):
    """BGV: Dec(ct) = m + t e, the keys' errors are multiples of t, ApproxModDown with t and ModReduce keep
    every rounding a multiple of t and divide by P (undone by the key's factor P) and by q_l:
    Dec(out) = m1 m2 prod(q_dropped)^-1 (mod t), exactly, product and square."""
    n, q, rq, p, rp, kp = _params(log_n, sq, sp, dnum)
    rng = np.random.default_rng([log_n, sq, sp, dnum, t])
    s = K.ternary(n, rng)
    qp, rqp = q + p, rq + rp
    kb, ka = K.keyswitch_gen(kp, negacyclic(s, s), s, rng, 0)          # no error, then t e added to b
    for d in range(kb.shape[0]):
        e = K.small_poly_eval(t * rng.integers(-KEY_ERR, KEY_ERR + 1, size=n), qp, rqp)
        kb[d] = O.eltwise("add", kb[d][None], e, qp)[0]
    m = [rng.integers(0, t, size=n) for _ in range(2)]
    cts = [encrypt(kp, s, mi + t * rng.integers(-ENC_ERR, ENC_ERR + 1, size=n), rng) for mi in m]
    for square in (False, True):
        a, b = cts[0], ((None, None) if square else cts[1])
        prod = negacyclic(m[0], m[0] if square else m[1])
        for levels in range(0, min(sq, 3)):
            o0, o1 = S.eval_mult(kp, a[0], a[1], b[0], b[1], kb, ka, S.BGV, t, levels)
            dinv = pow(math.prod(q[sq - levels:]) % t, -1, t) if levels else 1
            dec = decrypt(kp, s, [o0, o1])
            assert max(abs(d) for d in dec) << 20 < math.prod(q[:sq - levels])   # far from wrapping
            assert [d % t for d in dec] == [w * dinv % t for w in prod], (square, levels)


@pytest.mark.parametrize("log_n,sq,sp,dnum", CASES[:3])
def test_four_elements_relinearise_under_keys_for_s2_and_s3(log_n, sq, sp, dnum):
    """out0 + out1 s = c0 + c1 s + c2 s^2 + c3 s^3 + residual, |residual| <= 2 key_switch_noise; then one
    rescaling of the pair divides it by q_l up to 1 + h."""
    n, q, rq, p, rp, kp = _params(log_n, sq, sp, dnum)
    rng = np.random.default_rng([log_n, sq, sp, dnum])
    s = K.ternary(n, rng)
    h = int(np.count_nonzero(s))
    s2 = negacyclic(s, s)
    s3 = negacyclic(s2, s)
    keys = [K.keyswitch_gen(kp, s2, s, rng, KEY_ERR), K.keyswitch_gen(kp, s3, s, rng, KEY_ERR)]
    cv = [K.set_format(_uniform(rng, 1, q, n), q, rq, True) for _ in range(4)]
    o0, o1 = S.relinearize(kp, cv, keys)
    Q = math.prod(q)
    centre = lambda v: (v + Q // 2) % Q - Q // 2  # noqa: E731
    want = decrypt(kp, s, cv)
    got = decrypt(kp, s, [o0, o1])
    err = max(abs(centre(g - w)) for g, w in zip(got, want))
    bound = math.ceil(2 * key_switch_noise(kp, sq, h))
    print(f"residual {err.bit_length()} bits, bound {bound.bit_length()} bits, Q {Q.bit_length()} bits")
    assert bound << 40 < Q and err <= bound
    # dropping a key switch from the computation fails the same check
    p0, p1 = S.relinearize(kp, cv[:3], keys[:1])
    bad = decrypt(kp, s, [p0, p1])
    assert max(abs(centre(g - w)) for g, w in zip(bad, want)) > bound << 40
    r0, r1 = S.rescale(kp, [o0, o1], S.CKKS, 0, 1)
    low = decrypt(kp, s, [r0, r1])
    Ql = math.prod(q[:-1])
    c2 = lambda v: (v + Ql // 2) % Ql - Ql // 2  # noqa: E731
    assert max(abs(c2(lo * q[-1] - g)) for lo, g in zip(low, got)) <= q[-1] * (1 + h)
