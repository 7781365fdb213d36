"""Restatement of PKEBGVRNS::Decrypt (bgvrns-pke.cpp:44-99), PKERNS::DecryptCore (rns-pke.cpp:199-224) and
the ModReduce chain Q_l -> q_0, built from the oracle's own steps: keyswitch.mod_reduce
(DCRTPolyImpl::ModReduce, dcrtpoly-impl.h:792-812, which calls keyswitch.switch_modulus), keyswitch.set_format
and the element-wise ops of oracle.py, plus NativeVectorT::Mod(t) (mubintvecnat.cpp:139-166, 379-384) written out.
The tables are computed from their definitions (bgvrns-cryptoparameters.cpp:91-107) with Python integers.

Also what the tests of the chain share: the chains of moduli, the planted inputs, a BGV encryption with the
noise bound under which both branches certainly decrypt, and the scaling-factor definition."""
from fractions import Fraction

import numpy as np

import keyswitch as K
import oracle as O


# ---- tables -----------------------------------------------------------------------------------------------
def neg_t_inv_modq(q, t):
    """negtInvModq[j] = q_j - t^-1 mod q_j (bgvrns-cryptoparameters.cpp:97); None where t is not invertible"""
    out = []
    for m in q:
        try:
            out.append(int(m) - pow(int(t) % int(m), -1, int(m)))
        except ValueError:
            out.append(None)
    return out


def ql_inv_modq(q):
    """qlInvModq[j][i] = q_j^-1 mod q_i, i < j (:101-106)"""
    return [[pow(int(q[j]), -1, int(q[i])) for i in range(j)] for j in range(len(q))]


# ---- NativeVectorT::Mod(t), the three cases ---------------------------------------------------------------
def mod_t(v, q0, t):
    """mubintvecnat.cpp:139-166 on words mod q0 (PolyImpl::DecryptionCRTInterpolate, poly-impl.h:566-575)"""
    v = np.asarray(v, dtype=np.uint64).copy()
    half = np.uint64(q0 >> 1)
    if t == 2:  # ModByTwoEq (:379-384)
        return np.uint64(1) & (v ^ (v > half).astype(np.uint64))
    if t > q0:
        v[v > half] += np.uint64(t - q0)
        return v
    v[v > half] += np.uint64(t - q0 % t)
    big = v >= np.uint64(t)
    v[big] %= np.uint64(t)
    return v


# ---- the chain --------------------------------------------------------------------------------------------
def chain(x, q, t, to_plaintext, steps=None):
    """x [B][L][N] in coefficient form over q[:L] -> [B][N]: ModReduce for j = L - 1 down to 1
    (bgvrns-pke.cpp:55-60), then x_0 or Mod(t) of it.  steps, a list, receives (j, delta's tower before the
    step, the towers after it)."""
    x = np.ascontiguousarray(x, dtype=np.uint64)
    L = x.shape[1]
    nti, qli = neg_t_inv_modq(q[:L], t), ql_inv_modq(q[:L])
    for j in range(L - 1, 0, -1):
        before = x
        x = K.mod_reduce(x, q[:j + 1], [0] * (j + 1), False, t, nti[j], qli[j])
        if steps is not None:
            steps.append((j, before, x))
    x0 = x[:, 0]
    return mod_t(x0, int(q[0]), t) if to_plaintext else x0.copy()


# ---- DecryptCore and the two branches ---------------------------------------------------------------------
def decrypt_core(elems, s_eval, q):
    """b = c0 + c1 s (+ c2 s^2) over q (len(q) towers of the elements and the first len(q) of s), evaluation
    form (rns-pke.cpp:199-224)"""
    L = len(q)
    B = elems[0].shape[0]
    s = np.ascontiguousarray(np.broadcast_to(s_eval[:L], (B,) + s_eval[:L].shape))
    b = O.eltwise("add", np.ascontiguousarray(elems[0]), O.eltwise("mul", s, np.ascontiguousarray(elems[1]), q), q)
    if len(elems) == 3:
        s2 = O.eltwise("mul", s, s, q)
        b = O.eltwise("add", b, O.eltwise("mul", s2, np.ascontiguousarray(elems[2]), q), q)
    return b


def decrypt_core_call(elems, s_eval, q, rq, eval_form, coeff_out):
    """ofhe_hip_decrypt_core: coefficient-form elements are transformed first; coeff_out adds the INTT"""
    if not eval_form:
        elems = [K.set_format(c, q, rq, True) for c in elems]
    b = decrypt_core(elems, s_eval, q)
    return K.set_format(b, q, rq, False) if coeff_out else b


def decrypt(elems, s_eval, q, rq, t, eval_form, tower0=None):
    """PKEBGVRNS::Decrypt of elements [B][L][N] over q[:L]; s_eval [>= L][N].  tower0, a list, receives the
    tower-0 words the final Mod(t) is applied to."""
    L = elems[0].shape[1]
    ql, rql = list(q[:L]), list(rq[:L])
    if eval_form:  # :52-60
        b = K.set_format(decrypt_core(elems, s_eval, ql), ql, rql, False)
        w = chain(b, ql, t, False)
    else:  # :72-93
        red = [chain(c, ql, t, False)[:, None] for c in elems]
        red = [K.set_format(c, ql[:1], rql[:1], True) for c in red]
        w = K.set_format(decrypt_core(red, s_eval, ql[:1]), ql[:1], rql[:1], False)[:, 0]
    if tower0 is not None:
        tower0.append(w)
    return mod_t(w, int(q[0]), t)


# ---- scalingFactorInt -------------------------------------------------------------------------------------
def scaling_factor(sf, factors, size_ql, t):
    """bgvrns-pke.cpp:62-69: for i < size_ql - 1, sf = sf * ModInverse(factors[size_ql - 1 - i], t) mod t"""
    for i in range(size_ql - 1):
        sf = sf * pow(int(factors[size_ql - 1 - i]), -1, t) % t
    return sf


# ---- moduli and inputs ------------------------------------------------------------------------------------
def mixed_chain(towers, bits=(45, 60, 22, 59, 33, 60, 28, 51), m=2):
    """`towers` distinct primes = 1 mod m whose sizes cycle through `bits`, so that going down the chain
    SwitchModulus meets both q_i > q_j and q_i <= q_j (and, from 60 to 22 bits, q_j > 2 q_i)"""
    out, last = [], {}
    for k in range(towers):
        b = bits[k % len(bits)]
        # going down from 2^b: b-bit primes, the 60-bit ones below the library's bound of 2^60
        last[b] = O.previous_prime(last[b] if b in last else O.first_prime(b, m), m)
        out.append(last[b])
    assert len(set(out)) == towers
    return out


def planted(batch, q, n, seed):
    """[batch][L][n]: seeded uniform words, with 0, q - 1, q >> 1 and (q >> 1) + 1 planted on every tower: all
    four at once in the first coefficients of entry 0, and each mixed with the others along the chain"""
    L = len(q)
    x = O.uniform_dcrt(batch, L, n, q, seed)
    edge = lambda m, k: [0, m - 1, m >> 1, (m >> 1) + 1][k % 4]  # noqa: E731
    for c in range(min(n, 8)):
        for i, m in enumerate(q):
            # c < 4: the same edge on every tower; then edges rotating along the chain
            x[0, i, c] = edge(int(m), c if c < 4 else c + i)
    if n >= 16:
        rng = np.random.default_rng(seed)
        for i, m in enumerate(q):
            x[batch - 1, i, n - 8:] = [edge(int(m), int(k)) for k in rng.integers(0, 4, size=8)]
    return x


# ---- a BGV encryption -------------------------------------------------------------------------------------
def noise_bound(n, t, q):
    """The largest E such that m + t e with 0 <= m < t, |e| <= E certainly decrypts in both branches over the
    towers q (see tests/test_bgv_decrypt_oracle.py::test_real_encryptions_decrypt_in_both_branches)"""
    P = 1
    c = Fraction(0)
    for j in range(1, len(q)):
        c += Fraction(1, 2 * P)  # |delta_j| / q_j < 1/2, divided by q_1 .. q_{j-1}
        P *= int(q[j])
    room = Fraction(int(q[0]), 2) - t * c * (1 + n + n * n)
    return int(room * P / t) - 1


def negacyclic(a, b):
    n = len(a)
    res = np.zeros(n, dtype=object)
    for i in range(n):
        if b[i]:
            res = res + b[i] * np.concatenate((-a[n - i:], a[:n - i]))
    return res


def uniform_mod(rng, n, Q):
    """object array [n] of integers uniform mod Q up to a bias below 2^-60"""
    words = Q.bit_length() // 62 + 2
    return np.array([sum(int(rng.integers(0, 1 << 62)) << (62 * k) for k in range(words)) % Q for _ in range(n)],
                    dtype=object)


def encrypt(rng, v, s, q, rq, elements):
    """elements (2 or 3) polynomials [1][L][n], evaluation form over q, with c0 + c1 s (+ c2 s^2) = v, the
    caller's m + t e (object array [n]); s ternary (object array): c1, c2 uniform mod Q, c0 = v - c1 s - c2 s^2"""
    n = len(v)
    Q = 1
    for x in q:
        Q *= int(x)
    cs = [uniform_mod(rng, n, Q) for _ in range(elements - 1)]
    sp = s
    c0 = v
    for c in cs:
        c0 = c0 - negacyclic(c, sp)
        sp = negacyclic(sp, s)
    res = lambda p: np.stack([(p % int(x)).astype(np.uint64) for x in q])[None]  # noqa: E731
    return [K.set_format(res(p % Q), q, rq, True) for p in [c0] + cs]
