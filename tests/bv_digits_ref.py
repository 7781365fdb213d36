"""BV key switching with a digit size r > 0, restated in Python from the
reference's contract (DCRTPolyImpl::CRTDecompose(r), dcrtpoly-impl.h:266-320;
PolyImpl::BaseDecompose / PowersOfBase, poly-impl.h:516-563; KeySwitchBV,
keyswitch-bv.cpp:88-103, 283-338) with oracle/keyswitch.py's set_format and
switch_modulus and oracle.eltwise.  "Parity unpinned": no reference-run data
exists for this path; tests/test_bv_digits_oracle.py pins it by identities.

Digit numbering: tower i has w_i = ceil(bitlen(q_i) / r) windows, digit
arrWindows[i] + j (arrWindows[i] = w_0 + ... + w_{i-1}) is window j of tower i.
r = 0 is digitSize = 0: one digit per tower (keyswitch.crt_decompose0)."""
import numpy as np

import keyswitch as K
import oracle as O


def windows(q, r):
    """w_i per tower: ceil(GetLengthForBase(2) / r); one at r = 0."""
    return [-(-int(m).bit_length() // r) if r else 1 for m in q]


def digit_count(q, r):
    """nWindows."""
    return sum(windows(q, r))


def digit_index(q, r):
    """[(source tower i, window j)] in digit order."""
    return [(i, j) for i, w in enumerate(windows(q, r)) for j in range(w)]


def window(coef, j, r):
    """GetDigitAtIndexForBase(j + 1, 1 << r) of every coefficient."""
    return (coef >> np.uint64(j * r)) & np.uint64((1 << r) - 1)


def crt_decompose(c, q, rq, r):
    """c [B][T][N] in evaluation form -> digits [B][nWindows][T][N] in evaluation form."""
    if r == 0:
        return K.crt_decompose0(c, q, rq)
    B, T, n = c.shape
    coef = K.set_format(c, q, rq, False)
    idx = digit_index(q, r)
    out = np.empty((B, len(idx), T, n), np.uint64)
    for d, (i, j) in enumerate(idx):
        win = window(coef[:, i], j, r)
        dig = np.empty((B, T, n), np.uint64)
        for k in range(T):
            dig[:, k] = win if k == i else K.switch_modulus(win, int(q[i]), int(q[k]))
        out[:, d] = K.set_format(dig, q, rq, True)
    return out


def bv_fast_core_digits(digits, kb, ka, q):
    """EvalFastKeySwitchCore, term by term: digits [B][D][T][N], keys [>= D][>= T][N]."""
    B, D, T, n = digits.shape
    out0 = np.empty((B, T, n), np.uint64)
    out1 = np.empty_like(out0)
    for b in range(B):
        ct0 = O.eltwise("mul", kb[0:1, :T], digits[b, 0:1], q)
        ct1 = O.eltwise("mul", ka[0:1, :T], digits[b, 0:1], q)
        for d in range(1, D):
            ct0 = O.eltwise("add", ct0, O.eltwise("mul", kb[d:d + 1, :T], digits[b, d:d + 1], q), q)
            ct1 = O.eltwise("add", ct1, O.eltwise("mul", ka[d:d + 1, :T], digits[b, d:d + 1], q), q)
        out0[b], out1[b] = ct0[0], ct1[0]
    return out0, out1


def bv_keygen_digits(q, rq, s_old, s_new, r, rng, err_bound=3):
    """KeySwitchGenInternal with PowersOfBase: filtered_{i,j} = s_old_i 2^{j r} mod q_i in tower i, zero
    elsewhere; bv = filtered - (a s_new + e).  s_old, s_new [T][N] in evaluation form.  Returns (kb, ka, es,
    e_coef): keys and errors [D][T][N] in evaluation form, and the errors' signed coefficients [D][N]."""
    if r == 0:
        raise ValueError("digitSize = 0 keys come from keyswitch.bv_keygen")
    T, n = len(q), s_old.shape[1]
    idx = digit_index(q, r)
    kb = np.empty((len(idx), T, n), np.uint64)
    ka = np.empty_like(kb)
    es = np.empty_like(kb)
    ec = np.empty((len(idx), n), np.int64)
    for d, (i, j) in enumerate(idx):
        a = np.stack([rng.integers(0, int(m), size=n, dtype=np.uint64) for m in q])
        ec[d] = rng.integers(-err_bound, err_bound + 1, size=n)
        e = K.small_poly_eval(ec[d], q, rq)[0]
        filt = np.zeros((T, n), np.uint64)
        filt[i] = O.mul_scalar(s_old[i][None, None], [pow(2, j * r, int(q[i]))], [q[i]])[0, 0]
        ase = O.eltwise("add", O.eltwise("mul", a[None], s_new[None], q), e[None], q)
        kb[d] = O.eltwise("sub", filt[None], ase, q)[0]
        ka[d], es[d] = a, e
    return kb, ka, es, ec


def key_switch_in_place(cv, kb, ka, q, rq, r):
    """KeySwitchInPlace on a list of two or three [B][T][N] elements: c0 += ct0; c1 = ct1 (two) or c1 += ct1."""
    digits = crt_decompose(cv[-1], q, rq, r)
    ct0, ct1 = bv_fast_core_digits(digits, kb, ka, q)
    c0 = O.eltwise("add", np.ascontiguousarray(cv[0]), ct0, q)
    c1 = ct1 if len(cv) == 2 else O.eltwise("add", np.ascontiguousarray(cv[1]), ct1, q)
    return c0, c1
