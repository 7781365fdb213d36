"""CPU reference of the BFV (HPS family) multiplication's RNS steps, restated
per coefficient from the reference with exact Python integers (numpy object
arrays) and IEEE doubles (Python floats / numpy float64: one rounding per
multiply, one per add, correctly rounded int -> double conversion):

* ``switch_crt_basis``      DCRTPolyImpl::SwitchCRTBasis            dcrtpoly-impl.h:1178-1230
* ``expand_crt_basis``      DCRTPolyImpl::ExpandCRTBasis            dcrtpoly-impl.h:1311-1358
* ``fast_expand_p_over_q``  DCRTPolyImpl::FastExpandCRTBasisPloverQ dcrtpoly-impl.h:1413-1466
* ``scale_and_round``       DCRTPolyImpl::ScaleAndRound             dcrtpoly-impl.h:1876-1955
* ``eval_mult``             LeveledSHEBFVRNS::EvalMult, HPS / HPSPOVERQ  bfvrns-leveledshe.cpp:168-408

The oracle is used only for NTT / INTT, the element-wise products and the
approximate conversion.  ``nu_switch_fused`` is NOT the reference: it is what a
fused multiply-add chain would compute (each a*b+c exact, rounded once), kept
for the sensitivity check of the tests.

Polynomials are uint64 arrays [batch][towers][n].
"""
import json
import os
from fractions import Fraction

import numpy as np

import bfv_tables as BT


def obj(a):
    return np.asarray(a, dtype=np.uint64).astype(object)


def u64(a):
    return np.ascontiguousarray(np.asarray(a, dtype=object).astype(np.uint64))


# ---- SwitchCRTBasis ---------------------------------------------------------------
def switch_ys(x, q):
    """y_i = [x_i (Q/q_i)^-1]_{q_i} (ModMulFastConst, 1200): canonical, list of object arrays [batch][n]"""
    hinv = BT.hat_inv(q)
    return [obj(x[:, i, :]) * hinv[i] % int(q[i]) for i in range(len(q))]


def nu_switch(ys, q):
    """nu = 0.5; nu += double(y_i) * qInv[i] in tower order (1195-1205), separately rounded"""
    qinv = BT.inv_doubles(q)
    nu = np.full(ys[0].shape, 0.5, dtype=np.float64)
    for y, qi in zip(ys, qinv):
        prod = y.astype(np.float64) * np.float64(qi)
        nu = nu + prod
    return nu


def nu_switch_scalar(ys, q):
    """the same with Python floats, one coefficient (ys: list of ints)"""
    nu = 0.5
    for y, qi in zip(ys, BT.inv_doubles(q)):
        nu = nu + (float(y) * qi)
    return nu


def nu_switch_fused(ys, q):
    """NOT the reference: nu = fma(double(y_i), qInv[i], nu), i.e. every multiply-add exact
    (Fraction) and rounded once -- what a contracted a*b+c chain gives.  One coefficient."""
    nu = 0.5
    for y, qi in zip(ys, BT.inv_doubles(q)):
        nu = float(Fraction(nu) + Fraction(float(y)) * Fraction(qi))
    return nu


def switch_crt_basis(x, q, p, want_alpha=False):
    """x [batch][len(q)][n] -> [batch][len(p)][n] (1178-1230)"""
    x = np.asarray(x, dtype=np.uint64)
    ys = switch_ys(x, q)
    alpha = nu_switch(ys, q).astype(np.int64)  # static_cast<usint>(nu), 1209
    hm, aq = BT.hat_mod(q, p), BT.alpha_mod(q, p)
    out = np.empty((x.shape[0], len(p), x.shape[2]), dtype=np.uint64)
    for j, pj in enumerate(p):
        cur = sum(ys[i] * hm[i][j] for i in range(len(q))) % int(pj)  # Mul128 sums, Barrett (1218-1223)
        sub = np.array([aq[a][j] for a in range(len(q) + 1)], dtype=object)[alpha]
        out[:, j, :] = u64((cur - sub) % int(pj))  # ModSubFast (1226)
    return (out, alpha) if want_alpha else out


# ---- ScaleAndRound -------------------------------------------------------------------
def nu_scale(xin, frac):
    """nu = 0.5; nu += frac[i] * double(x_i) in tower order (1905-1910); xin uint64 [batch][size_i][n]"""
    nu = np.full((xin.shape[0], xin.shape[2]), 0.5, dtype=np.float64)
    for i, f in enumerate(frac):
        prod = np.float64(f) * xin[:, i, :].astype(np.float64)
        nu = nu + prod
    return nu


def scale_and_round(x, q, p, out_is_q, table, frac, want_nu=False):
    """x [batch][len(q) + len(p)][n], Q towers first (1876-1955); both alpha branches are
    floor(nu) mod o_j, taken here with exact integers"""
    x = np.asarray(x, dtype=np.uint64)
    sq, sp = len(q), len(p)
    xin, xown, outs = (x[:, sq:, :], x[:, :sq, :], q) if out_is_q else (x[:, :sq, :], x[:, sq:, :], p)
    si = xin.shape[1]
    nu = nu_scale(xin, frac)
    alpha = np.array([int(v) for v in nu.reshape(-1)], dtype=object).reshape(nu.shape)
    out = np.empty((x.shape[0], len(outs), x.shape[2]), dtype=np.uint64)
    xi = [obj(xin[:, i, :]) for i in range(si)]
    for j, oj in enumerate(outs):
        cur = sum(xi[i] * int(table[j][i]) for i in range(si)) + obj(xown[:, j, :]) * int(table[j][si])
        out[:, j, :] = u64((cur % int(oj) + alpha % int(oj)) % int(oj))
    return (out, nu) if want_nu else out


# ---- ExpandCRTBasis / FastExpandCRTBasisPloverQ ---------------------------------
def expand_crt_basis(O, x, q, r, tb_q, tb_r, eval_form):
    """-> [batch][Q+R][n] evaluation form (1311-1358, resultFormat = EVALUATION)"""
    x = np.asarray(x, dtype=np.uint64)
    coef = O.ntt_inv(x, tb_q) if eval_form else x
    part_r = O.ntt_fwd(switch_crt_basis(coef, q, r), tb_r)
    part_q = x if eval_form else O.ntt_fwd(x, tb_q)
    return np.concatenate([part_q, part_r], axis=1)


def approx_switch_with(O, x, q, p, c, d):
    """ApproxSwitchCRTBasis' loop with the caller's constants c_i (in place of QHatInvModq) and
    d_ij (in place of QHatModp), as FastExpandCRTBasisPloverQ's first loop (1419-1441)"""
    pre = O.base_conv_precompute(q, p)
    pre["qhinv"] = O.U(c)
    pre["qhinv_pre"] = O.U([(int(ci) << 64) // int(qi) for ci, qi in zip(c, q)])
    pre["qhmodp"] = O.U([v for row in d for v in row])
    return np.stack([O.approx_switch_crt_basis(np.ascontiguousarray(xb), q, p, pre) for xb in x])


def fast_expand_p_over_q(O, x, T):
    """x [batch][Q][n] coefficient form -> [batch][Q+R][n] coefficient form (1413-1466): the R part
    by the approximate switch with mNegRlQHatInvModq / qInvModr, the Q part replaced by its exact
    switch back"""
    part_r = approx_switch_with(O, np.asarray(x, dtype=np.uint64), T.q, T.r, T.neg_r_q_hat_inv_modq, T.q_inv_modr)
    part_q = switch_crt_basis(part_r, T.r, T.q)
    return np.concatenate([part_q, part_r], axis=1)


# ---- EvalMult -------------------------------------------------------------------------
class Ring:
    """Oracle NTT tables of the three bases of one parameter set"""

    def __init__(self, O, log_n, q, rq, r, rr):
        self.n = 1 << log_n
        self.tb_q, self.tb_r = O.Tables(self.n, q, rq), O.Tables(self.n, r, rr)
        self.tb_qr = O.Tables(self.n, list(q) + list(r), list(rq) + list(rr))


def eval_mult(O, T, ring, c0, c1, d0, d1):
    """(out0, out1, out2), [batch][Q][n] coefficient form, of two evaluation-form ciphertexts
    (bfvrns-leveledshe.cpp:168-408), technique T.technique"""
    q, r, qr = T.q, T.r, T.q + T.r
    ex = lambda v: expand_crt_basis(O, v, q, r, ring.tb_q, ring.tb_r, True)  # noqa: E731
    e = [ex(c0), ex(c1)]
    if T.technique == BT.HPS:
        e += [ex(d0), ex(d1)]
    else:
        e += [O.ntt_fwd(fast_expand_p_over_q(O, O.ntt_inv(v, ring.tb_q), T), ring.tb_qr) for v in (d0, d1)]
    mul = lambda a, b: O.eltwise("mul", a, b, qr)  # noqa: E731
    prods = [mul(e[0], e[2]), O.eltwise("add", mul(e[0], e[3]), mul(e[1], e[2]), qr), mul(e[1], e[3])]
    outs = []
    for pr in prods:
        sr = scale_and_round(O.ntt_inv(pr, ring.tb_qr), q, r, T.out_is_q, T.sr_table, T.sr_frac)
        outs.append(switch_crt_basis(sr, r, q) if T.technique == BT.HPS else sr)
    return outs


# ---- exact-integer helpers (definitions, encryption) -----------------------------------
def crt_lift(x, ms):
    """[batch][towers][n] residues -> object array [batch][n] of values in [0, M)"""
    M = BT.product(ms)
    acc = 0
    for i, m in enumerate(ms):
        Mi = M // int(m)
        acc = acc + obj(x[:, i, :]) * (Mi * pow(Mi % int(m), -1, int(m)))
    return acc % M


def residues(v, ms):
    """object array [batch][n] of integers -> uint64 [batch][towers][n]"""
    return np.stack([u64(v % int(m)) for m in ms], axis=1)


def negacyclic(a, b):
    """a * b mod X^n + 1 over the integers; object arrays [n]"""
    n = len(a)
    res = np.zeros(n, dtype=object)
    for i in range(n):
        if b[i]:
            res = res + b[i] * np.concatenate((-a[n - i:], a[:n - i]))
    return res


def encrypt(O, rng, m, s, q, tb_q, t):
    """BFV ciphertext (c0, c1), [1][Q][n] evaluation form, of plaintext m (object [n], mod t) under
    the ternary secret s: c0 = Delta m + e - a s, c1 = a, error bound 3"""
    Q = BT.product(q)
    n = len(m)
    a = np.array([int(rng.integers(0, 1 << 62)) * (1 << 62) + int(rng.integers(0, 1 << 62)) for _ in range(n)],
                 dtype=object) % Q
    e = np.array([int(v) for v in rng.integers(-3, 4, size=n)], dtype=object)
    c0 = ((Q // t) * m + e - negacyclic(a, s)) % Q
    enc = lambda v: O.ntt_fwd(residues(v.reshape(1, n), q), tb_q)  # noqa: E731
    return enc(c0), enc(a)


def decrypt3(outs, s, q, t):
    """round(t (c0 + c1 s + c2 s^2) / Q) mod t of a 3-element coefficient-form ciphertext, batch entry 0"""
    Q = BT.product(q)
    c = [crt_lift(o, q)[0] for o in outs]
    v = (c[0] + negacyclic(c[1], s) + negacyclic(negacyclic(c[2], s), s)) % Q
    v = np.where(v >= (Q + 1) // 2, v - Q, v)
    return np.array([(2 * t * int(x) + Q) // (2 * Q) % t for x in v], dtype=object)


# ---- shared inputs of the switch tests ------------------------------------------------------
SPECIAL, PLANTED, UNIFORM = 0, 1, 2
BAND = 512  # the dense band of small offsets: v = floor(Q / 2) + delta for every |delta| <= BAND


def fused_differs(v, q, hinv):
    """does a fused multiply-add chain give another alpha than the reference's sum for value v?"""
    ys = [v % int(m) * h % int(m) for m, h in zip(q, hinv)]
    return int(nu_switch_fused(ys, q)) != int(nu_switch_scalar(ys, q))


def switch_inputs(q, n, batch, seed, planted=None):
    """x [batch][len(q)][n] and kinds [batch][n], coefficient k = b n + ri.

    PLANTED coefficients hold v = floor(Q / 2) + delta, |delta| < 2^40, on the rounding boundary of
    alpha, where the order and the rounding of the double sum decide it.  Half of them (at least one)
    come from the dense band |delta| <= BAND, those first on which a fused multiply-add chain gives
    another alpha than the reference's separately rounded sum (fused_differs; with one tower only
    about 60 consecutive small offsets are such, since Q < 2^60 keeps every larger offset 2^-60
    |delta| away from 1/2), then the rest of the band in order; the other half has random delta.
    Coefficient 0 is the first planted one, so even N = 2 carries a sensitive coefficient; then come
    four SPECIAL ones (v = 0, 1, Q - 1, and x_i = q_i - 1 in every tower), the other planted ones,
    and UNIFORM residues per tower.  planted defaults to 1024 when the case has at least 2048
    coefficients, else a quarter of them (at least one)."""
    rng = np.random.default_rng(seed)
    total = n * batch
    Q = BT.product(q)
    hinv = BT.hat_inv(q)
    if planted is None:
        planted = 1024 if total >= 2048 else max(1, total // 4)
    band = [Q // 2 + d for d in range(-BAND, BAND + 1)]
    hot = [fused_differs(v, q, hinv) for v in band]
    band = [v for v, h in zip(band, hot) if h] + [v for v, h in zip(band, hot) if not h]
    values = band[:max(1, planted // 2)]
    values += [Q // 2 + int(rng.integers(-(1 << 40) + 1, 1 << 40)) for _ in range(planted - len(values))]
    special = [[0] * len(q), [1 % int(m) for m in q], [(Q - 1) % int(m) for m in q], [int(m) - 1 for m in q]]
    cols, kinds = [], []
    for k in range(total):
        if k == 0 or 5 <= k < 4 + planted:
            v = values[0 if k == 0 else k - 4]
            cols.append([v % int(m) for m in q])
            kinds.append(PLANTED)
        elif k < 5:
            cols.append(special[k - 1])
            kinds.append(SPECIAL)
        else:
            cols.append([int(rng.integers(0, int(m))) for m in q])
            kinds.append(UNIFORM)
    x = np.array(cols, dtype=np.uint64).reshape(batch, n, len(q)).transpose(0, 2, 1)
    return np.ascontiguousarray(x), np.array(kinds).reshape(batch, n)


# The generated exact-switch cases (log_n, size_q, size_p) of the GPU parity test; tests/test_bfv_oracle.py
# asserts on these very inputs that each case can tell a fused sum from the reference's.  All have
# 60-bit towers; (8, 5, 6) is a generic_moduli chain of mixed 22-60-bit towers.  (3, 2, 2) runs on
# the moduli of the reference's known answer in its direction, R -> Q (sources the fixture's r,
# targets its q).  The fixture's own 8 vectors (test_switch_known_answer) hold no sensitive
# coefficient; the planted ones of this generated case do.  In the other direction, with the
# fixture's q as sources, no sensitive input exists at all: both qInv doubles round up, and on
# 13,000 sampled values v = floor(Q / 2) + delta neither sum falls below the integer.
SWITCH_CASES = [(1, 1, 1), (3, 2, 2), (5, 3, 4), (12, 16, 17), (12, 17, 3), (10, 65, 2), (8, 5, 6)]
SWITCH_BATCH = 3
MIXED_BITS = [60, 22, 45, 31, 58, 50, 27, 60, 40, 36, 54]  # 5 sources + 6 targets
_switch_cases = {}


def switch_case(O, log_n, sq, sp):
    """(q, p, x [SWITCH_BATCH][sq][n], kinds) of one SWITCH_CASES entry, built once"""
    key = (log_n, sq, sp)
    if key not in _switch_cases:
        if key == (3, 2, 2):
            with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                                   "reference_fixtures.json")) as f:
                k = json.load(f)["kat_fast_expand_crt_basis"]
            m = k["r"] + k["q"]
        elif key == (8, 5, 6):
            from test_mixed_moduli_oracle import mixed_chain

            m, _ = mixed_chain(log_n, MIXED_BITS, generic=True)
        else:
            m, _ = O.moduli_chain(log_n, sq + sp)
        q, p = m[:sq], m[sq:]
        _switch_cases[key] = (q, p) + switch_inputs(q, 1 << log_n, SWITCH_BATCH, 1000 + 31 * sq + sp)
    return _switch_cases[key]


def two_branch_case(O, log_n, seed, out_is_q=False):
    """ScaleAndRound on both sides of nu = 2^64 (dcrtpoly-impl.h:1911 / 1933): 17 summed towers of 60
    bits (and 17 outputs), frac[i] = 1 - 2^-53, a random integer table; the summed towers hold
    q_i - 1 on the even coefficients (nu ~ 17 * 2^60 > 2^64) and values below q_i / 2 on the odd ones
    (nu < 8.5 * 2^60).  -> (q, p, table, frac, x [1][34][n])"""
    rng = np.random.default_rng(seed)
    n = 1 << log_n
    m, _ = O.moduli_chain(log_n, 34)
    q, p = m[:17], m[17:]
    outs = q if out_is_q else p
    frac = [1.0 - 2.0 ** -53] * 17
    table = [[int(rng.integers(0, int(o))) for _ in range(18)] for o in outs]
    even = np.arange(n) % 2 == 0
    x = np.empty((1, 34, n), dtype=np.uint64)
    for k, mod in enumerate(m):
        if (k >= 17) == bool(out_is_q):  # a summed tower
            x[0, k] = np.where(even, np.uint64(mod - 1), rng.integers(0, mod // 2, size=n, dtype=np.uint64))
        else:
            x[0, k] = rng.integers(0, mod, size=n, dtype=np.uint64)
    return q, p, table, frac, x

