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

``fast=True`` (switch_crt_basis, scale_and_round and their callers) computes the same residues with
64-bit words in numpy instead of Python integers, for the shapes of 2^16 and 2^17 coefficients whose
object arrays take seconds: every product c x mod m is Shoup's (floor(x floor(c 2^64 / m) / 2^64) as
the quotient, one correction), sums are taken mod m term by term.  The double sums are the same code.
tests/test_bfv_oracle.py checks the two paths against each other.
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


# ---- 64-bit words (fast = True) -----------------------------------------------------
_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def _mulhi(a, b):
    """floor(a b / 2^64) for a uint64 array a and an integer 0 <= b < 2^64, from 32-bit halves"""
    b0, b1 = np.uint64(b & 0xFFFFFFFF), np.uint64(b >> 32)
    a0, a1 = a & _M32, a >> _S32
    p01, p10 = a0 * b1, a1 * b0
    mid = ((a0 * b0) >> _S32) + (p01 & _M32) + (p10 & _M32)
    return a1 * b1 + (p01 >> _S32) + (p10 >> _S32) + (mid >> _S32)


def mulmod_const(a, c, m):
    """a c mod m, canonical, for a uint64 array a (any words), integers 0 <= c < m < 2^63"""
    c, m = int(c) % int(m), int(m)
    r = a * np.uint64(c) - _mulhi(a, (c << 64) // m) * np.uint64(m)  # wraps mod 2^64; in [0, 2 m)
    return np.where(r >= np.uint64(m), r - np.uint64(m), r)


def _addmod(a, b, m):
    s = a + b
    return np.where(s >= np.uint64(m), s - np.uint64(m), s)


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


def _switch_crt_basis_fast(x, q, p):
    hinv = BT.hat_inv(q)
    ys = [mulmod_const(x[:, i, :], hinv[i], q[i]) for i in range(len(q))]
    alpha = nu_switch(ys, q).astype(np.int64)
    hm, aq = BT.hat_mod(q, p), BT.alpha_mod(q, p)
    out = np.empty((x.shape[0], len(p), x.shape[2]), dtype=np.uint64)
    for j, pj in enumerate(p):
        cur = np.zeros(ys[0].shape, dtype=np.uint64)
        for i in range(len(q)):
            cur = _addmod(cur, mulmod_const(ys[i], hm[i][j], pj), pj)
        sub = np.array([aq[a][j] for a in range(len(q) + 1)], dtype=np.uint64)[alpha]
        out[:, j, :] = np.where(cur >= sub, cur - sub, cur + np.uint64(pj) - sub)
    return out


def switch_crt_basis(x, q, p, want_alpha=False, fast=False):
    """x [batch][len(q)][n] -> [batch][len(p)][n] (1178-1230)"""
    x = np.asarray(x, dtype=np.uint64)
    if fast:
        return _switch_crt_basis_fast(x, q, p)
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


def scale_and_round(x, q, p, out_is_q, table, frac, want_nu=False, fast=False):
    """x [batch][len(q) + len(p)][n], Q towers first (1876-1955); both alpha branches are
    floor(nu) mod o_j, taken here with exact integers"""
    x = np.asarray(x, dtype=np.uint64)
    sq, sp = len(q), len(p)
    xin, xown, outs = (x[:, sq:, :], x[:, :sq, :], q) if out_is_q else (x[:, :sq, :], x[:, sq:, :], p)
    si = xin.shape[1]
    nu = nu_scale(xin, frac)
    if fast and nu.max() < 2.0 ** 63:  # floor(nu) fits a word
        floor_nu = nu.astype(np.uint64)
        out = np.empty((x.shape[0], len(outs), x.shape[2]), dtype=np.uint64)
        for j, oj in enumerate(outs):
            cur = mulmod_const(xown[:, j, :], table[j][si], oj)
            for i in range(si):
                cur = _addmod(cur, mulmod_const(xin[:, i, :], table[j][i], oj), oj)
            out[:, j, :] = _addmod(cur, floor_nu % np.uint64(oj), oj)
        return (out, nu) if want_nu else out
    alpha = np.array([int(v) for v in nu.reshape(-1)], dtype=object).reshape(nu.shape)
    out = np.empty((x.shape[0], len(outs), x.shape[2]), dtype=np.uint64)
    xi = [obj(xin[:, i, :]) for i in range(si)]
    for j, oj in enumerate(outs):
        cur = sum(xi[i] * int(table[j][i]) for i in range(si)) + obj(xown[:, j, :]) * int(table[j][si])
        out[:, j, :] = u64((cur % int(oj) + alpha % int(oj)) % int(oj))
    return (out, nu) if want_nu else out


# ---- ExpandCRTBasis / FastExpandCRTBasisPloverQ ---------------------------------
def expand_crt_basis(O, x, q, r, tb_q, tb_r, eval_form, fast=False):
    """-> [batch][Q+R][n] evaluation form (1311-1358, resultFormat = EVALUATION)"""
    x = np.asarray(x, dtype=np.uint64)
    coef = O.ntt_inv(x, tb_q) if eval_form else x
    part_r = O.ntt_fwd(switch_crt_basis(coef, q, r, fast=fast), tb_r)
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


def fast_expand_p_over_q(O, x, T, fast=False):
    """x [batch][Q][n] coefficient form -> [batch][Q+R][n] coefficient form (1413-1466): the R part
    by the approximate switch with mNegRlQHatInvModq / qInvModr, the Q part replaced by its exact
    switch back"""
    part_r = approx_switch_with(O, np.asarray(x, dtype=np.uint64), T.q, T.r, T.neg_r_q_hat_inv_modq, T.q_inv_modr)
    part_q = switch_crt_basis(part_r, T.r, T.q, fast=fast)
    return np.concatenate([part_q, part_r], axis=1)


# ---- EvalMult -------------------------------------------------------------------------
class Ring:
    """Oracle NTT tables of the three bases of one parameter set"""

    def __init__(self, O, log_n, q, rq, r, rr):
        self.n = 1 << log_n
        self.tb_q, self.tb_r = O.Tables(self.n, q, rq), O.Tables(self.n, r, rr)
        self.tb_qr = O.Tables(self.n, list(q) + list(r), list(rq) + list(rr))


def eval_mult(O, T, ring, c0, c1, d0, d1, fast=False):
    """(out0, out1, out2), [batch][Q][n] coefficient form, of two evaluation-form ciphertexts
    (bfvrns-leveledshe.cpp:168-408), technique T.technique"""
    q, r, qr = T.q, T.r, T.q + T.r
    ex = lambda v: expand_crt_basis(O, v, q, r, ring.tb_q, ring.tb_r, True, fast)  # noqa: E731
    e = [ex(c0), ex(c1)]
    if T.technique == BT.HPS:
        e += [ex(d0), ex(d1)]
    else:
        e += [O.ntt_fwd(fast_expand_p_over_q(O, O.ntt_inv(v, ring.tb_q), T, fast), ring.tb_qr) for v in (d0, d1)]
    mul = lambda a, b: O.eltwise("mul", a, b, qr)  # noqa: E731
    prods = [mul(e[0], e[2]), O.eltwise("add", mul(e[0], e[3]), mul(e[1], e[2]), qr), mul(e[1], e[3])]
    outs = []
    for pr in prods:
        sr = scale_and_round(O.ntt_inv(pr, ring.tb_qr), q, r, T.out_is_q, T.sr_table, T.sr_frac, fast=fast)
        outs.append(switch_crt_basis(sr, r, q, fast=fast) if T.technique == BT.HPS else sr)
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


# ---- the matrix-core kernel's K-step counts, target chunks and grid cap -------------------------
# (log_n, size_q, size_p): one case per instantiated K-step count of k_switch_mma that SWITCH_CASES
# leaves out (KS = ceil(size_q / 4), rounded up to even above 8: 3, 6, 7, 8 and the WIDE combine's 10,
# 12, 14, 16), two of them with more targets than one block's LDS image holds (blockIdx.y > 0).
# tests/test_bfv_oracle.py restates the host's K-step / chunk arithmetic and asserts this table.
SWITCH_CASES_MMA = [(5, 12, 3), (5, 24, 5), (5, 28, 2), (6, 32, 29), (5, 40, 3), (5, 48, 2), (5, 56, 2), (6, 64, 13)]
# the cases on a generic_moduli chain of mixed 22-60-bit towers (no special-prime reduction); the
# others have 60-bit towers of the form 2^60 - d
SWITCH_MMA_MIXED = {(5, 24, 5): 6, (5, 48, 2): 12}  # case -> its K-step count
# the grid cap: 1024 blocks of 256 coefficients against a cap of 768, so the group loop's second trip
# is a partial one
SWITCH_CAP_CASE = (16, 2, 3)
SWITCH_CAP_BATCH = 4
EXTREME = 3  # kinds: the three columns of extreme_columns
DIGITS_MAX, DIGITS_MIN = 0x0F7F7F7F7F7F7F7F, 0x0080808080808080


def mma_ks(size_q):
    """K-steps of four source towers (bconv_mma_table)"""
    ks = (size_q + 3) // 4
    return (ks + 1) & ~1 if ks > 8 else ks


def mma_tpc(size_q, size_p, lds_max=64 * 1024, red_bytes=64, src_bytes=32):
    """(tiles, target tiles per chunk): the most tiles whose fragments [tpc][ks][64 lanes][16 B],
    reduction rows [4 tpc] and source rows [4 ks] fit the LDS budget (bconv_mma_lds)"""
    ks, tiles = mma_ks(size_q), (size_p + 3) // 4
    lds = lambda tpc: tpc * (ks * 1024 + 4 * red_bytes) + 4 * ks * src_bytes  # noqa: E731
    tpc = 0
    while tpc < tiles and lds(tpc + 1) <= lds_max:
        tpc += 1
    return tiles, tpc


def mma_spq(p):
    """the host's predicate for the special-prime reduction: every target 2^L - d, 33 <= L <= 60,
    0 < d < 2^32 and (2^(81-L) + 1) d + 2^49 + 2 d < 2^L"""
    for pj in p:
        L = int(pj).bit_length()
        d = (1 << L) - int(pj) if 33 <= L <= 60 else 0
        if not (0 < d < 1 << 32 and ((1 << (81 - L)) + 1) * d + (1 << 49) + 2 * d < 1 << L):
            return False
    return True


def extreme_columns(q):
    """Three columns given by their y_i = [x_i (Q/q_i)^-1]_{q_i}: q_i - 1 in every tower (nu = size_q +
    0.5, alpha = size_q: the last row of alphaQModp), and the values whose signed base-256 digits are
    the largest (127 in every position) and the most negative (-128, -127, ...) a tower allows, the
    bounds of the matrix-core kernel's partial sums.  -> [3][len(q)] residues x_i"""
    Q = BT.product(q)
    ys = [[int(m) - 1 for m in q], [min(int(m) - 1, DIGITS_MAX) for m in q], [DIGITS_MIN % int(m) for m in q]]
    return [[y * (Q // int(m) % int(m)) % int(m) for y, m in zip(row, q)] for row in ys]


def plant_extremes(x, kinds, q):
    """overwrite the last three coefficients of every batch entry (uniform ones) with extreme_columns"""
    n = x.shape[2]
    assert (kinds[:, n - 3:] == UNIFORM).all()
    x[:, :, n - 3:] = np.array(extreme_columns(q), dtype=np.uint64).T
    kinds[:, n - 3:] = EXTREME
    return x, kinds


def switch_case_mma(O, log_n, sq, sp):
    """(q, p, x [SWITCH_BATCH][sq][n], kinds) of one SWITCH_CASES_MMA entry, built once: switch_inputs'
    planted coefficients plus the extreme columns"""
    key = ("mma", log_n, sq, sp)
    if key not in _switch_cases:
        if (log_n, sq, sp) in SWITCH_MMA_MIXED:
            from test_mixed_moduli_oracle import mixed_chain

            m, _ = mixed_chain(log_n, [MIXED_BITS[i % len(MIXED_BITS)] for i in range(sq + sp)], generic=True)
        else:
            m, _ = O.moduli_chain(log_n, sq + sp)
        q, p = m[:sq], m[sq:]
        x, kinds = switch_inputs(q, 1 << log_n, SWITCH_BATCH, 2000 + 31 * sq + sp)
        _switch_cases[key] = (q, p) + plant_extremes(x, kinds, q)
    return _switch_cases[key]


def switch_case_cap(O):
    """(q, p, x [SWITCH_CAP_BATCH][sq][n], kinds) of SWITCH_CAP_CASE: batch entries 0 and 3 (the first
    and the second trip of the matrix-core kernel's group loop) start with 4096 coefficients of
    switch_inputs, the rest is uniform; every entry ends with the extreme columns"""
    log_n, sq, sp = SWITCH_CAP_CASE
    key = ("cap", log_n, sq, sp)
    if key not in _switch_cases:
        n = 1 << log_n
        m, _ = O.moduli_chain(log_n, sq + sp)
        q, p = m[:sq], m[sq:]
        rng = np.random.default_rng(3000)
        x = np.stack([np.stack([rng.integers(0, int(qi), size=n, dtype=np.uint64) for qi in q])
                      for _ in range(SWITCH_CAP_BATCH)])
        kinds = np.full((SWITCH_CAP_BATCH, n), UNIFORM)
        for b in (0, SWITCH_CAP_BATCH - 1):
            xs, ks = switch_inputs(q, 4096, 1, 3001 + b)
            x[b, :, :4096], kinds[b, :4096] = xs[0], ks[0]
        _switch_cases[key] = (q, p) + plant_extremes(x, kinds, q)
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

