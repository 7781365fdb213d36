"""CPU reference of BFV multiplication and relinearisation by HPSPOVERQLEVELED with dropped
levels, composed from tests/bfv_ref.py's restated steps (exact Python integers, IEEE doubles) and
the tables of bfv_tables.LeveledTables.  l is the index of the last kept tower.

* ``drop``                  DCRTPolyImpl::ScaleAndRound Q -> Q_l      dcrtpoly-impl.h:1876-1955
* ``expand_ql_hat``         DCRTPolyImpl::ExpandCRTBasisQlHat         dcrtpoly-impl.h:1514-1534
* ``fast_expand_leveled``   DCRTPolyImpl::FastExpandCRTBasisPloverQ   dcrtpoly-impl.h:1413-1466
* ``eval_mult``             LeveledSHEBFVRNS::EvalMult                bfvrns-leveledshe.cpp:235-274, 316-330, 367-382
* ``relinearize``           LeveledSHEBFVRNS::RelinearizeCore         bfvrns-leveledshe.cpp:845-899

Polynomials are uint64 arrays [batch][towers][n].  The ``*_coef`` functions work in the
coefficient domain only (negacyclic products with exact integers, no NTT, no oracle): the CPU tests
decrypt through them at every level.
"""
from fractions import Fraction

import numpy as np

import bfv_ref as R
import bfv_tables as BT


# ---- the steps ------------------------------------------------------------------------------
def drop(x, T, want_nu=False):
    """x [batch][size_q][n] coefficient form over Q -> [batch][l + 1][n] over Q_l"""
    x = np.asarray(x, dtype=np.uint64)
    if not T.dropped:
        return (x.copy(), None) if want_nu else x.copy()
    return R.scale_and_round(x, T.ql, T.q[T.l + 1:], True, T.drop_table, T.drop_frac, want_nu=want_nu)


def expand_ql_hat(x, T, addend=None):
    """x [batch][l + 1][n] -> [batch][size_q][n]: tower i <= l times (Q / Q_l) mod q_i (plus the
    addend's tower), towers past l zero (or the addend's)"""
    x = np.asarray(x, dtype=np.uint64)
    out = np.zeros((x.shape[0], len(T.q), x.shape[2]), dtype=np.uint64)
    if addend is not None:
        out[:] = np.asarray(addend, dtype=np.uint64)
    for i, qi in enumerate(T.ql):
        v = R.obj(x[:, i, :]) * T.ql_hat_modq[i] % qi
        if addend is not None:
            v = (v + R.obj(out[:, i, :])) % qi
        out[:, i, :] = R.u64(v)
    return out


def scale_round_product(x, T, want_nu=False):
    """x [batch][2 (l + 1)][n] over Q_l R_l, coefficient form -> [batch][l + 1][n] over Q_l"""
    return R.scale_and_round(x, T.ql, T.rl, True, T.sr_table, T.sr_frac, want_nu=want_nu)


def scale_round_lift(x, T):
    """ScaleAndRound to Q_l, then ExpandCRTBasisQlHat: [batch][2 (l + 1)][n] -> [batch][size_q][n]"""
    return expand_ql_hat(scale_round_product(x, T), T)


def approx_switch_exact_ints(x, q, p, c, d):
    """ApproxSwitchCRTBasis' loop with constants c_i, d_ij and exact integers (the sum is reduced
    once, as BarrettUint128ModUint64 does): [batch][len(q)][n] -> [batch][len(p)][n]"""
    ys = [R.obj(x[:, i, :]) * int(c[i]) % int(q[i]) for i in range(len(q))]
    return np.stack([R.u64(sum(ys[i] * int(d[i][j]) for i in range(len(q))) % int(pj))
                     for j, pj in enumerate(p)], axis=1)


def fast_expand_leveled(x, T):
    """x [batch][size_q][n] coefficient form over the FULL Q -> [batch][2 (l + 1)][n] coefficient form
    over Q_l R_l: the R_l part from all size_q towers with mNegRlQHatInvModq(l) / qInvModr, the Q_l
    part by the exact switch back"""
    part_r = approx_switch_exact_ints(np.asarray(x, dtype=np.uint64), T.q, T.rl, T.neg_rl_q_hat_inv_modq,
                                      T.q_inv_modr)
    part_q = R.switch_crt_basis(part_r, T.rl, T.ql)
    return np.concatenate([part_q, part_r], axis=1)


def expand_leveled(x, T):
    """ciphertext 1: x [batch][size_q][n] coefficient form -> [batch][2 (l + 1)][n] coefficient form
    (the drop, then the exact switch Q_l -> R_l next to the Q_l towers)"""
    xl = drop(x, T)
    return np.concatenate([xl, R.switch_crt_basis(xl, T.ql, T.rl)], axis=1)


# ---- with the oracle's transforms: what the device computes ----------------------------------
class LevelRing:
    """Oracle NTT tables of one level's bases"""

    def __init__(self, O, log_n, q, rq, r, rr, l):
        self.n = 1 << log_n
        L = l + 1
        self.tb_q = O.Tables(self.n, q, rq)
        self.tb_ql, self.tb_rl = O.Tables(self.n, q[:L], rq[:L]), O.Tables(self.n, r[:L], rr[:L])
        self.tb_qlrl = O.Tables(self.n, list(q[:L]) + list(r[:L]), list(rq[:L]) + list(rr[:L]))


def eval_mult(O, T, ring, c0, c1, d0, d1):
    """(out0, out1, out2), [batch][size_q][n] coefficient form, of two evaluation-form ciphertexts"""
    qr = T.ql + T.rl
    e = [O.ntt_fwd(expand_leveled(O.ntt_inv(v, ring.tb_q), T), ring.tb_qlrl) for v in (c0, c1)]
    e += [O.ntt_fwd(fast_expand_leveled(O.ntt_inv(v, ring.tb_q), T), ring.tb_qlrl) for v in (d0, d1)]
    mul = lambda a, b: O.eltwise("mul", a, b, qr)  # noqa: E731
    prods = [mul(e[0], e[2]), O.eltwise("add", mul(e[0], e[3]), mul(e[1], e[2]), qr), mul(e[1], e[3])]
    outs = []
    for pr in prods:
        sr = scale_round_product(O.ntt_inv(pr, ring.tb_qlrl), T)
        outs.append(expand_ql_hat(sr, T) if T.dropped else sr)
    return outs


def relinearize(O, K, T, ring, kp, elements, eval_form, key_b, key_a):
    """(out0, out1) [batch][size_q][n] evaluation form; kp: keyswitch.KeySwitchParams over the full Q"""
    last = np.asarray(elements[-1], dtype=np.uint64)
    coef = O.ntt_inv(last, ring.tb_q) if eval_form else last
    dl = O.ntt_fwd(drop(coef, T), ring.tb_ql)
    a0, a1 = K.ks_core(kp, dl, key_b, key_a)
    ev = [np.asarray(c, dtype=np.uint64) if eval_form else O.ntt_fwd(np.asarray(c, dtype=np.uint64), ring.tb_q)
          for c in elements[:2]]
    return expand_ql_hat(a0, T, ev[0]), expand_ql_hat(a1, T, ev[1] if len(elements) == 3 else None)


# ---- coefficient domain only, exact integers ---------------------------------------------------
def _negacyclic_towers(a, b, ms):
    """[1][towers][n] x [1][towers][n] -> [1][towers][n], the negacyclic product per tower"""
    return np.stack([R.u64(R.negacyclic(R.obj(a[0, i]), R.obj(b[0, i])) % int(m)) for i, m in enumerate(ms)])[None]


def _add_towers(a, b, ms):
    return np.stack([R.u64((R.obj(a[0, i]) + R.obj(b[0, i])) % int(m)) for i, m in enumerate(ms)])[None]


def uniform_mod(rng, M, n):
    """n uniform integers below M (object array), from 62-bit draws"""
    words = M.bit_length() // 62 + 2
    return np.array([sum(int(rng.integers(0, 1 << 62)) << (62 * k) for k in range(words)) % M for _ in range(n)],
                    dtype=object)


def encrypt_coef(rng, m, s, q, t, a=None):
    """BFV ciphertext (c0, c1), [1][Q][n] COEFFICIENT form, of plaintext m (object [n], mod t) under
    the ternary secret s: c0 = floor(Q / t) m + e - a s, c1 = a, errors <= 3"""
    Q = BT.product(q)
    n = len(m)
    if a is None:
        a = uniform_mod(rng, Q, n)
    e = np.array([int(v) for v in rng.integers(-3, 4, size=n)], dtype=object)
    c0 = ((Q // t) * m + e - R.negacyclic(a, s)) % Q
    return R.residues(c0.reshape(1, n), q), R.residues(a.reshape(1, n), q)


def eval_mult_coef(T, c0, c1, d0, d1):
    """the levelled EvalMult on coefficient-form inputs [1][size_q][n], coefficient-form outputs"""
    qr = T.ql + T.rl
    e = [expand_leveled(v, T) for v in (c0, c1)] + [fast_expand_leveled(v, T) for v in (d0, d1)]
    mul = lambda a, b: _negacyclic_towers(a, b, qr)  # noqa: E731
    prods = [mul(e[0], e[2]), _add_towers(mul(e[0], e[3]), mul(e[1], e[2]), qr), mul(e[1], e[3])]
    return [scale_round_lift(pr, T) for pr in prods]


def relin_key_coef(rng, s, q, p, alpha):
    """a HYBRID relinearisation key for s^2 -> s in the coefficient domain with exact integers:
    digit j covers towers [alpha j, alpha (j + 1)) of q; (b_j, a_j) are integer polynomials mod Q P
    with b_j = -a_j s + e_j + P (Q / D_j) [(Q / D_j)^-1]_{D_j} s^2"""
    Q, P = BT.product(q), BT.product(p)
    n = len(s)
    s2 = R.negacyclic(s, s)
    keys = []
    for st in range(0, len(q), alpha):
        D = BT.product(q[st:st + alpha])
        a = uniform_mod(rng, Q * P, n)
        e = np.array([int(v) for v in rng.integers(-3, 4, size=n)], dtype=object)
        g = P * (Q // D) * pow(Q // D % D, -1, D)
        keys.append(((-R.negacyclic(a, s) + e + g * s2) % (Q * P), a))
    return keys


def key_switch_coef(c, q, p, alpha, size_ql, keys):
    """HYBRID KeySwitchCore at size_ql towers with exact integers: c object [n] mod Q_l -> (a0, a1)
    mod Q_l with a0 + a1 s = c s^2 + small.  The digits are the exact residues (not the approximate
    switch's), the division by P is rounded: a semantic stand-in for the device's key switch, used
    only to decrypt the restated relinearisation on the CPU without transforms."""
    ql = q[:size_ql]
    Ql, P = BT.product(ql), BT.product(p)
    acc0 = acc1 = 0
    for j, st in enumerate(range(0, size_ql, alpha)):
        # the level's digit is c mod D with D the digit's towers still in Q_l: the full chain's
        # gadget P (Q / D_j) [(Q / D_j)^-1]_{D_j} is P on those towers and 0 on Q_l's other towers
        D = BT.product(ql[st:st + alpha])
        dj = np.array([int(v) % D for v in c], dtype=object)
        b, a = keys[j]
        acc0 = acc0 + R.negacyclic(b % (Ql * P), dj)
        acc1 = acc1 + R.negacyclic(a % (Ql * P), dj)
    rnd = lambda v: np.array([(2 * (int(x) % (Ql * P)) + P) // (2 * P) % Ql for x in v], dtype=object)  # noqa: E731
    return rnd(acc0), rnd(acc1)


def decrypt2(c0, c1, s, q, t):
    """round(t (c0 + c1 s) / Q) mod t of a 2-element ciphertext (object arrays [n] mod Q)"""
    Q = BT.product(q)
    v = (c0 + R.negacyclic(c1, s)) % Q
    v = np.where(v >= (Q + 1) // 2, v - Q, v)
    return np.array([(2 * t * int(x) + Q) // (2 * Q) % t for x in v], dtype=object)


# ---- the definition of the drop and its bound ------------------------------------------------
def drop_exact(x, T):
    """round(x Q_l / Q) mod Q_l per coefficient, from the CRT value: object array [batch][n]"""
    v = R.crt_lift(np.asarray(x, dtype=np.uint64), T.q)
    return np.array([int((2 * int(a) * T.Ql + T.Q) // (2 * T.Q)) % T.Ql for a in v.reshape(-1)],
                    dtype=object).reshape(v.shape)


def drop_bound(T):
    """|restated drop - round(x Q_l / Q)| <= 1 + (k + k^2) max q 2^-53 with k dropped towers: the k
    products frac_i double(x_i) are each off by less than q_i 2^-53 (frac's own error times x_i and
    the product's rounding), the k additions by less than k max q 2^-53 in all"""
    k = T.dropped
    return 1 + Fraction((k + k * k) * max(T.q), 1 << 53)


# ---- sensitivity: would a fused multiply-add chain give another floor(nu)? ---------------------
def nu_scale_scalar(xs, frac):
    nu = 0.5
    for f, x in zip(frac, xs):
        nu = nu + (f * float(int(x)))
    return nu


def nu_scale_fused(xs, frac):
    """NOT the reference: nu = fma(frac[i], double(x_i), nu), every multiply-add exact and rounded once"""
    nu = 0.5
    for f, x in zip(frac, xs):
        nu = float(Fraction(nu) + Fraction(f) * Fraction(float(int(x))))
    return nu


def plant_scale_inputs(x, summed, frac, in0, seed, tries=4000):
    """Overwrite coefficient 0 (and as many following ones as are found, at most 8) of batch entry 0
    of x [batch][towers][n] so that the separately rounded nu and a fused chain's nu have different
    floors: random summed towers, the last of them searched so that nu lands next to an integer.
    Returns the number planted (0 when the search finds none)."""
    rng = np.random.default_rng(seed)
    n = x.shape[2]
    planted = 0
    differs = lambda c: int(nu_scale_scalar(c, frac)) != int(nu_scale_fused(c, frac))  # noqa: E731
    for _ in range(tries):
        if planted >= min(8, n):
            break
        xs = [int(rng.integers(0, m)) for m in summed]
        cands = [xs]
        if frac[-1] > 0:
            # small towers: move the last one so that nu lands next to an integer
            head = nu_scale_scalar(xs[:-1], frac[:-1])
            near = int((np.ceil(head) + int(rng.integers(0, 3)) - head) / frac[-1])
            cands += [xs[:-1] + [min(max(near + d, 0), summed[-1] - 1)] for d in range(-3, 4)]
        for cand in cands:
            if differs(cand):
                for i, v in enumerate(cand):
                    x[0, in0 + i, planted] = v
                planted += 1
                break
    return planted
