"""CPU reference of the BFV (BEHZ) multiplication's RNS steps, restated per
coefficient from the reference's HAVE_INT128 && NATIVEINT == 64 branches with
exact Python integers (numpy object arrays); integers only, so every
comparison against it is bit-exact:

* ``q_to_bsk``       DCRTPolyImpl::FastBaseConvqToBskMontgomery  dcrtpoly-impl.h:2098-2187
* ``behz_expand``    the same with its format handling           dcrtpoly-impl.h:2050-2208
* ``floor_q``        DCRTPolyImpl::FastRNSFloorq                 dcrtpoly-impl.h:2212-2271
* ``conv_sk``        DCRTPolyImpl::FastBaseConvSK                dcrtpoly-impl.h:2309-2411
* ``eval_mult_behz`` LeveledSHEBFVRNS::EvalMult, BEHZ            bfvrns-leveledshe.cpp:275-297, 383-403
* ``behz_bases``     the choice of B and msk                     bfvrns-cryptoparameters.cpp:674-703

``conv_sk`` is the CENTRED definition: for alpha > floor(msk / 2) the
correction is the residue of alpha - msk.  ``conv_sk(..., wrapping=True)`` is
the reference's unsigned ``alpha.ModSubFast(msk, q_j)`` (alpha + q_j - msk mod
2^64), which differs when a q tower is smaller than msk - alpha.

Polynomials are uint64 arrays [batch][towers][n]; "Bsk" is T.b + [T.msk].
``fast=True`` computes the same residues with 64-bit words in numpy
(bfv_ref.mulmod_const, sums taken mod m term by term) for the larger shapes;
tests/test_behz_oracle.py checks the two paths against each other.

The oracle is used for NTT / INTT, the element-wise products and the prime
search only.
"""
import json
import os

import numpy as np

import bfv_ref as BR
import bfv_tables as BT
from bfv_ref import obj, u64

HERE = os.path.dirname(os.path.abspath(__file__))


def load_vectors():
    with open(os.path.join(HERE, "golden", "behz_vectors.json")) as f:
        return json.load(f)


# ---- arithmetic on either representation ---------------------------------------------
def _tower(x, i, fast):
    return np.ascontiguousarray(x[:, i, :]) if fast else obj(x[:, i, :])


def _mm(a, c, m, fast):
    """a c mod m (ModMulFastConst: canonical for any word a)"""
    return BR.mulmod_const(a, c, m) if fast else a * int(c) % int(m)


def _dot(ys, cs, m, fast):
    """sum_i ys[i] cs[i] mod m (Mul128 sums, BarrettUint128ModUint64)"""
    if not fast:
        return sum(y * int(c) for y, c in zip(ys, cs)) % int(m)
    cur = np.zeros(ys[0].shape, dtype=np.uint64)
    for y, c in zip(ys, cs):
        cur = BR._addmod(cur, BR.mulmod_const(y, c, m), m)
    return cur


def _add(a, b, m, fast):
    return BR._addmod(a, b, m) if fast else (a + b) % int(m)


def _sub(a, b, m, fast):
    """(a - b) mod m for canonical a, b"""
    if not fast:
        return (a - b) % int(m)
    return np.where(a >= b, a - b, a + np.uint64(m) - b)


def _out(cols, fast):
    return np.ascontiguousarray(np.stack([c if fast else u64(c) for c in cols], axis=1))


# ---- the three functions ----------------------------------------------------------------
def q_to_bsk(x, T, want_r=False, fast=False):
    """x [batch][Q][n] coefficient form -> [batch][Bsk][n] (2098-2187); want_r: also r [batch][n],
    the Montgomery remainder mod mtilde before centring"""
    x = np.asarray(x, dtype=np.uint64)
    ys = [_mm(_tower(x, i, fast), T.mtildeQHatInvModq[i], T.q[i], fast) for i in range(len(T.q))]  # 2103-2111
    # 2150-2166: word sums, only the low 16 bits survive
    r = sum((BR.obj(y) if fast else y) % BT.MTILDE * h for y, h in zip(ys, T.QHatModmtilde)) % BT.MTILDE
    r = r * T.negQInvModmtilde % BT.MTILDE
    cols = []
    for j, bj in enumerate(T.bsk):
        c = _dot(ys, [T.QHatModbsk[i][j] for i in range(len(T.q))], bj, fast)                      # 2114-2126
        rj = np.where(r >= BT.MTILDE // 2, r + bj - BT.MTILDE, r)                                 # 2172-2174
        rj = u64(rj) if fast else rj
        v = _add(_mm(rj, T.QModbsk[j], bj, fast), c, bj, fast)                                     # 2176-2179
        cols.append(_mm(v, T.mtildeInvModbsk[j], bj, fast))                                        # 2180-2181
    out = _out(cols, fast)
    return (out, np.array(r, dtype=np.int64)) if want_r else out


def floor_q(x, T, fast=False):
    """x [batch][Q + Bsk][n] coefficient form -> [batch][Bsk][n] (2212-2271)"""
    x = np.asarray(x, dtype=np.uint64)
    Q = len(T.q)
    ys = [_mm(_tower(x, i, fast), T.tQHatInvModq[i], T.q[i], fast) for i in range(Q)]              # 2230-2240
    cols = []
    for j, bj in enumerate(T.bsk):
        conv = _dot(ys, [T.qInvModbsk[i][j] for i in range(Q)], bj, fast)                          # 2243-2254
        own = _mm(_tower(x, Q + j, fast), T.tQInvModbsk[j], bj, fast)                              # 2264-2265
        cols.append(_sub(own, conv, bj, fast))                                                     # 2266
    return _out(cols, fast)


def conv_sk(x, T, want_alpha=False, fast=False, wrapping=False):
    """x [batch][Bsk][n] -> [batch][Q][n] (2309-2411), the centred correction; wrapping = True (exact
    integers only): the reference's unsigned ModSubFast instead.  want_alpha: also alpha [batch][n]
    in [0, msk) as Python integers"""
    x = np.asarray(x, dtype=np.uint64)
    nb, msk = len(T.b), T.msk
    zs = [_mm(_tower(x, i, fast), T.BHatInvModb[i], T.b[i], fast) for i in range(nb)]              # 2331-2338
    a = _sub(_dot(zs, T.BHatModmsk, msk, fast), _tower(x, nb, fast), msk, fast)                    # 2355-2371
    a = _mm(a, T.BInvModmsk, msk, fast)                                                            # 2372
    neg = a > (np.uint64(msk // 2) if fast else msk // 2)                                          # 2376, 2384
    if fast:
        mag = np.where(neg, np.uint64(msk) - a, a)
    else:
        neg = neg.astype(bool)
        mag = np.where(neg, msk - a, a)
    cols = []
    for j, qj in enumerate(T.q):
        s = _dot(zs, [T.BHatModq[i][j] for i in range(nb)], qj, fast)                              # 2340-2351
        if wrapping:
            assert not fast
            al = np.where(neg, (a + qj - msk) % (1 << 64), a)                                      # 2385
            cols.append((s - al * T.BModq[j] % qj) % qj)                                           # 2387-2388
            continue
        ab = _mm(mag, T.BModq[j], qj, fast)
        cols.append(np.where(neg, _add(s, ab, qj, fast), _sub(s, ab, qj, fast)))
    out = _out(cols, fast)
    return (out, BR.obj(a) if fast else a) if want_alpha else out


# ---- format handling and the multiplication ---------------------------------------------
class Ring:
    """Oracle NTT tables of the three bases of one BehzTables, and the roots the plans take"""

    def __init__(self, O, log_n, T, rq=None):
        self.n = 1 << log_n
        m = 2 * self.n
        self.rq = list(rq) if rq is not None else [O.root_of_unity(m, v) for v in T.q]
        self.rbsk = [O.root_of_unity(m, v) for v in T.bsk]
        self.tb_q, self.tb_bsk = O.Tables(self.n, T.q, self.rq), O.Tables(self.n, T.bsk, self.rbsk)
        self.tb_qbsk = O.Tables(self.n, T.q + T.bsk, self.rq + self.rbsk)


def behz_expand(O, x, T, ring, eval_form, fast=False):
    """-> [batch][Q + Bsk][n] evaluation form (2050-2208): an evaluation-form input keeps its Q towers"""
    x = np.asarray(x, dtype=np.uint64)
    coef = O.ntt_inv(x, ring.tb_q) if eval_form else x
    part_b = O.ntt_fwd(q_to_bsk(coef, T, fast=fast), ring.tb_bsk)
    part_q = x if eval_form else O.ntt_fwd(x, ring.tb_q)
    return np.concatenate([part_q, part_b], axis=1)


def eval_mult_behz(O, T, ring, c0, c1, d0, d1, fast=False):
    """(out0, out1, out2), [batch][Q][n] coefficient form, of two evaluation-form ciphertexts
    (bfvrns-leveledshe.cpp:275-297, 326-337, 383-403)"""
    qb = T.q + T.bsk
    e = [behz_expand(O, v, T, ring, True, fast) for v in (c0, c1, d0, d1)]
    mul = lambda a, b: O.eltwise("mul", a, b, qb)  # noqa: E731
    prods = [mul(e[0], e[2]), O.eltwise("add", mul(e[0], e[3]), mul(e[1], e[2]), qb), mul(e[1], e[3])]
    return [conv_sk(floor_q(O.ntt_inv(pr, ring.tb_qbsk), T, fast=fast), T, fast=fast) for pr in prods]


# ---- the choice of B and msk ---------------------------------------------------------------
def behz_bases(O, log_n, q, t):
    """(b, msk, info) by the reference's rule (bfvrns-cryptoparameters.cpp:674-703): len(q) primes by
    PreviousPrime below q[-1], msk the next one below, then msk regrown from FirstPrime(s + 1) /
    NextPrime while Q B msk < 2N t Q^2, an error once it passes 60 bits.  On a chain that is not
    descending the walk can meet a prime of q; such a prime is skipped (info["skipped"] lists them),
    which changes nothing on the reference's own descending chains.  info["grown"] counts the trips
    of the msk loop."""
    m = 2 << log_n
    q = [int(v) for v in q]
    skipped = []

    def prev(p):
        p = O.previous_prime(p, m)
        while p in q:
            skipped.append(p)
            p = O.previous_prime(p, m)
        return p

    b = [prev(q[-1])]
    while len(b) < len(q):
        b.append(prev(b[-1]))
    msk = prev(b[-1])
    s = msk.bit_length()
    Q, B = BT.product(q), BT.product(b)
    grown = 0
    while Q * B * msk < m * t * Q * Q:
        msk = O.next_prime(O.first_prime(s + 1, m), m)
        while msk in q or msk in b:
            skipped.append(msk)
            msk = O.next_prime(msk, m)
        grown += 1
        s += 1
        if s >= 60:
            raise ValueError("msk is larger than 60 bits")
    return b, msk, {"skipped": skipped, "grown": grown}


# ---- shared inputs of the GPU parity tests and their coverage checks -------------------------
# (name, log_n, size_q, size_b).  size_b == size_q cases take B and msk from behz_bases on a 60-bit
# chain ("kat": the known answer's q); "mixed" is a chain of 22-60-bit towers, the largest last, so
# B and msk are 60-bit and three q towers are below msk / 2; "uneven" has size_b != size_q.  The
# target tile of the kernels is 4 towers wide: the Bsk kernels have size_b + 1 targets (4 at size_b
# = 3, 5 at 4), FastBaseConvSK size_q (4 and 5 at log_n 10); the limb kernel of q -> Bsk (up to 16
# sources) has tiles of 8 targets (size_b + 1 = 8 and 9 at "ltile", "ltile1"); 16 and 17 straddle the
# fused kernel's column cap and the limb kernel's source cap.
T_PLAIN = 65537
PT = 4
LIMB_PT = 8
FUSED_MAX_B = 16
CASES = [("n2", 1, 1, 1), ("kat", 3, 2, 2), ("odd", 5, 3, 3), ("tile", 10, PT, PT), ("tile1", 10, PT + 1, PT + 1),
         ("ltile", 10, LIMB_PT - 1, LIMB_PT - 1), ("ltile1", 10, LIMB_PT, LIMB_PT), ("cap", 12, 16, 16),
         ("cap1", 12, 17, 17), ("mixed", 6, 4, 4), ("uneven", 6, 2, 4)]
MIXED_BITS = [22, 45, 31, 60]
BATCH = 3
R_TARGETS = [0, 0x7FFF, 0x8000, 0xFFFF]
_cases = {}


def case_moduli(O, name, log_n, sq, sb):
    """(q, roots of q, b, msk) of one CASES entry"""
    if name == "kat":
        q = load_vectors()["q"]
        rq = [O.root_of_unity(2 << log_n, v) for v in q]
    elif name == "mixed":
        from test_mixed_moduli_oracle import mixed_chain

        q, rq = mixed_chain(log_n, MIXED_BITS, generic=True)
    elif name == "uneven":
        m, r = O.moduli_chain(log_n, sq + sb + 1)
        return m[:sq], r[:sq], m[sq:sq + sb], m[sq + sb]
    else:
        q, rq = O.moduli_chain(log_n, sq)
    b, msk, _ = behz_bases(O, log_n, q, T_PLAIN)
    return q, rq, b, msk


def alpha_targets(msk):
    return [0, msk // 2, msk // 2 + 1, msk - 1]


def plant_r(T, x, target, rng):
    """residues of one coefficient (a column of x, [Q]) whose Montgomery remainder r is `target`:
    towers 1.. as given, x_0 found by a vectorised search over 2^20 candidates"""
    q0 = T.q[0]
    cand = rng.integers(0, q0, size=1 << 20, dtype=np.uint64)
    y0 = BR.mulmod_const(cand, T.mtildeQHatInvModq[0], q0) & np.uint64(0xFFFF)
    rest = sum(int(x[i]) * T.mtildeQHatInvModq[i] % T.q[i] % BT.MTILDE * T.QHatModmtilde[i]
               for i in range(1, len(T.q))) % BT.MTILDE
    r = ((y0 * np.uint64(T.QHatModmtilde[0] % BT.MTILDE) + np.uint64(rest)) & np.uint64(0xFFFF)) \
        * np.uint64(T.negQInvModmtilde) & np.uint64(0xFFFF)
    hit = np.flatnonzero(r == np.uint64(target))
    assert hit.size, "no candidate with this remainder"
    col = [int(v) for v in x]
    col[0] = int(cand[hit[0]])
    return col


def plant_alpha(T, target, rng):
    """Bsk residues of Y = small - k B whose alpha is `target`: with z_i from small alone the
    overshoot alpha' = (sum_i z_i B / b_i - small) / B is known, and k = target - alpha' mod msk"""
    small = int(rng.integers(0, 1 << 40))
    z = [small % bi * h % bi for bi, h in zip(T.b, T.BHatInvModb)]
    over = (sum(zi * (T.B // bi) for zi, bi in zip(z, T.b)) - small) // T.B
    k = (target - over) % T.msk
    return [small % bi for bi in T.b] + [(small - k * T.B) % T.msk]


def case(O, name):
    """One CASES entry, built once: dict with T (BehzTables), ring roots rq, and the inputs
    xq [BATCH][Q][n] (q -> Bsk; coefficients 0..3 of the flattened (batch, n) order planted with
    r = R_TARGETS), xqb [BATCH][Q + Bsk][n] (floor; uniform) and xb [BATCH][Bsk][n] (SK; coefficients
    0..3 planted with alpha = alpha_targets(msk)).  With n = 2 the planted ones spill into batch
    entry 1; the other coefficients are uniform."""
    if name in _cases:
        return _cases[name]
    _, log_n, sq, sb = next(c for c in CASES if c[0] == name)
    q, rq, b, msk = case_moduli(O, name, log_n, sq, sb)
    T = BT.BehzTables(q, b, msk, T_PLAIN)
    n = 1 << log_n
    fast = sq >= 16
    for salt in range(64):
        # the seed is advanced until the unplanted coefficients hold both sides of r >= 2^15 and both
        # signs of the centred alpha (only the six-coefficient case ever needs a second draw)
        rng = np.random.default_rng(7000 + 97 * log_n + 13 * sq + sb + 1000 * salt)
        uni = lambda mods: np.stack([np.stack([rng.integers(0, int(m), size=n, dtype=np.uint64) for m in mods])  # noqa: E731
                                     for _ in range(BATCH)])
        xq, xqb, xb = uni(T.q), uni(T.q + T.bsk), uni(T.bsk)
        r = q_to_bsk(xq, T, want_r=True, fast=fast)[1].reshape(-1)[len(R_TARGETS):]
        a = conv_sk(xb, T, want_alpha=True, fast=fast)[1].reshape(-1)[len(R_TARGETS):]
        if (r >= 0x8000).any() and (r < 0x8000).any() and (a > msk // 2).any() and (a <= msk // 2).any():
            break
    for k, target in enumerate(R_TARGETS):
        xq[k // n, :, k % n] = plant_r(T, xq[k // n, :, k % n], target, rng)
    for k, target in enumerate(alpha_targets(msk)):
        xb[k // n, :, k % n] = plant_alpha(T, target, rng)
    _cases[name] = dict(T=T, rq=rq, log_n=log_n, n=n, xq=xq, xqb=xqb, xb=xb, fast=fast)
    return _cases[name]
