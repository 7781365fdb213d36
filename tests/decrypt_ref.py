"""CPU reference of BFV decryption and of TimesQovert, restated per coefficient
from the reference with numpy float64 (one rounding per multiply, add,
subtract and divide; correctly rounded uint64 -> double) and 64-bit words /
Python integers:

* ``scale_round``        DCRTPolyImpl::ScaleAndRound -> NativePoly, HPS family  dcrtpoly-impl.h:1537-1814
  (its eight loops, labelled A-H as UnitTestBFVrnsDecrypt.cpp:126-148 does)
* ``scale_round_behz``   DCRTPolyImpl::ScaleAndRound -> NativePoly, BEHZ        dcrtpoly-impl.h:2005-2049
* ``one_tower``          MultiplyAndRound + SwitchModulus                       bfvrns-pke.cpp:233-245,
                                                                                mubintvecnat.cpp:420-435
* ``times_q_over_t``     DCRTPolyImpl::TimesQovert                              dcrtpoly-impl.h:1015-1031
* ``decrypt_core`` / ``decrypt``  PKERNS::DecryptCore / PKEBFVRNS::Decrypt      rns-pke.cpp:199-224,
                                                                                bfvrns-pke.cpp:205-248

``scale_round_scalar(..., fused=True)`` is NOT the reference: its floating chain
computes every a * b + c exactly (fractions.Fraction) and rounds once, which is
what a contracted multiply-add gives.  The sensitivity test needs it.
``tables_by_tower`` (the loop and the split point taken from another tower than
q[0]) is not the reference either; ``one_tower_scalar`` restates ``one_tower``
on one value and names the path it took.  tests/test_decrypt_cases.py needs both.

The reference's cast of a negative double to uint64 is undefined, so
``scale_round`` asserts floatSum + 0.5 >= 0 before the final cast of the loops
E-H; ``case`` replaces any input that would violate it (none has been met).

Polynomials are uint64 arrays [batch][towers][n].
"""
import copy
from fractions import Fraction

import numpy as np

import bfv_ref as BR
import bfv_tables as BT
import keyswitch as K

F64, U64 = np.float64, np.uint64


# ---- ScaleAndRound to t, HPS family ---------------------------------------------------------
def _split(v, hf):
    hi = v >> U64(hf)
    return v - (hi << U64(hf)), hi


def float_chain(x, T):
    """floatSum after the tower loop, [batch][n]: 0.5 (t a power of two) or 0.0, then per tower in order
    floatSum = floatSum + (double(x_i) * frac[i]); in the split loops for lo with frac, then hi with fracB"""
    x = np.asarray(x, dtype=U64)
    fs = np.full((x.shape[0], x.shape[2]), 0.5 if T.branch < 4 else 0.0, dtype=F64)
    for i in range(len(T.q)):
        if T.split:
            lo, hi = _split(x[:, i, :], T.q_msb_hf)
            prod = lo.astype(F64) * F64(T.tQHatInvModqDivqFrac[i])
            fs = fs + prod
            prod = hi.astype(F64) * F64(T.tQHatInvModqBDivqFrac[i])
            fs = fs + prod
        else:
            prod = x[:, i, :].astype(F64) * F64(T.tQHatInvModqDivqFrac[i])
            fs = fs + prod
    return fs


def int_sum(x, T):
    """intSum modulo 2^64 (NativeInteger words), [batch][n]: MulEqFast products in A, C, E, G;
    ModMulFastConst products mod t in B, D, F, H; AddEqFast sums"""
    x = np.asarray(x, dtype=U64)
    reduced = bool(T.branch & 1)
    mul = (lambda v, w: BR.mulmod_const(v, w, T.t)) if reduced else (lambda v, w: v * U64(w))
    acc = np.zeros((x.shape[0], x.shape[2]), dtype=U64)
    for i in range(len(T.q)):
        if T.split:
            lo, hi = _split(x[:, i, :], T.q_msb_hf)
            acc = acc + mul(lo, T.tQHatInvModqDivqModt[i])
            acc = acc + mul(hi, T.tQHatInvModqBDivqModt[i])
        else:
            acc = acc + mul(x[:, i, :], T.tQHatInvModqDivqModt[i])
    return acc


def _finish(fs, acc, T, check=True):
    if T.branch < 4:
        return (acc + fs.astype(U64)) & U64(T.t - 1)
    td = F64(T.t)
    tinv = F64(1.0) / td
    fs = fs + acc.astype(F64)
    quot = (fs * tinv).astype(U64)
    prod = td * quot.astype(F64)
    fs = fs - prod
    if check:
        assert (fs + F64(0.5) >= 0).all(), "the reference's cast of a negative double is undefined"
    return (fs + F64(0.5)).astype(U64)


def scale_round(x, T):
    """x [batch][Q][n] coefficient form -> [batch][n] (dcrtpoly-impl.h:1537-1814), len(T.q) > 1"""
    with np.errstate(over="ignore"):
        return _finish(float_chain(x, T), int_sum(x, T), T)


def defined(x, T):
    """[batch][n] bool: the final cast of the loops E-H is defined for this coefficient"""
    if T.branch < 4:
        return np.ones((x.shape[0], x.shape[2]), dtype=bool)
    with np.errstate(over="ignore"):
        fs = float_chain(x, T) + int_sum(x, T).astype(F64)
        quot = (fs * (F64(1.0) / F64(T.t))).astype(U64)
        return fs - F64(T.t) * quot.astype(F64) + F64(0.5) >= 0


def scale_round_scalar(col, T, fused=False):
    """one coefficient (col: the Q residues as Python integers) with Python floats; fused = True is NOT the
    reference: every a * b + c of the tower loop is exact and rounded once"""
    def step(fs, v, f):
        if fused:
            return float(Fraction(fs) + Fraction(float(v)) * Fraction(f))
        return fs + (float(v) * f)

    reduced, t = bool(T.branch & 1), T.t
    fs, acc = (0.5 if T.branch < 4 else 0.0), 0
    for i, v in enumerate(col):
        v = int(v)
        parts = [(v, T.tQHatInvModqDivqFrac[i], T.tQHatInvModqDivqModt[i])]
        if T.split:
            hi = v >> T.q_msb_hf
            parts = [(v - (hi << T.q_msb_hf), T.tQHatInvModqDivqFrac[i], T.tQHatInvModqDivqModt[i]),
                     (hi, T.tQHatInvModqBDivqFrac[i], T.tQHatInvModqBDivqModt[i])]
        for v, f, w in parts:
            fs = step(fs, v, f)
            acc = (acc + (v * w % t if reduced else v * w)) & (2 ** 64 - 1)
    if T.branch < 4:
        return (acc + int(fs)) & (t - 1)
    td = float(t)
    fs = fs + float(acc)
    quot = int(fs * (1.0 / td))
    fs = fs - (td * float(quot))
    return int(fs + 0.5)


def definition(v, Q, t):
    """round(t v / Q) mod t with exact integers (halves up)"""
    return (2 * t * int(v) + Q) // (2 * Q) % t


# ---- ScaleAndRound to t, BEHZ -------------------------------------------------------------------
def scale_round_behz(x, T):
    """dcrtpoly-impl.h:2005-2049: gamma = 2^26, integers only"""
    x = np.asarray(x, dtype=U64)
    s = np.zeros((x.shape[0], x.shape[2]), dtype=U64)
    for i, qi in enumerate(T.q):
        y = BR.mulmod_const(x[:, i, :], T.tgammaQHatInvModq[i], qi)
        s = BR._addmod(s, BR.mulmod_const(y, T.negInvqModtgamma[i], T.tgamma), T.tgamma)
    return (s + (s & U64((1 << BT.GAMMA_BITS) - 1))) >> U64(BT.GAMMA_BITS)


# ---- one tower ----------------------------------------------------------------------------------
def multiply_and_round(x, t, q):
    """NativeVectorT::MultiplyAndRound(t, q) (mubintvecnat.cpp:420-435) of values mod q"""
    x = np.asarray(x, dtype=U64)

    def mr(y):  # ubintnat.h:536-540: one division, one multiply, one add
        quo = y.astype(F64) / F64(q)
        prod = F64(t) * quo
        return (prod + F64(0.5)).astype(U64)

    big = x > U64(q >> 1)
    with np.errstate(over="ignore"):
        return np.where(big, U64(q) - mr(np.where(big, U64(q) - x, U64(0))), mr(np.where(big, U64(0), x)) % U64(q))


def one_tower(x, q, t):
    """x [batch][1][n] -> [batch][n] (bfvrns-pke.cpp:233-245)"""
    x = np.asarray(x, dtype=U64)
    return K.switch_modulus(multiply_and_round(x[:, 0, :], t, q), q, t)


def scale_round_any(x, T, behz=False):
    if len(T.q) == 1:
        return one_tower(x, T.q[0], T.t)
    return scale_round_behz(x, T) if behz else scale_round(x, T)


# ---- TimesQovert --------------------------------------------------------------------------------
def times_q_over_t(x, T):
    """out_i = ((x_i NegQModt) mod t) tInvModq[i] mod q_i (dcrtpoly-impl.h:1015-1031), any 64-bit x_i"""
    x = np.asarray(x, dtype=U64)
    out = np.empty_like(x)
    for i, qi in enumerate(T.q):
        y = BR.mulmod_const(x[:, i, :], T.negQModt % T.t, T.t)
        out[:, i, :] = BR.mulmod_const(y, T.tInvModq[i], qi)
    return out


# ---- DecryptCore and Decrypt ----------------------------------------------------------------------
def decrypt_core(O, elems, s, q):
    """b = c0 + c1 s (+ c2 s^2), evaluation form (rns-pke.cpp:199-224); s [Q][n] evaluation form"""
    sb = np.broadcast_to(s, elems[0].shape)
    b, sp = elems[0], sb
    for c in elems[1:]:
        b = O.eltwise("add", b, O.eltwise("mul", sp, c, q), q)
        sp = O.eltwise("mul", sp, sb, q)
    return b


def decrypt(O, elems, s, T, tb_q, eval_form, behz=False):
    """PKEBFVRNS::Decrypt (bfvrns-pke.cpp:205-248) -> [batch][n]"""
    if not eval_form:
        elems = [O.ntt_fwd(c, tb_q) for c in elems]
    return scale_round_any(O.ntt_inv(decrypt_core(O, elems, s, T.q), tb_q), T, behz)


# ---- shared cases ---------------------------------------------------------------------------------
# (t, tower bits) of every loop, towers = primes = 1 mod 2N just below 2^bits
BRANCH_TABLE = [("A", 1 << 15, 30), ("B", 1 << 31, 35), ("C", 1 << 15, 60), ("D", 1 << 31, 60), ("E", 65537, 30),
                ("F", 5308417, 30), ("F", 65537, 45), ("G", 65537, 60), ("H", 5308417, 55), ("H", 3221225473, 60)]
# (branch letter, t, tower bits, towers, log_n, batch)
HPS_CASES = [(b, t, bits, towers, 8, 3) for b, t, bits in BRANCH_TABLE for towers in (2, 5)] + \
    [("G", 65537, 50, 12, 8, 3),  # G through sizeQMSB
     # past any tile or cap on the towers
     ("F", 65537, 30, 17, 8, 3), ("H", 65537, 60, 17, 8, 3), ("C", 1 << 15, 60, 33, 8, 3), ("H", 65537, 60, 33, 8, 3),
     # a grid below one workgroup, and sixteen workgroups per batch entry
     ("C", 1 << 15, 60, 5, 1, 3), ("H", 5308417, 55, 5, 1, 3), ("C", 1 << 15, 60, 5, 12, 2),
     ("H", 5308417, 55, 5, 12, 2)]
BEHZ_CASES = [(t, towers) for towers in (2, 5, 17) for t in (2, 65537, (1 << 31) - 1)]  # 60-bit towers, N = 2^8, batch 3
ONE_TOWER_CASES = [(t, bits) for bits in (30, 60) for t in (65537, 1 << 15)]          # N = 2^8, batch 3
POOL = 1320   # planted candidates drawn per case
REAL, PLANTED, UNIFORM, EDGE = 0, 1, 2, 3
_moduli, _cases = {}, {}


def case_id(c):
    return "-".join(str(v) for v in c)


def towers_below(O, log_n, bits, count):
    """`count` primes = 1 mod 2N, the first below 2^bits, in decreasing order"""
    key = (log_n, bits, count)
    if key not in _moduli:
        m = 2 << log_n
        q, out = ((1 << bits) // m) * m + 1, []
        for _ in range(count):
            q = O.previous_prime(q, m)
            assert q.bit_length() == bits
            out.append(q)
        _moduli[key] = out
    return _moduli[key]


def encryption_sum(rng, q, t, n):
    """(b, m): b = Delta m + e mod Q as residues [1][Q][n] -- what DecryptCore and the INTT leave of an
    encryption c0 = Delta m + e - a s, c1 = a (bfv_ref.encrypt: error bound 3) -- and the plaintext m.
    Delta = floor(Q / t) makes t b / Q = m - m (Q mod t) / Q + t e / Q, so where Q is not far above t^2
    (one 30-bit tower) the plaintext is drawn below Q / (8 t^2): BFV decrypts no larger one there."""
    Q = BT.product(q)
    m = np.array([int(v) for v in rng.integers(0, min(t, max(2, Q // (8 * t * t))), size=n)], dtype=object)
    e = np.array([int(v) for v in rng.integers(-3, 4, size=n)], dtype=object)
    return BR.residues((((Q // t) * m + e) % Q).reshape(1, n), q), m


def planted_values(rng, Q, t, count):
    """v = floor((2k + 1) Q / (2t)) + delta, random k, |delta| <= 16: on a rounding boundary of t v / Q"""
    return [((2 * int(rng.integers(0, t)) + 1) * Q // (2 * t) + int(rng.integers(-16, 17))) % Q for _ in range(count)]


def fused_differs(col, T):
    return scale_round_scalar(col, T, fused=True) != scale_round_scalar(col, T)


def tables_by_tower(T, q_ref, rederive=True):
    """NOT the reference: T's tables with the loop choice and the split point taken from the tower q_ref where the
    reference takes them from q[0] (dcrtpoly-impl.h:1547).  What a kernel that branched or split on another tower
    would compute; the sensitivity tests of tests/test_decrypt_cases.py need it.  rederive = False keeps the B
    tables of q[0]'s split point, as a kernel does whose tables come from the caller and whose shift does not."""
    W = copy.copy(T)
    W.q_msb_hf = int(q_ref).bit_length() >> 1
    W.branch = BT.decrypt_branch(len(T.q), int(q_ref), T.t)
    W.split = bool(W.branch & 2)
    if not rederive:
        return W
    XB = [(T.t * h) << W.q_msb_hf for h in BT.hat_inv(T.q)]
    W.tQHatInvModqBDivqModt = [x // m % T.t for x, m in zip(XB, T.q)]
    W.tQHatInvModqBDivqFrac = [float(x % m) / float(m) for x, m in zip(XB, T.q)]
    return W


def one_tower_scalar(v, q, t):
    """one value of one_tower with Python integers and floats (mubintvecnat.cpp:420-435, ubintnat.h:536-540,
    mubintvecnat.cpp:111-136; every word wraps mod 2^64 as NativeInteger's does) -> (output, the path it took):
    path holds "upper" / "lower" (the side of q / 2), "wrapped" (q - MR(q - v) below zero), "reduced" (MR(v) >= q)
    and the SwitchModulus branch "up" (t > q), "small" (q <= 2 t) or "down"."""
    M = (1 << 64) - 1
    mr = lambda y: int(float(t) * (float(y) / float(q)) + 0.5)  # noqa: E731
    path = set()
    if v > q >> 1:
        path.add("upper")
        if mr(q - v) > q:
            path.add("wrapped")
        r = (q - mr(q - v)) & M
    else:
        path.add("lower")
        r = mr(v)
        if r >= q:
            path.add("reduced")
            r %= q
    if r > q >> 1:
        r = (r + (t - q if t > q else t - q % t)) & M
    if t > q:
        path.add("up")
    else:
        path.add("small" if q <= 2 * t else "down")
        if r >= t:
            r %= t
    return r, path


def hps_case(O, c):
    """One HPS_CASES entry, built once: dict with T, x [batch][Q][n], kinds [batch][n], plain (the
    plaintext of batch entry 0), pool_hot / pool (how many of the POOL planted candidates tell a fused
    chain from the reference's).  Batch entry 0 is a real encryption; of the other coefficients three
    quarters are PLANTED -- drawn from the pool, those first on which the fused chain gives another
    output -- and the rest UNIFORM residues."""
    key = ("hps",) + tuple(c)
    if key in _cases:
        return _cases[key]
    letter, t, bits, towers, log_n, batch = c
    n = 1 << log_n
    q = towers_below(O, log_n, bits, towers)
    T = BT.DecryptTables(q, t)
    rng = np.random.default_rng(4000 + 131 * towers + 17 * bits + log_n + t % 1009)
    rest = n * (batch - 1)
    planted = rest * 3 // 4
    cols = [[v % m for m in q] for v in planted_values(rng, T.Q, t, max(POOL, planted))]
    hot = [fused_differs(col, T) for col in cols]
    cols = [col for col, h in zip(cols, hot) if h] + [col for col, h in zip(cols, hot) if not h]
    x = np.empty((batch, towers, n), dtype=U64)
    x[:1], plain = encryption_sum(rng, q, t, n)
    tail = np.array(cols[:planted], dtype=U64).reshape(planted, towers)
    uni = np.stack([rng.integers(0, m, size=rest - planted, dtype=U64) for m in q], axis=1)
    x[1:] = np.concatenate([tail, uni]).reshape(batch - 1, n, towers).transpose(0, 2, 1)
    kinds = np.concatenate([np.full(n, REAL), np.full(planted, PLANTED), np.full(rest - planted, UNIFORM)])
    for _ in range(64):  # an input whose final cast would be undefined is replaced
        bad = ~defined(x, T)
        if not bad.any():
            break
        for b, ri in zip(*np.nonzero(bad)):
            x[b, :, ri] = [int(rng.integers(0, m)) for m in q]
            kinds[b * n + ri] = UNIFORM
    _cases[key] = dict(T=T, log_n=log_n, n=n, batch=batch, x=np.ascontiguousarray(x), kinds=kinds.reshape(batch, n),
                       plain=plain, pool_hot=sum(hot), pool=len(hot), letter=letter)
    return _cases[key]


def behz_case(O, c):
    """One BEHZ_CASES entry: batch entry 0 a real encryption, the rest uniform"""
    key = ("behz",) + tuple(c)
    if key not in _cases:
        t, towers = c
        log_n, batch = 8, 3
        n = 1 << log_n
        q = towers_below(O, log_n, 60, towers)
        rng = np.random.default_rng(5000 + 7 * towers + t % 1009)
        x = np.stack([np.stack([rng.integers(0, m, size=n, dtype=U64) for m in q]) for _ in range(batch)])
        x[:1], plain = encryption_sum(rng, q, t, n)
        _cases[key] = dict(T=BT.DecryptTables(q, t), log_n=log_n, n=n, batch=batch, x=x, plain=plain)
    return _cases[key]


def one_tower_case(O, c):
    """One ONE_TOWER_CASES entry: batch entry 0 a real encryption; entry 1 starts with x = q >> 1,
    (q >> 1) + 1, 0 and q - 1; the rest uniform"""
    key = ("one",) + tuple(c)
    if key not in _cases:
        t, bits = c
        log_n, batch = 8, 3
        n = 1 << log_n
        q = towers_below(O, log_n, bits, 1)
        rng = np.random.default_rng(6000 + bits + t % 1009)
        x = rng.integers(0, q[0], size=(batch, 1, n), dtype=U64)
        x[:1], plain = encryption_sum(rng, q, t, n)
        x[1, 0, :4] = [q[0] >> 1, (q[0] >> 1) + 1, 0, q[0] - 1]
        _cases[key] = dict(T=BT.DecryptTables(q, t), log_n=log_n, n=n, batch=batch, x=x, plain=plain)
    return _cases[key]
