"""CRT tables of the BFV (HPS family) multiplication for one level, with Python
integers and floats only (no device, no native library).

A restatement of ``CryptoParametersBFVRNS::PrecomputeCRTTables``
(pke/lib/scheme/bfvrns/bfvrns-cryptoparameters.cpp) for the full level: every
table the calls of ``ofhe_hip.py`` (``BaseConverter``, ``ScaleRound``,
``BfvMult``, ``Behz``, ``BfvDecrypt``) take, and per level l for HPSPOVERQLEVELED
(``LeveledTables``, what ``BfvLevel`` takes; ``levels_to_drop`` restates the
reference's choice of l).  The reference's line numbers are cited at each table.

The fractional tables are ``float(X mod s_i) / float(s_i)``: the reference's
expression (two correctly rounded conversions and one IEEE division), not a
correctly rounded quotient of big integers.
"""
from __future__ import annotations

from typing import List, Sequence

HPS, HPSPOVERQ = 0, 1


def product(ms: Sequence[int]) -> int:
    r = 1
    for m in ms:
        r *= int(m)
    return r


def hat_inv(ms: Sequence[int]) -> List[int]:
    """[(M / m_i)^-1 mod m_i]: QlHatInvModq (:193-200), RlHatInvModr (:372-377)."""
    M = product(ms)
    return [pow(M // m % m, -1, m) for m in ms]


def hat_mod(ms: Sequence[int], ts: Sequence[int]) -> List[List[int]]:
    """[i][j] = (M / m_i) mod t_j: QlHatModr (:204-209, stored [j][i] there), RlHatModq (:381-386)."""
    M = product(ms)
    return [[M // m % t for t in ts] for m in ms]


def alpha_mod(ms: Sequence[int], ts: Sequence[int]) -> List[List[int]]:
    """[a][j] = a M mod t_j, a = 0 .. len(ms): alphaQlModr (:343-350), alphaRlModq (:418-424)."""
    M = product(ms)
    return [[(M % t) * a % t for t in ts] for a in range(len(ms) + 1)]


def inv_doubles(ms: Sequence[int]) -> List[float]:
    """1. / static_cast<double>(m_i): qInv (:270-273), rInv (:441-444)."""
    return [1.0 / float(int(m)) for m in ms]


def scale_round_tables(summed: Sequence[int], outs: Sequence[int], t: int, scale: int, QR: int):
    """ScaleAndRound's (tOSHatInvModsDivsModo [len(outs)][len(summed) + 1], tOSHatInvModsDivsFrac
    [len(summed)]) for the summed towers s_i, the output towers o_j, and X_s = t * scale *
    ((QR / s)^-1 mod s):

    * frac[i] = double(X_{s_i} mod s_i) / double(s_i)                      (:289-297, :532-541)
    * table[j][i] = floor(X_{s_i} / s_i) mod o_j, i < len(summed)          (:299-306, :543-551)
    * table[j][len(summed)] = floor(X_{o_j} / o_j) mod o_j                 (:308-310, :553-555)

    scale is R for HPS (modulusR, :281-283) and Q for HPSPOVERQ (modulusQ, :527)."""
    def X(s):
        return t * scale * pow(QR // s % s, -1, s)

    frac = [float(X(s) % s) / float(s) for s in summed]
    table = [[X(s) // s % o for s in summed] + [X(o) // o % o] for o in outs]
    return table, frac


class BfvTables:
    """All tables of one technique for ciphertext towers q, auxiliary towers r and plaintext modulus t."""

    def __init__(self, q: Sequence[int], r: Sequence[int], t: int, technique: int = HPS):
        self.q, self.r, self.t = [int(v) for v in q], [int(v) for v in r], int(t)
        self.technique = technique
        Q, R = product(self.q), product(self.r)
        self.Q, self.R = Q, R
        # ExpandCRTBasis Q -> R and SwitchCRTBasis R -> Q: the true CRT tables
        self.q_hat_inv_modq = hat_inv(self.q)             # :193-200
        self.q_hat_modr = hat_mod(self.q, self.r)         # :204-209, [i][j]
        self.r_hat_inv_modr = hat_inv(self.r)             # :372-377
        self.r_hat_modq = hat_mod(self.r, self.q)         # :381-386, [j][i]
        self.alpha_q_modr = alpha_mod(self.q, self.r)     # :343-350
        self.alpha_r_modq = alpha_mod(self.r, self.q)     # :418-424
        self.q_inv = inv_doubles(self.q)                  # :270-273
        self.r_inv = inv_doubles(self.r)                  # :441-444
        if technique == HPS:
            # tRSHatInvModsDivsModr / Frac (:289-311)
            self.sr_table, self.sr_frac = scale_round_tables(self.q, self.r, self.t, R, Q * R)
            self.out_is_q = False
        elif technique == HPSPOVERQ:
            if len(self.r) != len(self.q):
                raise ValueError("HPSPOVERQ needs as many auxiliary towers as ciphertext towers")
            # mNegRlQHatInvModq (:501-515) and qInvModr (:517-523)
            self.neg_r_q_hat_inv_modq = [qi - R * h % qi for qi, h in zip(self.q, self.q_hat_inv_modq)]
            self.q_inv_modr = [[pow(qi, -1, rj) for rj in self.r] for qi in self.q]
            # tQlSlHatInvModsDivsModq / Frac (:532-556)
            self.sr_table, self.sr_frac = scale_round_tables(self.r, self.q, self.t, Q, Q * R)
            self.out_is_q = True
        else:
            raise ValueError("technique must be HPS or HPSPOVERQ")

    @staticmethod
    def flat(rows) -> List[int]:
        return [v for row in rows for v in row]


class LeveledTables:
    """The tables of HPSPOVERQLEVELED at level l (the index of the last kept tower) for ciphertext
    towers q, auxiliary towers r (len(r) == len(q)) and plaintext modulus t: Q_l = q[:l+1],
    R_l = r[:l+1], Q the full chain.

    * the true CRT tables of Q_l -> R_l and R_l -> Q_l with their alpha tables: QlHatInvModq(l),
      QlHatModr(l) (:156-188), alphaQlModr(l) (:317-339), RlHatInvModr(l), RlHatModq(l) (:352-364,
      :390-416), alphaRlModq(l) (:418-439), qInv / rInv (:270-273, :441-444)
    * neg_rl_q_hat_inv_modq[i] = q_i - R_l (Q / q_i)^-1 mod q_i, i < size_q, with the FULL Q (:501-515)
    * q_inv_modr[i][j] = q_i^-1 mod r_j, i < size_q, j <= l (:517-523)
    * drop_table / drop_frac = QlQHatInvModqDivqModq(l) / Frac(l), ScaleAndRound Q -> Q_l (:592-615):
      the summed towers are q[l+1:], the outputs q[:l+1]
    * sr_table / sr_frac = tQlSlHatInvModsDivsModq(l) / Frac(l), ScaleAndRound Q_l R_l -> Q_l (:558-586)
    * ql_hat_modq[i] = (Q / Q_l) mod q_i, i <= l (:621-631)

    At l == len(q) - 1 the shared tables are BfvTables(q, r, t, HPSPOVERQ)'s and ``dropped`` is 0."""

    def __init__(self, q: Sequence[int], r: Sequence[int], t: int, l: int):
        self.q, self.r, self.t, self.l = [int(v) for v in q], [int(v) for v in r], int(t), int(l)
        if len(self.r) != len(self.q):
            raise ValueError("HPSPOVERQLEVELED needs as many auxiliary towers as ciphertext towers")
        if not 0 <= self.l < len(self.q):
            raise ValueError("l must be in [0, len(q) - 1]")
        L = self.l + 1
        self.ql, self.rl = self.q[:L], self.r[:L]
        self.dropped = len(self.q) - L
        Q, Ql, Rl = product(self.q), product(self.ql), product(self.rl)
        self.Q, self.Ql, self.Rl = Q, Ql, Rl
        self.q_hat_inv_modq = hat_inv(self.ql)
        self.q_hat_modr = hat_mod(self.ql, self.rl)
        self.r_hat_inv_modr = hat_inv(self.rl)
        self.r_hat_modq = hat_mod(self.rl, self.ql)
        self.alpha_q_modr = alpha_mod(self.ql, self.rl)
        self.alpha_r_modq = alpha_mod(self.rl, self.ql)
        self.q_inv = inv_doubles(self.ql)
        self.r_inv = inv_doubles(self.rl)
        self.neg_rl_q_hat_inv_modq = [qi - Rl * h % qi for qi, h in zip(self.q, hat_inv(self.q))]
        self.q_inv_modr = [[pow(qi, -1, rj) for rj in self.rl] for qi in self.q]
        self.drop_table, self.drop_frac = scale_round_tables(self.q[L:], self.ql, 1, Ql, Q)
        self.sr_table, self.sr_frac = scale_round_tables(self.rl, self.ql, self.t, Ql, Ql * Rl)
        self.ql_hat_modq = [Q // Ql % qi for qi in self.ql]
        self.out_is_q = True


def levels_to_drop(depth: int, size_q: int, dcrt_bits: float, n: int, t: int, sigma: float = 3.19,
                   assurance: float = 36.0, digit_size: int = 0, hybrid: bool = True, num_per_part_q: int = 1,
                   num_part_q: int = 1, threshold_parties: int = 1, gaussian_secret: bool = False,
                   extended_encryption: bool = False, key_switch: bool = False) -> int:
    """FindLevelsToDrop (bfvrns-leveledshe.cpp:77-166) with the quantities it reads from the crypto
    parameters as plain arguments, in double precision and in the reference's order of operations:
    depth = multiplicativeDepth, n = the ring dimension, t = the plaintext modulus, sigma / assurance
    = GetDistributionParameter / GetAssuranceMeasure, digit_size = GetDigitSize (relinWindow),
    hybrid = (GetKeySwitchTechnique() == HYBRID), num_per_part_q / num_part_q = GetNumPerPartQ /
    GetNumPartQ.  The result is clamped to [0, size_q - 1]; the level is l = size_q - 1 - result."""
    import math

    p = float(t)
    b_key = math.sqrt(threshold_parties) * sigma * math.sqrt(assurance) if gaussian_secret else float(threshold_parties)
    w = math.pow(2, dcrt_bits) if digit_size == 0 else math.pow(2, digit_size)
    b_err = sigma * math.sqrt(assurance)
    delta = 2. * math.sqrt(n)
    v_norm = (1. + delta * b_key) / 2. if extended_encryption else b_err * (1. + 2. * delta * b_key)

    def noise_ks(logq_prev):
        if hybrid:
            return num_per_part_q * (num_part_q * delta * b_err + delta * b_key + 1.0) / 2
        return delta * (math.floor(logq_prev / (math.log(2) * dcrt_bits)) + 1) * w * b_err

    c1 = delta * delta * p * b_key

    def c2(logq_prev):
        return delta * delta * b_key * b_key / 2.0 + noise_ks(logq_prev)

    def logq_bfv(logq_prev):
        if depth > 0:
            return math.log(4 * p) + (depth - 1) * math.log(c1) + math.log(c1 * v_norm + depth * c2(logq_prev))
        return math.log(p * (4 * v_norm))

    logq_prev = 6. * math.log(10)
    logq = logq_bfv(logq_prev)
    while math.fabs(logq - logq_prev) > math.log(1.001):
        logq_prev = logq
        logq = logq_bfv(logq_prev)
    loge = logq / math.log(2) - 2 - math.log2(p)
    log_extra = math.log2(noise_ks(logq)) if key_switch else math.log2(delta)
    levels = math.floor((loge - 2 * depth - 16 - log_extra) / dcrt_bits)
    return max(0, min(int(levels), size_q - 1))


MTILDE = 1 << 16  # m_mtilde, the Montgomery modulus of the BEHZ base extension


class BehzTables:
    """The BEHZ tables of ``PrecomputeCRTTables`` (:665-851) for ciphertext towers q, auxiliary towers
    b, the extra modulus msk and plaintext modulus t.  "bsk" is b followed by msk.  The class takes B
    and msk as given (the reference chooses them at :674-703); Shoup and Barrett constants are not
    tables of this class (the library derives them)."""

    TABLES = ("tQHatInvModq", "QHatModbsk", "QHatModmtilde", "qInvModbsk", "mtildeQHatInvModq",
              "negQInvModmtilde", "QModbsk", "mtildeInvModbsk", "tQInvModbsk", "BHatInvModb", "BHatModq",
              "BHatModmsk", "BInvModmsk", "BModq")

    def __init__(self, q: Sequence[int], b: Sequence[int], msk: int, t: int):
        self.q, self.b, self.msk, self.t = [int(v) for v in q], [int(v) for v in b], int(msk), int(t)
        self.bsk = self.b + [self.msk]
        Q, B = product(self.q), product(self.b)
        self.Q, self.B = Q, B
        qhi = hat_inv(self.q)
        self.tQHatInvModq = [h * self.t % m for h, m in zip(qhi, self.q)]            # :724-735
        self.QHatModbsk = hat_mod(self.q, self.bsk)                                  # :737-747, [i][j]
        self.QHatModmtilde = [Q // m % MTILDE for m in self.q]                       # :748
        self.qInvModbsk = [[pow(m, -1, bj) for bj in self.bsk] for m in self.q]      # :751-757, [i][j]
        self.mtildeQHatInvModq = [h * MTILDE % m for h, m in zip(qhi, self.q)]       # :759-772
        self.negQInvModmtilde = (MTILDE - 1) * pow(Q, -1, MTILDE) % MTILDE           # :774-777
        self.QModbsk = [Q % bj for bj in self.bsk]                                   # :779-787
        self.mtildeInvModbsk = [pow(MTILDE % bj, -1, bj) for bj in self.bsk]         # :789-797
        self.tQInvModbsk = [pow(Q, -1, bj) * self.t % bj for bj in self.bsk]         # :799-808
        self.BHatInvModb = hat_inv(self.b)                                           # :810-821
        self.BHatModq = hat_mod(self.b, self.q)                                      # :823-832, [i][j]
        self.BHatModmsk = [B // bi % self.msk for bi in self.b]                      # :834-839
        self.BInvModmsk = pow(B, -1, self.msk)                                       # :841-843
        self.BModq = [B % m for m in self.q]                                         # :845-851

    def flat(self, name: str) -> List[int]:
        """the table as the flat row-major list of words the C ABI takes (a scalar as one word)"""
        v = getattr(self, name)
        if isinstance(v, int):
            return [v]
        return [w for row in v for w in row] if v and isinstance(v[0], list) else list(v)


BEHZ = 2          # the decryption handle's technique next to HPS / HPSPOVERQ
GAMMA_BITS = 26   # m_gamma = 2^26 (rns-cryptoparameters.h:1701)
BRANCHES = "ABCDEFGH"  # the reference's labels of ScaleAndRound's eight loops (UnitTestBFVrnsDecrypt.cpp:126-148)


def decrypt_branch(size_q: int, q0: int, t: int) -> int:
    """Which of the eight loops DCRTPolyImpl::ScaleAndRound -> NativePoly takes (dcrtpoly-impl.h:1547-1803), as
    an index into BRANCHES: MSB is the bit length (GetMSB), qMSB that of q[0]."""
    q_msb, t_msb, s_msb = int(q0).bit_length(), int(t).bit_length(), int(size_q).bit_length()
    pow2 = t & (t - 1) == 0
    split = q_msb + s_msb >= 52
    bits = ((q_msb >> 1) if split else q_msb) + t_msb + s_msb
    reduced = bits >= ((62 if split else 63) if pow2 else 52)
    return (0 if pow2 else 4) + (2 if split else 0) + (1 if reduced else 0)


class DecryptTables:
    """The tables of decryption and of TimesQovert for ciphertext towers q and plaintext modulus t, from
    ``PrecomputeCRTTables`` (bfvrns-cryptoparameters.cpp): with X_i = t ((Q / q_i)^-1 mod q_i),

    * tQHatInvModqDivqModt[i] = floor(X_i / q_i) mod t, tQHatInvModqDivqFrac[i] = double(X_i mod q_i) /
      double(q_i)                                                                       (:453-485)
    * the same for X_i 2^qMSBHf: tQHatInvModqBDivqModt / Frac; the reference fills them only when
      qMSB + sizeQMSB >= 52 (``split``), this class always                              (:474-493)
    * tgamma = t 2^26, negInvqModtgamma[i] = -(q_i^-1) mod tgamma, tgammaQHatInvModq[i] =
      t 2^26 (Q / q_i)^-1 mod q_i                                                       (:853-884)
    * tInvModq[i] = t^-1 mod q_i, negQModt = t - (Q mod t)                              (:87-94)

    ``branch`` is the loop the reference takes (an index into BRANCHES)."""

    TABLES = ("tQHatInvModqDivqModt", "tQHatInvModqBDivqModt", "tQHatInvModqDivqFrac", "tQHatInvModqBDivqFrac",
              "tgammaQHatInvModq", "negInvqModtgamma", "tInvModq", "negQModt")

    def __init__(self, q: Sequence[int], t: int):
        self.q, self.t = [int(v) for v in q], int(t)
        Q = product(self.q)
        self.Q = Q
        self.q_msb_hf = self.q[0].bit_length() >> 1
        self.branch = decrypt_branch(len(self.q), self.q[0], self.t)
        self.split = bool(self.branch & 2)
        X = [self.t * h for h in hat_inv(self.q)]
        XB = [x << self.q_msb_hf for x in X]
        self.tQHatInvModqDivqModt = [x // m % self.t for x, m in zip(X, self.q)]
        self.tQHatInvModqDivqFrac = [float(x % m) / float(m) for x, m in zip(X, self.q)]
        self.tQHatInvModqBDivqModt = [x // m % self.t for x, m in zip(XB, self.q)]
        self.tQHatInvModqBDivqFrac = [float(x % m) / float(m) for x, m in zip(XB, self.q)]
        self.tgamma = self.t << GAMMA_BITS
        self.negInvqModtgamma = [(self.tgamma - 1) * pow(m, -1, self.tgamma) % self.tgamma for m in self.q]
        self.tgammaQHatInvModq = [h * (1 << GAMMA_BITS) % m * self.t % m for h, m in zip(hat_inv(self.q), self.q)]
        self.tInvModq = [pow(self.t, -1, m) for m in self.q]
        self.negQModt = self.t - Q % self.t
