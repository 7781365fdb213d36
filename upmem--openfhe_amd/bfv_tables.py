"""CRT tables of the BFV (HPS family) multiplication for one level, with Python
integers and floats only (no device, no native library).

A restatement of ``CryptoParametersBFVRNS::PrecomputeCRTTables``
(pke/lib/scheme/bfvrns/bfvrns-cryptoparameters.cpp) for the full level: every
table the calls of ``ofhe_hip.py`` (``BaseConverter``, ``ScaleRound``,
``BfvMult``) take.  The reference's line numbers are cited at each table.

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
