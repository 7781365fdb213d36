"""CPU tests of the BFV entry points' boundary and of bfv_tables.py: the new
calls reject NULL handles before touching a device, and the pure-Python tables
agree with the constants the existing known-answer test derives and with their
defining identities."""
import ctypes
from fractions import Fraction

import bfv_tables as BT
from conftest import load_golden
from test_oracle import fast_expand_constants

REF = load_golden("reference_fixtures.json")


def test_bfv_argument_errors_without_device():
    import ofhe_hip as H

    L = H.lib()
    vp = ctypes.c_void_p
    null = vp()
    q = (ctypes.c_uint64 * 2)(97, 193)
    fr = (ctypes.c_double * 2)(0.25, 0.5)
    cases = [
        L.ofhe_hip_switch_crt_basis(null, null, null, 1, null),
        L.ofhe_hip_expand_crt_basis(null, null, null, 1, null, null, 1, null),
        L.ofhe_hip_scale_round_create(null, 4, 1, 1, q, q, 0, q, fr, ctypes.byref(vp())),
        L.ofhe_hip_scale_round_destroy(null),
        L.ofhe_hip_scale_and_round(null, null, null, 1, null),
        L.ofhe_hip_bfv_mult_create(null, 0, null, null, null, null, null, null, null, ctypes.byref(vp())),
        L.ofhe_hip_bfv_mult_destroy(null),
        L.ofhe_hip_bfv_eval_mult(null, null, null, null, null, null, null, null, 1, null),
    ]
    assert all(rc != 0 for rc in cases), cases
    assert L.ofhe_hip_last_error()


def test_tables_match_the_known_answer_constants():
    """mNegRlQHatInvModq / qInvModr equal the constants test_kat_fast_expand_crt_basis uses"""
    k = REF["kat_fast_expand_crt_basis"]
    T = BT.BfvTables(k["q"], k["r"], 65537, BT.HPSPOVERQ)
    c, d = fast_expand_constants(k["q"], k["r"])
    assert T.neg_r_q_hat_inv_modq == c and T.q_inv_modr == d


def test_table_identities():
    """CRT: sum_i [QHat_i^-1]_{q_i} QHat_i = 1 mod Q; alpha rows are multiples of Q mod r_j; the
    ScaleAndRound tables split t R / q_i (HPS) into integer and fractional part: table + frac
    reassemble t R QHatQR_i^-1 / q_i up to the double's rounding."""
    q = [1152921504606846577, 1152921504606846097]
    r = [1152921504606845777, 1152921504606845473, 1152921504606844513]
    t = 65537
    T = BT.BfvTables(q, r, t, BT.HPS)
    assert sum(h * (T.Q // qi) for h, qi in zip(T.q_hat_inv_modq, q)) % T.Q == 1
    assert sum(h * (T.R // rj) for h, rj in zip(T.r_hat_inv_modr, r)) % T.R == 1
    assert T.q_hat_modr == [[T.Q // qi % rj for rj in r] for qi in q]
    assert T.alpha_q_modr == [[a * T.Q % rj for rj in r] for a in range(len(q) + 1)]
    assert T.q_inv == [1.0 / qi for qi in q]
    assert len(T.sr_table) == len(r) and all(len(row) == len(q) + 1 for row in T.sr_table)
    for i, qi in enumerate(q):
        X = t * T.R * pow(T.Q * T.R // qi, -1, qi)
        for j, rj in enumerate(r):
            assert T.sr_table[j][i] == X // qi % rj
        assert abs(Fraction(T.sr_frac[i]) - Fraction(X % qi, qi)) < Fraction(1, 1 << 52)
        assert 0.0 <= T.sr_frac[i] < 1.0
    P = BT.BfvTables(q, r[:2], t, BT.HPSPOVERQ)
    assert P.out_is_q and len(P.sr_table) == len(q) and len(P.sr_frac) == 2
