"""bfv_tables.BehzTables against the definition of every table
(bfvrns-cryptoparameters.cpp:724-851) and behz_ref.behz_bases against the
reference's choice of B and msk (:674-703).  CPU only."""
import pytest

import behz_ref as Z
import bfv_tables as BT

KAT = Z.load_vectors()


def chains(O):
    yield "kat", 3, KAT["q"]
    yield "one", 4, O.moduli_chain(4, 1)[0]
    yield "four", 6, O.moduli_chain(6, 4)[0]
    from test_mixed_moduli_oracle import mixed_chain

    yield "mixed", 6, mixed_chain(6, Z.MIXED_BITS, generic=True)[0]


def test_known_answer_bases(O):
    """the reference's rule gives the Bsk moduli of its own N = 8 test, without growing msk"""
    b, msk, info = Z.behz_bases(O, KAT["log_n"], KAT["q"], KAT["t"])
    assert b + [msk] == KAT["bsk"]
    assert info == {"skipped": [], "grown": 0}


def test_every_table_matches_its_definition(O):
    for name, log_n, q in chains(O):
        b, msk, _ = Z.behz_bases(O, log_n, q, Z.T_PLAIN)
        T = BT.BehzTables(q, b, msk, Z.T_PLAIN)
        Q, B, t, mt = BT.product(q), BT.product(b), Z.T_PLAIN, 1 << 16
        bsk = b + [msk]
        assert T.bsk == bsk and T.Q == Q and T.B == B and BT.MTILDE == mt
        for i, qi in enumerate(q):
            Qh = Q // qi
            assert T.tQHatInvModq[i] * Qh % qi == t % qi and 0 <= T.tQHatInvModq[i] < qi
            assert T.mtildeQHatInvModq[i] * Qh % qi == mt % qi and 0 <= T.mtildeQHatInvModq[i] < qi
            assert T.QHatModmtilde[i] == Qh % mt
            assert T.BModq[i] == B % qi
            for j, bj in enumerate(bsk):
                assert T.QHatModbsk[i][j] == Qh % bj
                assert T.qInvModbsk[i][j] * qi % bj == 1 and 0 < T.qInvModbsk[i][j] < bj
        assert (T.negQInvModmtilde * Q + 1) % mt == 0 and 0 < T.negQInvModmtilde < mt
        for j, bj in enumerate(bsk):
            assert T.QModbsk[j] == Q % bj
            assert T.mtildeInvModbsk[j] * mt % bj == 1 and 0 < T.mtildeInvModbsk[j] < bj
            assert T.tQInvModbsk[j] * Q % bj == t % bj and 0 <= T.tQInvModbsk[j] < bj
        for i, bi in enumerate(b):
            Bh = B // bi
            assert T.BHatInvModb[i] * Bh % bi == 1 and 0 < T.BHatInvModb[i] < bi
            assert T.BHatModmsk[i] == Bh % msk
            assert T.BHatModq[i] == [Bh % qj for qj in q]
        assert T.BInvModmsk * B % msk == 1 and 0 < T.BInvModmsk < msk
        # the flat forms the C ABI takes
        assert len(T.TABLES) == 14
        assert T.flat("QHatModbsk") == [T.QHatModbsk[i][j] for i in range(len(q)) for j in range(len(bsk))]
        assert T.flat("BHatModq") == [T.BHatModq[i][j] for i in range(len(b)) for j in range(len(q))]
        assert T.flat("BInvModmsk") == [T.BInvModmsk] and T.flat("negQInvModmtilde") == [T.negQInvModmtilde]
        assert T.flat("BModq") == T.BModq, name


def test_bases_are_distinct_primes_of_the_ring(O):
    for name, log_n, q in chains(O):
        b, msk, info = Z.behz_bases(O, log_n, q, Z.T_PLAIN)
        every = list(q) + b + [msk]
        assert len(set(every)) == len(every) and len(b) == len(q), name
        assert all(v % (2 << log_n) == 1 and v < 1 << 60 for v in every)
        # the walk goes down from q[-1]: B descending, msk below it unless it was regrown
        assert b == sorted(b, reverse=True) and b[0] < q[-1]
        assert info["grown"] or msk < b[-1]
        Q, B = BT.product(q), BT.product(b)
        assert Q * B * msk >= (2 << log_n) * Z.T_PLAIN * Q * Q


def test_non_descending_chain_skips_the_primes_of_q(O):
    """the largest tower last: the walk below it meets the other 60-bit towers of q"""
    log_n = 6
    q = O.moduli_chain(log_n, 3)[0][::-1]  # ascending
    b, msk, info = Z.behz_bases(O, log_n, q, Z.T_PLAIN)
    assert info["skipped"] == [q[1], q[0]]
    assert not set(q) & set(b + [msk])


def test_msk_loop_runs(O):
    """three 30-bit towers at N = 2^13, t = 65537: Q B msk < 2N t Q^2 with the 30-bit msk, so the
    loop regrows msk from FirstPrime / NextPrime"""
    log_n = 13
    q = O.moduli_chain(log_n, 3, 30)[0]
    b, msk, info = Z.behz_bases(O, log_n, q, Z.T_PLAIN)
    assert info["grown"] > 0
    Q, B = BT.product(q), BT.product(b)
    assert Q * B * msk >= (2 << log_n) * Z.T_PLAIN * Q * Q
    # s starts at the bit length of the first msk (30); trip g takes NextPrime(FirstPrime(s + g))
    m = 2 << log_n
    assert msk == O.next_prime(O.first_prime(30 + info["grown"], m), m) and msk % m == 1
    assert msk not in q + b and not info["skipped"]


def test_msk_past_60_bits_raises(O):
    """q = 60, 45, 30 bits in that order: B is about 2^90, so msk would need about 2^75"""
    from test_mixed_moduli_oracle import mixed_chain

    q = mixed_chain(10, [60, 45, 30])[0]
    with pytest.raises(ValueError, match="60 bits"):
        Z.behz_bases(O, 10, q, Z.T_PLAIN)


def test_case_table_is_what_the_kernels_need():
    """the GPU cases hold the tile width, both sides of the fused column cap, and size_b != size_q"""
    import ofhe_hip as H

    import os
    import re

    from conftest import ROOT

    src = open(os.path.join(ROOT, "upmem--openfhe_amd", "csrc", "behz_kernels.hpp")).read()
    assert int(re.search(r"BEHZ_PT = (\d+);", src).group(1)) == Z.PT
    assert int(re.search(r"BEHZ_FUSED_BMAX = (\d+);", src).group(1)) == Z.FUSED_MAX_B
    # k_behz_q_to_bsk_limb takes up to BCONV_LIMB_QMAX sources, the 128-bit kernel the rest
    elt = open(os.path.join(ROOT, "upmem--openfhe_amd", "csrc", "eltwise_kernels.hpp")).read()
    limb_max = int(re.search(r"BCONV_LIMB_QMAX = (\d+);", elt).group(1))
    assert {limb_max, limb_max + 1} <= {sq for _, _, sq, _ in Z.CASES}
    assert int(re.search(r"define OFHE_BCONV_PT (\d+)", elt).group(1)) == Z.LIMB_PT
    assert {Z.LIMB_PT, Z.LIMB_PT + 1} <= {sb + 1 for _, _, sq, sb in Z.CASES if sq <= limb_max}
    hdr = open(os.path.join(ROOT, "include", "ofhe_hip.h")).read()
    assert int(re.search(r"#define OFHE_BEHZ_FUSED_MAX_B (\d+)", hdr).group(1)) == Z.FUSED_MAX_B
    assert Z.FUSED_MAX_B == H.BEHZ_FUSED_MAX_B
    shapes = {(sq, sb) for _, _, sq, sb in Z.CASES}
    assert {(Z.PT, Z.PT), (Z.PT + 1, Z.PT + 1), (Z.FUSED_MAX_B, Z.FUSED_MAX_B),
            (Z.FUSED_MAX_B + 1, Z.FUSED_MAX_B + 1)} <= shapes
    assert any(sq != sb for sq, sb in shapes) and any(sb + 1 == Z.PT for _, sb in shapes)
    assert len({c[0] for c in Z.CASES}) == len(Z.CASES)
