"""CPU: the tables of HPSPOVERQLEVELED (bfv_tables.LeveledTables, levels_to_drop) against their
definitions with Python integers, and the restated levelled EvalMult / RelinearizeCore
(tests/bfv_leveled_ref.py) against exact-integer decryption at every level.

The reference's unit tests hold no known answer for the levelled pieces, so the restatement is
pinned by definitions: the drop is round(x Q_l / Q) up to the double sum's error (bound derived in
bfv_leveled_ref.drop_bound), the lift is multiplication by Q / Q_l mod Q, and a product of two
fresh encryptions decrypts to the negacyclic product of the plaintexts at every l, before and after
relinearisation.  No device, no transforms (coefficient domain, N = 16, t = 17)."""
from fractions import Fraction

import numpy as np
import pytest

import bfv_leveled_ref as LR
import bfv_ref as R
import bfv_tables as BT
import oracle as O
from test_mixed_moduli_oracle import mixed_chain

LOG_N, N, T_PLAIN = 4, 16, 17


def chains(size_q):
    """the three (name, q, r) chains of size_q + size_q towers: 50-bit, 60-bit, mixed 31-60-bit"""
    m50, _ = mixed_chain(LOG_N, [50] * (2 * size_q))
    m60, _ = O.moduli_chain(LOG_N, 2 * size_q)
    mixq, _ = mixed_chain(LOG_N, [60, 35, 45, 31, 58][:size_q], generic=True)
    mixr, _ = mixed_chain(LOG_N, [60, 36, 46, 32, 59][:size_q])
    assert not set(mixq) & set(mixr)
    return [("50", m50[:size_q], m50[size_q:]), ("60", m60[:size_q], m60[size_q:]), ("mixed", mixq, mixr)]


CASES = [(sq, name, q, r) for sq in (4, 5) for name, q, r in chains(sq)]
IDS = [f"{sq}x{name}" for sq, name, _, _ in CASES]


# ---- tables -------------------------------------------------------------------------------------
@pytest.mark.parametrize("sq,name,q,r", CASES, ids=IDS)
def test_tables_match_their_definitions(sq, name, q, r):
    for l in range(sq):
        T = BT.LeveledTables(q, r, T_PLAIN, l)
        L = l + 1
        ql, rl = q[:L], r[:L]
        Q, Ql, Rl = BT.product(q), BT.product(ql), BT.product(rl)
        assert (T.ql, T.rl, T.dropped) == (ql, rl, sq - L)
        for i, qi in enumerate(ql):
            assert T.q_hat_inv_modq[i] * (Ql // qi) % qi == 1
            assert T.q_hat_modr[i] == [Ql // qi % rj for rj in rl]
            assert T.ql_hat_modq[i] == (Q // Ql) % qi and T.ql_hat_modq[i] < qi
        for j, rj in enumerate(rl):
            assert T.r_hat_inv_modr[j] * (Rl // rj) % rj == 1
            assert T.r_hat_modq[j] == [Rl // rj % qi for qi in ql]
        assert T.alpha_q_modr == [[a * Ql % rj for rj in rl] for a in range(L + 1)]
        assert T.alpha_r_modq == [[a * Rl % qi for qi in ql] for a in range(L + 1)]
        assert T.q_inv == [1.0 / float(v) for v in ql] and T.r_inv == [1.0 / float(v) for v in rl]
        # the negated constant uses the FULL Q and all size_q towers
        assert len(T.neg_rl_q_hat_inv_modq) == sq
        for i, qi in enumerate(q):
            assert (T.neg_rl_q_hat_inv_modq[i] + Rl * pow(Q // qi, -1, qi)) % qi == 0
            assert 0 < T.neg_rl_q_hat_inv_modq[i] <= qi
            assert [v * qi % rj for v, rj in zip(T.q_inv_modr[i], rl)] == [1] * L
        # the drop: X_s = Q_l ((Q / s)^-1 mod s) for a dropped tower s, and for a kept tower
        k = sq - L
        assert len(T.drop_frac) == k and len(T.drop_table) == L and all(len(row) == k + 1 for row in T.drop_table)
        for i, s in enumerate(q[L:]):
            X = Ql * pow(Q // s, -1, s)
            assert T.drop_frac[i] == float(X % s) / float(s) and 0 <= T.drop_frac[i] < 1
            assert [row[i] for row in T.drop_table] == [X // s % qi for qi in ql]
        for j, qj in enumerate(ql):
            X = Ql * pow(Q // qj, -1, qj)
            assert X % qj == 0 and T.drop_table[j][k] == X // qj % qj
        # the product's scale-and-round: X_s = t Q_l ((Q_l R_l / s)^-1 mod s)
        assert len(T.sr_frac) == L and len(T.sr_table) == L and all(len(row) == L + 1 for row in T.sr_table)
        for i, s in enumerate(rl):
            X = T_PLAIN * Ql * pow(Ql * Rl // s, -1, s)
            assert T.sr_frac[i] == float(X % s) / float(s)
            assert [row[i] for row in T.sr_table] == [X // s % qi for qi in ql]
        for j, qj in enumerate(ql):
            X = T_PLAIN * Ql * pow(Ql * Rl // qj, -1, qj)
            assert T.sr_table[j][L] == X // qj % qj


@pytest.mark.parametrize("sq,name,q,r", CASES, ids=IDS)
def test_full_level_equals_hpspoverq(sq, name, q, r):
    T, F = BT.LeveledTables(q, r, T_PLAIN, sq - 1), BT.BfvTables(q, r, T_PLAIN, BT.HPSPOVERQ)
    for name_ in ("q_hat_inv_modq", "q_hat_modr", "r_hat_inv_modr", "r_hat_modq", "alpha_q_modr", "alpha_r_modq",
                  "q_inv", "r_inv", "q_inv_modr", "sr_table", "sr_frac", "out_is_q"):
        assert getattr(T, name_) == getattr(F, name_), name_
    assert T.neg_rl_q_hat_inv_modq == F.neg_r_q_hat_inv_modq
    assert T.dropped == 0 and T.drop_frac == [] and T.ql_hat_modq == [1] * sq
    with pytest.raises(ValueError):
        BT.LeveledTables(q, r, T_PLAIN, sq)
    with pytest.raises(ValueError):
        BT.LeveledTables(q, r[:-1], T_PLAIN, 0)


def test_levels_to_drop_is_clamped_and_monotone():
    """FindLevelsToDrop's estimate of the noise grows with the depth already consumed, so the number
    of droppable levels never shrinks with it: the kept level l = size_q - 1 - levels is clamped to
    [0, size_q - 1] and non-increasing in the depth."""
    for size_q, bits, n, t in [(4, 60, 1 << 13, 65537), (8, 60, 1 << 14, 65537), (16, 50, 1 << 16, 786433),
                               (3, 30, 1 << 11, 17)]:
        for ks in (False, True):
            for hybrid in (True, False):
                got = [BT.levels_to_drop(d, size_q, bits, n, t, hybrid=hybrid, num_per_part_q=2, num_part_q=3,
                                         key_switch=ks) for d in range(0, 12)]
                assert all(0 <= g <= size_q - 1 for g in got), got
                kept = [size_q - 1 - g for g in got]
                assert all(a >= b for a, b in zip(kept, kept[1:])), kept
    # both clamps are reached: nothing to drop from a fresh ciphertext over 60-bit towers, everything
    # but one tower after many multiplications over small ones
    assert BT.levels_to_drop(0, 4, 60, 1 << 12, 17) == 0
    assert BT.levels_to_drop(40, 16, 30, 1 << 12, 17) == 15
    # by hand, depth 0: delta = 2 sqrt(4096) = 128, Berr = 3.19 * 6 = 19.14, Vnorm = 19.14 * 257,
    # logq = ln(17 * 4 * Vnorm), loge = log2(4 Vnorm) = 14.26..., levels = floor((loge - 16 - 7) / 2) = -5 -> 0;
    # with key_switch the extra term is log2(noiseKS) instead of log2(delta) = 7
    assert BT.levels_to_drop(0, 4, 2, 1 << 12, 17) == 0
    import math
    v = 19.14 * 257
    assert BT.levels_to_drop(1, 64, 2, 1 << 12, 17) == math.floor(
        ((math.log(4 * 17) + math.log(128. * 128. * 17 * v + (128. * 128. / 2.0 + (128 * 19.14 + 128 + 1.0) / 2)))
         / math.log(2) - 2 - math.log2(17.) - 2 - 16 - 7) / 2)


# ---- drop and lift --------------------------------------------------------------------------------
def uniform(rng, ms, n, batch=1):
    return np.stack([np.stack([rng.integers(0, m, size=n, dtype=np.uint64) for m in ms]) for _ in range(batch)])


@pytest.mark.parametrize("sq,name,q,r", CASES, ids=IDS)
def test_drop_is_rounding_division_within_the_double_sum_error(sq, name, q, r):
    rng = np.random.default_rng(sq * 7 + len(name))
    worst = {}
    for l in range(sq - 1):
        T = BT.LeveledTables(q, r, T_PLAIN, l)
        x = uniform(rng, q, 1024)
        got = R.crt_lift(LR.drop(x, T), T.ql)
        d = (got - LR.drop_exact(x, T)) % T.Ql
        d = np.array([int(v) - T.Ql if int(v) > T.Ql // 2 else int(v) for v in d.reshape(-1)], dtype=object)
        worst[l] = max(abs(int(v)) for v in d)
        assert worst[l] <= LR.drop_bound(T), (l, worst[l], float(LR.drop_bound(T)))
        if max(q) < 1 << 45:
            assert worst[l] == 0
    print(f"drop {sq}x{name}: max |d| per l = {worst}")


def test_drop_is_exact_on_small_towers():
    """chains of <= 45-bit towers: every product frac_i x_i is below 2^45 and the sum's error stays
    far below the distance of x Q_l / Q from a rounding boundary -- the restated drop IS the rounding
    division, at every level, with up to four dropped towers"""
    for bits in ([30] * 5, [45, 40, 35, 30, 22]):
        q, _ = mixed_chain(LOG_N, bits, generic=True)
        r, _ = mixed_chain(LOG_N, [b + 1 for b in bits])
        rng = np.random.default_rng(sum(bits))
        for l in range(len(q) - 1):
            T = BT.LeveledTables(q, r, T_PLAIN, l)
            x = uniform(rng, q, 1024)
            assert (R.crt_lift(LR.drop(x, T), T.ql) == LR.drop_exact(x, T)).all(), (bits, l)


@pytest.mark.parametrize("sq,name,q,r", CASES, ids=IDS)
def test_lift_multiplies_by_q_over_ql(sq, name, q, r):
    rng = np.random.default_rng(5)
    for l in range(sq):
        T = BT.LeveledTables(q, r, T_PLAIN, l)
        x = uniform(rng, T.ql, 64, batch=2)
        x[0, :, 0], x[0, :, 1] = 0, [m - 1 for m in T.ql]
        v = R.crt_lift(x, T.ql)
        assert (R.crt_lift(LR.expand_ql_hat(x, T), q) == v * (T.Q // T.Ql) % T.Q).all()
        add = uniform(rng, q, 64, batch=2)
        want = (v * (T.Q // T.Ql) + R.crt_lift(add, q)) % T.Q
        assert (R.crt_lift(LR.expand_ql_hat(x, T, add), q) == want).all()


# ---- the product decrypts at every level ----------------------------------------------------------
def fresh(rng, q):
    s = np.array([int(v) for v in rng.integers(-1, 2, size=N)], dtype=object)
    ms = [np.array([int(v) for v in rng.integers(0, T_PLAIN, size=N)], dtype=object) for _ in range(2)]
    cts = list(LR.encrypt_coef(rng, ms[0], s, q, T_PLAIN)) + list(LR.encrypt_coef(rng, ms[1], s, q, T_PLAIN))
    return s, ms, cts


@pytest.mark.parametrize("sq,name,q,r", CASES, ids=IDS)
def test_levelled_product_decrypts_at_every_level(sq, name, q, r):
    rng = np.random.default_rng(100 + sq)
    s, ms, cts = fresh(rng, q)
    want = R.negacyclic(ms[0], ms[1]) % T_PLAIN
    for l in range(sq):
        T = BT.LeveledTables(q, r, T_PLAIN, l)
        outs = LR.eval_mult_coef(T, *cts)
        assert (R.decrypt3(outs, s, q, T_PLAIN) == want).all(), l
        for o in outs:
            assert not o[:, l + 1:].any()  # the lifted polynomial is zero on the dropped towers


def test_square_equals_mult_by_itself_and_decrypts():
    sq, _, q, r = CASES[3]
    rng = np.random.default_rng(9)
    s, ms, cts = fresh(rng, q)
    for l in (0, 2, sq - 1):
        T = BT.LeveledTables(q, r, T_PLAIN, l)
        outs = LR.eval_mult_coef(T, cts[0], cts[1], cts[0], cts[1])
        assert (R.decrypt3(outs, s, q, T_PLAIN) == R.negacyclic(ms[0], ms[0]) % T_PLAIN).all(), l


@pytest.mark.parametrize("sq,name,q,r", [CASES[1], CASES[5]], ids=[IDS[1], IDS[5]])
def test_relinearised_product_decrypts_at_every_level(sq, name, q, r):
    """the restated RelinearizeCore's steps (drop the last element, key switch at l + 1 towers, lift,
    add) with a real relinearisation key for s^2: the two-element result decrypts to the product"""
    rng = np.random.default_rng(200 + sq)
    s, ms, cts = fresh(rng, q)
    p, _ = mixed_chain(LOG_N, [59, 57, 55])
    assert not set(p) & set(q)
    alpha = 2
    keys = LR.relin_key_coef(rng, s, q, p, alpha)
    want = R.negacyclic(ms[0], ms[1]) % T_PLAIN
    full = BT.LeveledTables(q, r, T_PLAIN, sq - 1)
    for l in range(sq):
        T = BT.LeveledTables(q, r, T_PLAIN, l)
        outs = LR.eval_mult_coef(T, *cts)
        c2l = R.crt_lift(LR.drop(outs[2], T), T.ql)[0]
        a0, a1 = LR.key_switch_coef(c2l, q, p, alpha, l + 1, keys)
        lift = lambda a, add: R.crt_lift(LR.expand_ql_hat(R.residues(a.reshape(1, N), T.ql), T, add), q)[0]  # noqa: E731
        got = LR.decrypt2(lift(a0, outs[0]), lift(a1, outs[1]), s, q, T_PLAIN)
        assert (got == want).all(), l
    del full


# ---- sensitivity of the scale-round-lift cases -------------------------------------------------------
def test_planted_inputs_tell_a_fused_chain_apart():
    """for each shape of the GPU scale-round-lift test, the planted coefficients give another
    floor(nu) under a fused multiply-add chain than under the contract's separately rounded one"""
    import leveled_cases as C

    for case in C.SR_LIFT_CASES:
        T, x, planted = C.sr_lift_case(*case)
        assert planted >= 1, case
        L = T.l + 1
        for k in range(planted):
            xs = [int(x[0, L + i, k]) for i in range(L)]
            assert int(LR.nu_scale_scalar(xs, T.sr_frac)) != int(LR.nu_scale_fused(xs, T.sr_frac)), (case, k)
        _, nu = LR.scale_round_product(x[:1], T, want_nu=True)
        assert [float(v) for v in nu[0, :planted]] == \
            [LR.nu_scale_scalar([int(x[0, L + i, k]) for i in range(L)], T.sr_frac) for k in range(planted)]
        assert Fraction(float(nu.max())) < 1 << 127
