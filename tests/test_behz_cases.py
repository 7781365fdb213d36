"""CPU: the committed seed range, the fixed shapes and the synthetic tables of
tests/test_gpu_fuzz_behz.py reach what that file exists for.  Conditions on the
generator (tests/behz_cases.py), not measurements: if a change to the draws
loses one of these, pin a seed in behz_cases.PINS rather than relax the count."""
from collections import Counter
from functools import lru_cache

import numpy as np

import behz_cases as C
import behz_ref as Z
import oracle as O
import tier2_cases as C2
import tier3_cases as C3
from test_tier2_cases import _at_least_twice, _log_n_class
from test_tier3_cases import CLASSES

PLANS = ("plan_q", "plan_bsk", "plan_qbsk")
LIMB = 30


@lru_cache(maxsize=None)
def _cases():
    return [C.case(seed) for seed in range(C.SEEDS)]


def _bits(c):
    return [m.bit_length() for m in c["q"] + c["b"] + [c["msk"]]]


def test_seed_range_and_shared_helpers():
    assert C.SEEDS == 40 and C.SCALE is C2.SCALE
    assert C.BASE not in set(C2.BASE.values()) | set(C3.BASE.values())
    for name in ("_moduli", "_log_n", "_plan_options", "valid_splits"):
        assert not hasattr(C, name), name + " is tier2_cases' own, not copied"
    assert C.FUSED_MAX_B == 16 and C.LIMB_QMAX == 16


def test_draws_are_deterministic_and_valid():
    for seed, c in enumerate(_cases()):
        assert c["seed"] == seed and c == C.case(seed)
        m = 2 << c["log_n"]
        mods = c["q"] + c["b"] + [c["msk"]]
        assert len(set(mods)) == len(mods) and all(v % m == 1 and 3 <= v < 1 << 60 for v in mods)
        assert all(v > 1 << 16 for v in c["b"] + [c["msk"]])
        assert 1 <= c["log_n"] <= 17 and all(v.bit_length() >= max(22, c["log_n"] + 4) for v in mods)
        assert (len(c["q"]), len(c["b"])) == (c["size_q"], c["size_b"]) and 1 <= c["batch"] <= 3
        assert c["mode"] in C.MODES
        for split, generic in c["plans"].values():
            assert split in C2.valid_splits(c["log_n"]) and generic in (0, 1)
        if "sizes" not in C.PINS.get(seed, {}):
            qmax, bmax = (2, 1) if c["log_n"] >= 15 else (3, 2) if c["log_n"] >= 13 else (6, 3)
            assert 1 <= c["size_q"] <= qmax and c["batch"] <= bmax and c["size_b"] - c["size_q"] in (-1, 0, 1)


def test_ring_sizes_and_plans():
    cs = _cases()
    assert {c["log_n"] for c in cs} == set(range(1, 18))
    _at_least_twice(Counter(_log_n_class(c["log_n"]) for c in cs), CLASSES, "ring size class")
    for log_n in (16, 17):
        for plan in PLANS:
            got = {c["plans"][plan][0] for c in cs if c["log_n"] == log_n}
            assert got >= {"SPLIT_AUTO", "SPLIT_COLS"}, f"{plan} at 2^{log_n}: {got}"
        allp = {c["plans"][p][0] for c in cs if c["log_n"] == log_n for p in PLANS}
        assert allp == set(C2.valid_splits(log_n)), f"splits at 2^{log_n}: {allp}"
    for plan in PLANS:
        _at_least_twice(Counter(c["plans"][plan][1] for c in cs), (0, 1), plan + " generic_moduli")
    assert any(len(set(c["plans"].values())) > 1 for c in cs), "the three plans' options differ somewhere"


def test_sizes_batches_and_modes():
    cs = _cases()
    _at_least_twice(Counter(c["size_q"] for c in cs), range(1, 7), "Q")
    _at_least_twice(Counter(c["size_b"] - c["size_q"] for c in cs), (-1, 0, 1), "B - Q")
    _at_least_twice(Counter(c["batch"] for c in cs), (1, 2, 3), "batch")
    _at_least_twice(Counter(c["mode"] for c in cs), C.MODES, "floor_sk mode")
    _at_least_twice(Counter(c["eval_form"] for c in cs), (True, False), "expand form")
    past = [c for c in cs if max(c["size_q"], c["size_b"]) > 16]
    assert all(c["log_n"] <= 6 and c["batch"] == 2 and len(set(_bits(c))) >= 8 for c in past)
    assert sorted((c["size_q"], c["size_b"]) for c in past) == [(17, 18), (18, 16)]
    assert any(c["size_q"] > C.LIMB_QMAX and c["size_b"] <= C.FUSED_MAX_B for c in past)  # wide sums, fused floor -> SK
    assert any(c["size_b"] > C.FUSED_MAX_B for c in past)  # the two-launch branch
    assert any(c["size_b"] > C.FUSED_MAX_B and c["mode"] == "BEHZ_FUSED" for c in past), "floor_sk refusing BEHZ_FUSED"
    assert all(c["eval_form"] for c in past)  # expand reads its sources from out's Q slots


def test_moduli():
    cs = _cases()
    mixed = [c for c in cs if min(v.bit_length() for v in c["q"]) < 32 and max(v.bit_length() for v in c["q"]) == 60
             and c["msk"].bit_length() == 60]
    assert len(mixed) >= 2, "a tower below 32 bits and one of 60 in q, and a 60-bit msk"
    below = [c for c in cs if min(c["q"]) < c["msk"] // 2]
    assert len(below) >= 4, "a q tower below msk / 2"
    assert any(max(c["q"]) > c["msk"] for c in cs), "msk smaller than some q tower"
    assert len([c for c in cs if len(set(_bits(c))) >= 3]) >= 16, "mixed sizes"
    told_apart = 0
    for c in below:
        if c["log_n"] >= C.FAST_LOG_N:
            continue
        T, xb = C.tables(c), C.standalone_inputs(c)[2]
        told_apart += not np.array_equal(Z.conv_sk(xb, T, wrapping=True), Z.conv_sk(xb, T))
    assert told_apart >= 1, "no SK input on which the centred correction differs from the wrapping one"


def test_planted_inputs():
    for c in _cases():
        T, n, batch, fast = C.tables(c), 1 << c["log_n"], c["batch"], c["log_n"] >= C.FAST_LOG_N
        xq, xqb, xb = C.standalone_inputs(c)
        assert xq.shape == (batch, len(T.q), n) and xqb.shape == (batch, len(T.q) + len(T.bsk), n)
        assert xb.shape == (batch, len(T.bsk), n)
        assert (xq < np.array(T.q, dtype=np.uint64)[None, :, None]).all()
        assert (xqb < np.array(T.q + T.bsk, dtype=np.uint64)[None, :, None]).all()
        assert (xb < np.array(T.bsk, dtype=np.uint64)[None, :, None]).all()
        k = min(4, batch * n)
        r = Z.q_to_bsk(xq, T, want_r=True, fast=fast)[1].reshape(-1)
        a = Z.conv_sk(xb, T, want_alpha=True, fast=fast)[1].reshape(-1)
        assert list(r[:k]) == Z.R_TARGETS[:k], c["seed"]
        assert [int(v) for v in a[:k]] == Z.alpha_targets(T.msk)[:k], c["seed"]
        if n * batch > 8:
            rest = np.array([int(v) > T.msk // 2 for v in a[k:]])
            assert (r[k:] >= 0x8000).any() and (r[k:] < 0x8000).any() and rest.any() and not rest.all(), c["seed"]


# ---- the synthetic extreme tables -------------------------------------------------------------------------------
def _limbs(v):
    return v & ((1 << LIMB) - 1), v >> LIMB


def test_limb_sums_of_sixteen_sources_carry():
    """k_behz_q_to_bsk_limb's decomposition on the all-large case: no limb sum overflows its word, a3 is within
    2^36 of 2^64 and a1 + a2 carries out of 64 bits (limb_reduce's `mid < a1` branch)"""
    for name in ("16-16", "16-16-n9", "16-40"):
        T, log_n, xq, _, _ = C.max_sum_case(name)
        assert len(T.q) == C.LIMB_QMAX
        for col in range(0, 1 << log_n, 2):
            ys = [int(xq[0, i, col]) * T.mtildeQHatInvModq[i] % T.q[i] for i in range(len(T.q))]
            assert ys == [m - 1 for m in T.q]
            for j in range(len(T.bsk)):
                a = [0, 0, 0, 0]
                for i, y in enumerate(ys):
                    (y0, y1), (c0, c1) = _limbs(y), _limbs(T.QHatModbsk[i][j])
                    a = [a[0] + y0 * c0, a[1] + y0 * c1, a[2] + y1 * c0, a[3] + y1 * c1]
                assert max(a) < 1 << 64 and a[3] >= (1 << 64) - (1 << 36) and a[1] + a[2] >= 1 << 64, (name, col, j)
                assert a[0] + ((a[1] + a[2]) << LIMB) + (a[3] << 2 * LIMB) == sum(
                    y * T.QHatModbsk[i][j] for i, y in enumerate(ys))
    assert 16 * ((1 << LIMB) - 1) ** 2 == (1 << 64) - (1 << 35) + 16  # a3 at y = c = 2^60 - 1: the designed bound


def test_wide_sums_of_255_sources_reach_128_bits():
    T, log_n, xq, xqb, xb = C.max_sum_case("255-255")
    assert len(T.q) == len(T.b) == 255
    sums = []
    for col in range(0, 1 << log_n, 2):
        for x, srcs, table in ((xq, T.q, T.QHatModbsk), (xqb, T.q, T.qInvModbsk), (xb, T.b, T.BHatModq)):
            for j in range(len(table[0])):
                sums.append(sum(int(x[0, i, col]) * table[i][j] for i in range(len(srcs))))
        sums.append(sum(int(xb[0, i, col]) * T.BHatModmsk[i] for i in range(len(T.b))))
    assert max(sums) < 1 << 128 and max(sums) >= 1 << 127 and min(sums) >= 1 << 127


def test_fast_path_equals_exact_integers_on_the_extreme_tables():
    for name in C.MAX_SUM_IDS:
        T, _, xq, xqb, xb = C.max_sum_case(name)
        assert (xq[0, :, 0] == np.array(T.q, dtype=np.uint64) - np.uint64(1)).all()
        assert (xb[0, :, 0] == np.array(T.bsk, dtype=np.uint64) - np.uint64(1)).all()
        assert np.array_equal(Z.q_to_bsk(xq, T, fast=True), Z.q_to_bsk(xq, T)), name
        assert np.array_equal(Z.floor_q(xqb, T, fast=True), Z.floor_q(xqb, T)), name
        assert np.array_equal(Z.conv_sk(xb, T, fast=True), Z.conv_sk(xb, T)), name


def test_spread_moduli_are_the_extremes_create_admits():
    for name, (q, b, msk) in C.SPREAD.items():
        bsk = b + [msk]
        assert len(q) == len(b) == 8 and len(set(q + bsk)) == 17 and all(m & 1 and 3 <= m < 1 << 60 for m in q + bsk)
        assert min(q) == 3 and min(bsk) == 65537 and max(q) == C.TOP - 2 and max(bsk) == C.TOP
        assert {65537, (1 << 45) + 7, (1 << 59) + 1, C.TOP} <= set(bsk) and {3, (1 << 31) + 1, C.TOP - 2} <= set(q)
    (q, b, msk), (q2, b2, msk2) = C.SPREAD["spread"], C.SPREAD["spread-msk"]
    assert (1 << 32) + 15 in b and (1 << 32) + 15 in q2  # in one handle a modulus may not repeat
    assert msk == C.TOP and msk2 == 65537


def test_past_the_caps_outputs_tell_offsets_apart():
    """the three outputs of a past-the-caps multiplication differ pairwise, and so do their batch entries: a wrong
    offset into the floors of the two-launch branch (3 * batch rows) cannot pass"""
    c = C.past_caps_case(16, 17, 5)
    assert len(c["T"].b) > C.FUSED_MAX_B and len(c["T"].q) <= C.LIMB_QMAX
    rows = [w[b] for w in c["want"] for b in range(C.PAST_BATCH)]
    assert len(rows) == 9
    for i in range(9):
        for k in range(i):
            assert (rows[i] != rows[k]).mean() > 0.9, (i, k)
    full = C.past_caps_case(17, 17, 5)
    m = O.moduli_chain(5, 35)[0]
    assert (full["T"].q, full["T"].b, full["T"].msk) == (m[:17], m[17:34], m[34])  # behz_bases continues the chain
