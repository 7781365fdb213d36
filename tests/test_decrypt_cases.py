"""CPU: the committed seed range and the fixed inputs of
tests/test_gpu_fuzz_decrypt.py reach what that file exists for.  Conditions on
the generator (tests/decrypt_cases.py) computed from the reference
(tests/decrypt_ref.py) alone, not measurements: if a change to the draws loses
one of these, pin a seed in decrypt_cases.PINS rather than relax the condition."""
from functools import lru_cache

import numpy as np
import pytest

import behz_cases as CB
import bfv_ref as BR
import bfv_tables as BT
import decrypt_cases as C
import decrypt_ref as D
import tier2_cases as C2
import tier3_cases as C3

U64 = np.uint64


@lru_cache(maxsize=None)
def _cases():
    return [C.case(seed) for seed in range(C.SEEDS)]


def _hps(c):
    return not C.behz(c) and c["size_q"] > 1


def _is_prime(v):
    d, r = v - 1, 0
    while d % 2 == 0:
        d, r = d // 2, r + 1
    for a in (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37):  # enough below 2^64
        x = pow(a, d, v)
        if x in (1, v - 1):
            continue
        for _ in range(r - 1):
            x = x * x % v
            if x == v - 1:
                break
        else:
            return False
    return True


# ---- the sweep ------------------------------------------------------------------------------------------------
def test_seed_range_and_shared_helpers():
    assert C.SEEDS == 40 and C.SCALE is C2.SCALE
    assert C.BASE not in set(C2.BASE.values()) | set(C3.BASE.values()) | {CB.BASE}
    for name in ("_moduli", "_log_n", "_plan_options", "valid_splits"):
        assert not hasattr(C, name), name + " is tier2_cases' own, not copied"
    assert set(C.T_LIST) == {2, 1 << 15, 1 << 31, 65537, 5308417, 3221225473, C.P45, C.P55}
    assert _is_prime(C.P45) and _is_prime(C.P55) and _is_prime((1 << 32) - 5) and _is_prime((1 << 61) - 1)


def test_draws_are_deterministic_and_valid():
    for seed, c in enumerate(_cases()):
        assert c["seed"] == seed and c == C.case(seed)
        m, q = 2 << c["log_n"], c["q"]
        assert len(set(q)) == len(q) == c["size_q"] and all(v % m == 1 and 3 <= v < 1 << 60 for v in q)
        assert 1 <= c["log_n"] <= 17 and all(22 <= v.bit_length() <= 60 for v in q)
        assert c["technique"] in C.TECHNIQUES and c["elements"] in (2, 3) and c["t"] in C.T_LIST
        assert C.admissible(c["t"], q, c["technique"])
        assert 2 * len(q) * c["t"] < 1 << 64 and (not C.behz(c) or len(q) == 1 or c["t"] < 1 << 32)
        split, generic = c["plan_q"]
        assert split in C2.valid_splits(c["log_n"]) and generic in (0, 1)
        if "bits" not in C.PINS.get(seed, {}):
            assert 1 <= c["size_q"] <= (2 if c["log_n"] >= 15 else 6)
        assert 1 <= c["batch"] <= (1 if c["log_n"] >= 15 else 3)


def test_sweep_reaches_every_loop_ring_and_plan():
    cs = _cases()
    names = {C.branch_name(BT.DecryptTables(c["q"], c["t"]), C.behz(c)) for c in cs}
    assert names == set("ABCDEFGH") | {"BEHZ", "ONE_TOWER"}, names
    assert {c["log_n"] for c in cs} == set(range(1, 18))
    for log_n in (13, 16, 17):
        got = {c["plan_q"] for c in cs if c["log_n"] == log_n}
        want = {(s, g) for s in C2.valid_splits(log_n) for g in (0, 1)}
        assert got == want, f"plan options at 2^{log_n}: missing {sorted(want - got)}"
    for family in (True, False):
        mine = [c for c in cs if C.behz(c) == family and c["size_q"] > 1]
        assert {c["elements"] for c in mine} == {2, 3} and {c["eval_form"] for c in mine} == {True, False}, family
    assert {c["batch"] for c in cs} == {1, 2, 3} and {c["technique"] for c in cs} == set(C.TECHNIQUES)
    # every case runs through the decrypt call: a power-of-two loop among them
    assert any(_hps(c) and BT.DecryptTables(c["q"], c["t"]).branch < 4 for c in cs)
    assert {c["size_q"] for c in cs} >= {1, 2, 3, 4, 5, 6, 7, 8, 17}
    one = {c["log_n"] for c in cs if c["size_q"] == 1}
    assert {13, 16} <= one, one
    assert any(c["size_q"] == 17 and c["log_n"] == 10 for c in cs)


def test_pinned_chains_land_in_their_loops():
    cs = _cases()
    bits = lambda c: [m.bit_length() for m in c["q"]]  # noqa: E731
    want = {(60, 24, 45, 31, 60): "G", (27, 60, 60, 30, 52, 22, 58): "F", (30, 60): "B", (24, 60, 60): "A",
            (48,) * 7: "F", (48,) * 8: "G", (52, 60, 45): "H"}
    seen = {}
    for c in cs:
        if tuple(bits(c)) in want:
            seen[tuple(bits(c))] = C.branch_name(BT.DecryptTables(c["q"], c["t"]), C.behz(c))
    assert seen == want


@pytest.mark.parametrize("seed", range(C.SEEDS))
def test_sweep_entry_0_decrypts(seed):
    """the synthesised encryption decrypts to its plaintext under the reference, in the case's form and through
    the scale-round input alone (t stands for 0), wherever the reference's error analysis covers the chain
    (decrypt_cases.reference_decrypts); every input of the loops E-H has a defined final cast"""
    c = C.case(seed)
    k = C.sweep_inputs(c)
    T, n = k["T"], 1 << c["log_n"]
    assert len(k["elems"]) == c["elements"] and all(e.shape == (c["batch"], c["size_q"], n) for e in k["elems"])
    assert k["salt"] == 0, "an input with an undefined final cast was met: state the share in the GPU file"
    plain = k["plain"].astype(U64)
    want = C.want_decrypt(c, k)
    assert want.shape == (c["batch"], n) and (want <= U64(T.t)).all()
    if C.reference_decrypts(T, C.behz(c)):
        assert (want[0] % U64(T.t) == plain).all(), seed
    direct = D.scale_round_any(k["x"], T, C.behz(c))
    assert np.array_equal(direct, want), "the two forms of the call are one computation"
    if _hps(c):
        assert D.defined(k["x"], T).all()


def test_reference_decrypts_most_of_the_sweep():
    """the chains behind a narrower q[0] and the sums past 2^52, on which the reference itself does not decrypt,
    stay a minority, and every family keeps a case that decrypts"""
    ok = [c for c in _cases() if C.reference_decrypts(BT.DecryptTables(c["q"], c["t"]), C.behz(c))]
    assert len(ok) >= 28, len(ok)
    names = {C.branch_name(BT.DecryptTables(c["q"], c["t"]), C.behz(c)) for c in ok}
    assert names >= set("ACDEFG") | {"BEHZ", "ONE_TOWER"}, names  # B and H are the pinned chains behind a narrow q[0]
    assert any(len(set(m.bit_length() for m in c["q"])) >= 3 for c in ok if _hps(c)), "a mixed chain that decrypts"


# ---- mixed chains ---------------------------------------------------------------------------------------------
def _wider(c):
    return max(c["q"]).bit_length() - c["q"][0].bit_length() >= 8


def _narrower(c):
    return c["q"][0].bit_length() - min(c["q"]).bit_length() >= 8


def _told_apart(c, q_ref, rederive=True):
    """coefficients of the case's own scale-round input on which tables derived from q_ref give another output"""
    k = C.sweep_inputs(c)
    W = D.tables_by_tower(k["T"], q_ref, rederive)
    assert (W.branch, W.q_msb_hf) != (k["T"].branch, k["T"].q_msb_hf)
    with np.errstate(over="ignore"):
        other = D._finish(D.float_chain(k["x"], W), D.int_sum(k["x"], W), W, check=False)
    return int((other != D.scale_round(k["x"], k["T"])).sum())


def test_mixed_chains_reach_the_wide_and_narrow_towers():
    """Sensitivity: on the pinned chains' own inputs, tables re-derived with qMSB from the widest (narrowest) tower
    instead of q[0] give another output, so a kernel that branched or split on the wrong tower fails the GPU test.
    All eight loops compute the same sum, so re-derived tables differ from the reference's only where one of the two
    loses precision: a split point moved consistently (shift and B tables) between two split loops is the same
    sum up to rounding ties.  The split case is therefore told apart by the kernel-side mistake: the shift from
    the widest tower, the B tables the caller's."""
    cs = [c for c in _cases() if _hps(c)]
    pinned = lambda c: "bits" in C.PINS.get(c["seed"], {})  # noqa: E731
    flat, split = [], []
    for c in cs:
        if not _wider(c):
            continue
        k = C.sweep_inputs(c)
        T, x = k["T"], k["x"]
        if not T.split and (x >= U64(1 << 53)).any():
            flat.append(c)  # u2d rounds its input, lo * w wraps
        if T.split and (x >> U64(T.q_msb_hf) >= U64(1 << 31)).any():
            split.append(c)
    narrow = [c for c in cs if _narrower(c)]
    assert any(map(pinned, flat)) and any(map(pinned, split)) and any(map(pinned, narrow))
    assert {BT.DecryptTables(c["q"], c["t"]).branch < 4 for c in flat if pinned(c)} == {True, False}, "A-B and E-F"
    for c in filter(pinned, flat):
        assert _told_apart(c, max(c["q"])) >= 1, c["seed"]
    for c in filter(pinned, split):
        assert _told_apart(c, max(c["q"]), rederive=False) >= 1, c["seed"]
    for c in filter(pinned, narrow):
        if c["q"][0] == max(c["q"]):
            assert _told_apart(c, min(c["q"])) >= 1, c["seed"]
    assert any(c["q"][0] == max(c["q"]) for c in narrow if pinned(c))
    print(f"wide towers behind q[0]: {len(flat)} cases not split, {len(split)} split; {len(narrow)} with narrow towers")


# ---- LARGE_T --------------------------------------------------------------------------------------------------
# the entries in which the bounded search found planted coefficients that tell a fused chain from the reference's
# before this test was written; the others report (in H the integer sum of 55 bits and more swamps the chain)
FUSED_SENSITIVE = {"F-2^46-21-40x255"}


@pytest.mark.parametrize("name", list(C.LARGE_T))
def test_large_t(name):
    k = C.large_t_case(name)
    T, x = k["T"], k["x"]
    technique, t, _, towers, _, _ = C.LARGE_T[name]
    assert 2 * len(T.q) * t < 1 << 64 and len(T.q) == towers <= 255 and all(m & 1 and 3 <= m < 1 << 60 for m in T.q)
    assert (x < np.array(T.q, dtype=U64)[None, :, None]).all()
    assert k["replaced"] < 0.01 * x.shape[0] * x.shape[2], "share of inputs with an undefined final cast"
    if technique == "BFV_BEHZ":
        assert t < 1 << 32 and t >= (1 << 32) - 5
        want = D.scale_round_behz(x, T)
        assert (want <= U64(t)).all()
        if "narrow" in name:
            assert all(T.tgamma > m for m in T.q)
        for ri in range(4):  # the loop with Python integers
            s = 0
            for i, m in enumerate(T.q):
                y = int(x[1, i, ri]) * T.tgammaQHatInvModq[i] % m
                s = (s + y * T.negInvqModtgamma[i] % T.tgamma) % T.tgamma
            assert (s + (s & ((1 << 26) - 1))) >> 26 == int(want[1, ri])
        return
    assert BT.BRANCHES[T.branch] == name[0] and name[0] in "FH"
    assert D.defined(x, T).all()
    want = D.scale_round(x, T)
    assert (want <= U64(t)).all()
    acc = D.int_sum(x, T)
    assert (acc >= U64(1 << 53)).any(), "u2d(intSum) never rounds"
    if towers == 255 and name[0] == "H":
        assert (acc >= U64(1 << 63)).any()
    flat = x.transpose(0, 2, 1).reshape(-1, towers)
    for p in list(k["planted"][:4]) + [0, 1]:
        assert D.scale_round_scalar([int(v) for v in flat[p]], T) == int(want.reshape(-1)[p]), (name, p)
    # reported; asserted only where the bounded search finds any, as test_fused_chain_differs does
    pool = min(len(k["planted"]), 64 if towers <= 33 else 8)
    hits = sum(D.fused_differs([int(v) for v in flat[p]], T) for p in k["planted"][:pool])
    if name in FUSED_SENSITIVE:
        assert hits >= 1, name
    print(f"{name}: fused differs on {hits} of the first {pool} planted coefficients; intSum up to "
          f"{int(acc.max()).bit_length()} bits; {k['replaced']} inputs replaced")


def test_large_t_covers_what_it_lists():
    h = [v for n, v in C.LARGE_T.items() if n[0] == "H"]
    assert {(v[1], v[2], v[3]) for v in h} == {((1 << 55) + 3, 60, 33), ((1 << 50) + 5, 55, 17),
                                               ((1 << 56) - 5, 60, 100), ((1 << 55) + 3, 60, 255)}
    assert sum(n[0] == "F" for n in C.LARGE_T) >= 1
    b = {(v[1], v[2]) for v in C.LARGE_T.values() if v[0] == "BFV_BEHZ" and isinstance(v[2], int)}
    assert b == {((1 << 32) - 1, 60), ((1 << 32) - 5, 60)}
    assert any(isinstance(v[2], list) and max(v[2]) <= 30 and min(v[2]) == 22 for v in C.LARGE_T.values())


# ---- EQUALS_T -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", C.EQUALS_T, ids=[D.case_id(c) for c in C.EQUALS_T])
def test_equals_t(c):
    technique, letter, t, bits, towers = c
    k = C.equals_t_case(c)
    T, x = k["T"], k["x"]
    lift = BR.crt_lift(x[:1, :, :C.EQUALS_E], T.q)[0]
    if k["replaced"] == 0:
        assert [int(v) for v in lift] == [T.Q - e for e in range(1, C.EQUALS_E + 1)]
    assert k["replaced"] < 0.01 * x.shape[0] * x.shape[2]
    if technique == "BFV_BEHZ":
        want = D.scale_round_behz(x, T)
        assert (want == U64(t)).any(), "BEHZ writes t for a zero plaintext under negative noise"
    else:
        assert BT.BRANCHES[T.branch] == letter
        want = D.scale_round(x, T)
        if (letter, t, bits, towers) in (("F", 5308417, 30, 5), ("H", 5308417, 55, 2)):
            assert (want == U64(t)).any(), c
    assert (want <= U64(t)).all()
    print(f"{D.case_id(c)}: {int((want == U64(t)).sum())} of {want.size} outputs equal t, {k['replaced']} replaced")


def test_equals_t_covers_the_table():
    assert {(c[1], c[2], c[3]) for c in C.EQUALS_T if c[0] == "BFV_HPS"} == \
        {r for r in D.BRANCH_TABLE if r[0] in "EFGH"}
    assert {(c[1], c[2], c[3]) for c in C.EQUALS_T if c[0] == "BFV_BEHZ"} == set(D.BRANCH_TABLE)
    assert all(t < 1 << 32 for _, t, _ in D.BRANCH_TABLE)
    assert ("BFV_HPS", "F", 5308417, 30, 5) in C.EQUALS_T and ("BFV_HPS", "H", 5308417, 55, 2) in C.EQUALS_T


# ---- ONE_TOWER_WIDE -------------------------------------------------------------------------------------------
def test_one_tower_wide():
    assert [(q, t) for q, t in C.ONE_TOWER_WIDE if q] == [(17, 5), (17, 9), (17, 16), (17, 19), (97, 65537),
                                                          (4194217, (1 << 31) - 1)]
    assert C.ONE_TOWER_WIDE[-1] == (None, (1 << 61) - 1)
    paths = set()
    for c in C.ONE_TOWER_WIDE:
        k = C.one_tower_wide_case(c)
        q, t, x = k["T"].q[0], k["T"].t, k["x"]
        assert q & 1 and 3 <= q < 1 << 60 and 2 * t < 1 << 64 and (x < U64(q)).all()
        if q <= 256:
            assert set(int(v) for v in x[0, 0]) == set(range(q)), "every residue"
        else:
            assert q.bit_length() == 60 or c[0] == q
            assert [int(v) for v in x[0, 0, :5]] == [0, 1, q >> 1, (q >> 1) + 1, q - 1]
        want = D.one_tower(x, q, t)
        mine = set()
        for v, w in zip(x.reshape(-1), want.reshape(-1)):  # the scalar restatement agrees word for word
            r, path = D.one_tower_scalar(int(v), q, t)
            assert r == int(w), (c, int(v))
            mine |= path
        assert {"upper", "lower"} <= mine, c
        paths |= mine
    assert paths == {"upper", "lower", "wrapped", "reduced", "up", "small", "down"}, paths


# ---- TimesQovert ----------------------------------------------------------------------------------------------
def test_tqt_lists_what_it_must():
    bits = lambda name: sorted(m.bit_length() for m in C.tqt_case(name)["T"].q)  # noqa: E731
    assert C.TQT["t2-60x3"][0] == 2 and bits("t2-60x3") == [60, 60, 60]
    assert C.TQT["t2^31-mixed"][0] == 1 << 31 and bits("t2^31-mixed")[0] == 22 and bits("t2^31-mixed")[-1] == 60
    q = C.tqt_case("t65537-above-q")["T"].q
    assert q[:2] == [17, 97] and q[2].bit_length() == 22 and C.TQT["t65537-above-q"][0] == 65537 > q[1]
    assert C.TQT["tP55-60x2"][0] == C.P55 and bits("tP55-60x2") == [60, 60]
    assert C.TQT["t2^62-60x2"][0] == 1 << 62 and bits("t2^62-60x2") == [60, 60]
    # create admits 2 size_q t < 2^64: exactly the refused entries miss it
    for name in C.TQT:
        T = C.tqt_case(name)["T"]
        assert (2 * len(T.q) * T.t >= 1 << 64) == (name in C.TQT_REFUSED), name
    assert C.TQT["t2^61-60x2"] == (1 << 61, [60, 60]) and C.TQT["t2^62-60x1"] == (1 << 62, [60])


@pytest.mark.parametrize("name", list(C.TQT))
def test_tqt(name):
    k = C.tqt_case(name)
    T, x, n = k["T"], k["x"], k["n"]
    t = T.t
    for i, m in enumerate(T.q):
        assert [int(v) for v in x[0, i, :7]] == [0, t - 1, t, m - 1, m, 1 << 63, (1 << 64) - 1]
    assert (x[0] >= U64(1 << 63)).any() and (x[0, :, 7:] >= np.array(T.q, dtype=U64)[:, None]).any()
    out = D.times_q_over_t(x, T)
    assert (out < np.array(T.q, dtype=U64)[None, :, None]).all()
    # exact integers: the output depends on x mod t alone
    nqt = T.negQModt % t
    big = False
    for i, m in enumerate(T.q):
        for b in range(k["batch"]):
            for ri in range(n):
                v = int(x[b, i, ri])
                y = (v % t) * nqt % t
                big |= y >= m
                assert int(out[b, i, ri]) == y * T.tInvModq[i] % m, (name, b, i, ri)
    reduced = D.times_q_over_t(x % U64(t), T)
    assert np.array_equal(out, reduced)
    if any(t > m for m in T.q):
        assert big, "no intermediate y at or above q_i"
    if all(t <= m for m in T.q):
        # the CRT lift on m < t is (Q m + r) / t with r = -Q m mod t: the integer next to Q m / t
        msg = [int(v) for v in x[1, 0, :n // 2]]
        assert all(v < t for v in msg) and (x[1, :, :n // 2] == x[1, :1, :n // 2]).all()
        lift = BR.crt_lift(out[1:, :, :n // 2], T.q)[0]
        for mi, v in zip(msg, lift):
            r = -T.Q * mi % t
            assert (T.Q * mi + r) % t == 0 and int(v) == (T.Q * mi + r) // t % T.Q
    else:
        assert any(t > m for m in T.q)
