"""CPU: the directed cases, the committed seed range and the grid of
tests/test_gpu_fuzz_linear_transform.py reach what that file exists for.  Conditions on the case
data (tests/linear_transform_cases.py), not measurements: if a change to the draws loses one of
these, pin a seed in linear_transform_cases.PINS rather than relax the count.

The sensitivity tests build the directed cases' very inputs (the GPU file's Bsgs with the upload
replaced by the identity) and compute the reference twice."""
import os
from collections import Counter
from functools import lru_cache

import numpy as np
import pytest

import keyswitch as K
import linear_transform_cases as C
import test_gpu_linear_transform as T
import tier2_cases as C2
from test_tier2_cases import _at_least_twice

CAP = C.KS_ROT_CAP


@lru_cache(maxsize=None)
def _draws():
    return [C.case(seed) for seed in range(C.SEEDS)]


def _plan(c):
    n = 1 << c["log_n"]
    beta = c["beta"] if "beta" in c else C.params_of(c).beta(c["level"])
    return C.launch_plan(c["baby"], c["giant"], n, beta)


def _all_plans():
    return [_plan(c) for c in C.DIRECTED + _draws()]


def test_seed_range_and_shared_helpers():
    assert C.SEEDS == 48 and C.SCALE is C2.SCALE
    assert C.BASE not in C2.BASE.values() and (C.KS_ROT_CAP, C.LT_SUM_CAP, C.LT_TERM_CAP) == (16, 16, 16)
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "upmem--openfhe_amd", "csrc",
                            "lt_kernels.hpp")).read()
    assert "LT_SUM_CAP = 16;" in src and "LT_TERM_CAP = 16;" in src, "the caps launch_plan restates"
    for name in ("_moduli", "_log_n", "_plan_options", "valid_splits", "valid_dnums", "keyswitch_draw", "mixed_chain"):
        assert not hasattr(C, name), name + " is shared, not copied"


def test_launch_plan_on_the_shipped_shapes():
    """launch_plan against launches counted by hand from csrc/keyswitch.hip"""
    n = 8
    k = T.nonid(n, 0)
    p = C.launch_plan([1] + [k] * 16, [1, k], n, 2)  # the shipped 17-baby case: one full run
    assert p["baby_runs"] == [(1, 16)] and p["term_chunks"] == 2 and (p["nrot"], p["nid"]) == (1, 1)
    assert p["inner_rot"] == [(0, 0), (0, 16)] and p["outer"] == [1] and p["first"] == 1 and not p["mid_set_reduction"]
    p = C.launch_plan([1, k], [k] * 17, n, 2)  # the shipped cap + 1 giants
    assert p["outer"] == [16, 1] and p["first"] == 2 and p["sum_chunks_rot"] == 2 and p["sum_chunks_id"] == 0
    assert p["inner_rot"] == [(0, 0), (16, 0)] and p["inner_id"] == [] and p["mod_down_polys"] == 2
    p = C.launch_plan([1], [1, 2 * n + 1], n, 3)  # identities only: one empty outer launch carries the addends
    assert p["outer"] == [0] and p["first"] == 1 and p["baby_runs"] == [] and p["mod_down_polys"] == 4
    assert C.launch_plan([1], [k] * 6, n, 3)["mid_set_reduction"]      # the shipped extreme test: 6 sets x 3
    assert not C.launch_plan([1], [k] * 3, n, 5)["mid_set_reduction"]  # 15 products: no reduction before the end
    assert C.launch_plan([1], [k] * 4, n, 5)["mid_set_reduction"]      # the 16th product: first digit of set 4
    assert not C.launch_plan([1], [k] * 33, n, 1)["mid_set_reduction"]


def test_draws_are_deterministic_and_valid():
    for seed, c in enumerate(_draws()):
        assert c["seed"] == seed and c["kind"] == "linear_transform" and c == C.case(seed)
        n, m = 1 << c["log_n"], 2 << c["log_n"]
        mods = c["q"] + c["p"]
        assert len(set(mods)) == len(mods) and all(q % m == 1 and 3 <= q < 1 << 60 for q in mods)
        assert 4 <= c["log_n"] <= 17 and all(q.bit_length() >= max(22, c["log_n"] + 4) for q in mods)
        assert c["split"] in C2.valid_splits(c["log_n"]) and c["dnum"] in C2.valid_dnums(c["size_q"])
        kp = K.KeySwitchParams(n, c["q"], c["rq"], c["p"], c["rp"], c["dnum"])  # accepts dnum
        assert kp.beta(c["level"]) == c["beta"] and 1 <= c["level"] <= c["size_q"]
        assert 1 <= c["batch"] <= 3 and 1 <= len(c["baby"]) <= 20 and 1 <= len(c["giant"]) <= 20
        assert all(k % 2 == 1 and 0 < k < 1 << 32 for k in c["baby"] + c["giant"])
        assert c["t"] < min(mods) and (c["t"] == 0 or c["t"] % 2 == 1)
        nd = len(c["baby"]) * len(c["giant"])
        assert c["present"] is None or len(c["present"]) == nd
        towers = c["level"] + c["size_p"]
        assert max(nd, len(c["baby"]) * c["batch"]) * towers * n <= C.LT_WORDS or (nd == 1 and c["batch"] == 1)
        if not c["unreduced"]:
            assert all(k < m for k in c["baby"] + c["giant"])


def test_launch_chunking_is_reached():
    plans = _all_plans()
    assert any(CAP in [m for _, m in p["baby_runs"]] and len(p["baby_runs"]) >= 2 for p in plans), "a run split"
    assert any(len(p["baby_runs"]) >= 3 for p in plans), "three baby runs"
    # the second call of a split run starts at baby i >= 16 (r0 + i * per)
    assert any(i >= CAP for p in plans for i, _ in p["baby_runs"])
    assert any(p["term_chunks"] >= 3 for p in plans), "three term chunks (i0 = 32)"
    assert any(p["sum_chunks_rot"] >= 2 for p in plans) and any(p["sum_chunks_id"] >= 2 for p in plans)
    assert any(p["nid"] > CAP for p in plans), "more than 16 addends and 2 + nid > 18 ModDown polynomials"
    assert any(len(p["outer"]) >= 3 and p["first"] >= 3 for p in plans), "three outer and first launches (j0 = 32)"
    # g0 != 0 and i0 != 0 in one launch: in the fused call and in the stage call
    fused = any(g0 and i0 for p in plans for g0, i0 in p["inner_rot"] + p["inner_id"])
    stage = any(nterm > C.LT_TERM_CAP and nsum > C.LT_SUM_CAP for nterm, nsum in C.STAGE_SUMS)
    assert fused and stage
    assert stage and any(nsum > 2 * C.LT_SUM_CAP for _, nsum in C.STAGE_SUMS), "three sum chunks of the stage call"
    assert any(nterm > 2 * C.LT_TERM_CAP for nterm, _ in C.STAGE_SUMS)


def test_stage_present_has_empty_chunks():
    """some sum lacks its whole first chunk (the first launch stores zeros), some a later one (an acc
    launch adds nothing), some every diagonal, and some none of its chunks"""
    for nterm, nsum in C.STAGE_SUMS:
        pr = C.stage_present(nterm, nsum)
        assert len(pr) == nterm * nsum
        chunks = -(-nterm // C.LT_TERM_CAP)
        empty = [[not any(pr[j * nterm + i] for i in range(c * 16, min(nterm, c * 16 + 16))) for c in range(chunks)]
                 for j in range(nsum)]
        assert any(e[0] and not all(e) for e in empty) or chunks == 1
        assert any(all(e) for e in empty[:16]) and any(not any(e) for e in empty)
        if chunks > 1:
            assert any(e[-1] and not e[0] for e in empty)
        if nsum > C.LT_SUM_CAP:
            assert any(any(e) for e in empty[16:]), "an empty chunk in the second sum chunk"


def test_runtime_beta_reduces_inside_a_set():
    n = 16
    idx = lambda nset: [T.nonid(n, r) for r in range(nset)]  # noqa: E731
    inside = [(b, s) for b, s in C.EXTREME_SETS if C.launch_plan([1], idx(s), n, b)["mid_set_reduction"]]
    assert {b for b, _ in inside} == {5, 6} and (5, 3) not in inside and (5, 4) in inside and (6, 3) in inside
    for chain in sorted(T.EXTREME_CHAINS):
        q, _, p, _ = T.EXTREME_CHAINS[chain](4)
        for beta, nset in C.EXTREME_SETS:
            mods = q[:beta] + p
            # nset * beta products of (m - 1)^2 = 1: the expected word of the all-top case
            assert all((nset * beta * (m - 1) ** 2) % m == (nset * beta) % m for m in mods)
            if chain == "60-bit" and (beta, nset) in inside:
                # a kernel that reduced only at the set's end would have summed this past 64 bits
                assert C.top_limb_sum(mods, C.products_to_set_end(beta)) >= 1 << 64
                assert C.top_limb_sum(mods, 16) < 1 << 64
    # the fused call reaches it too
    c = C.FUSED_BETA5
    assert C.params_of(c).beta(c["level"]) == 5 and _plan(c)["mid_set_reduction"] and _plan(c)["nrot"] == 4


def test_sweep_structure():
    cs = _draws()
    plans = [_plan(c) for c in cs]
    groups = {
        "nrot = 0": [p["nrot"] == 0 for p in plans],
        "nid = 0": [p["nid"] == 0 for p in plans],
        "nrot and nid nonzero": [p["nrot"] > 0 and p["nid"] > 0 for p in plans],
        "a giant with no diagonal present": [
            c["present"] is not None and any(not any(c["present"][j * len(c["baby"]):(j + 1) * len(c["baby"])])
                                             for j in range(len(c["giant"]))) for c in cs],
        "level below Q": [c["level"] < c["size_q"] for c in cs],
        "t != 0": [c["t"] != 0 for c in cs],
    }
    for what, hits in groups.items():
        assert sum(hits) >= 6, f"{what}: {sum(hits)} seeds"
    assert {c["log_n"] for c in cs} == set(range(4, 18)), "every ring size"
    for log_n in (16, 17):
        _at_least_twice(Counter(c["split"] for c in cs if c["log_n"] == log_n), C2.valid_splits(log_n),
                        f"split at 2^{log_n}")
    for opt in ("single_stream", "separate_cols", "separate_icol", "generic_moduli"):
        _at_least_twice(Counter(c[opt] for c in cs), (0, 1), opt)
    _at_least_twice(Counter(c["chunk"] > 0 for c in cs), (True, False), "chunk")
    full17 = [c for c in cs if c["log_n"] == 17 and c["level"] == c["size_q"] and _plan(c)["nrot"]]
    for opt in ("separate_cols", "separate_icol"):
        assert any(c[opt] for c in full17), opt + " at 2^17, full level, with a rotated giant"
    _at_least_twice(Counter(c["unreduced"] for c in cs), (True, False), "unreduced indices")
    _at_least_twice(Counter(c["pad"] > 0 for c in cs), (True, False), "diag_stride padding")
    _at_least_twice(Counter(c["batch"] for c in cs), (1, 2, 3), "batch")
    _at_least_twice(Counter(d for c in cs for d in c["density"]), C.DENSITY, "present density")
    _at_least_twice(Counter(c["present"] is None for c in cs), (True,), "present = NULL")
    _at_least_twice(Counter(c["baby_ids"] for c in cs), C.BABY_IDS, "identity babies")
    _at_least_twice(Counter(c["giant_ids"] for c in cs), C.GIANT_IDS, "identity giants")
    _at_least_twice(Counter(min(c["beta"], 5) for c in cs if _plan(c)["nrot"]), (1, 2, 3, 4, 5), "beta with k_lt_outer")


def test_tower_widths():
    def wide_and_narrow(mods):
        bits = [m.bit_length() for m in mods]
        return min(bits) <= 24 and max(bits) >= 59

    assert all(wide_and_narrow(sum(C.chain_of(c)[::2], [])) for c in C.DIRECTED)
    assert sum(wide_and_narrow(c["q"][:c["level"]] + c["p"]) for c in _draws()) >= 2
    for log_n in C.GRID_RINGS:
        q, _, p, _ = C.grid_chain(log_n)
        assert wide_and_narrow(q + p) and wide_and_narrow(q[:3] + p)


def test_grid_covers_every_engine():
    for log_n in C.GRID_RINGS:
        for level in (4, 3):
            got = {(s, g) for ln, lv, s, g, o in C.GRID if (ln, lv) == (log_n, level) and o is None}
            assert got == {(s, g) for s in C2.valid_splits(log_n) for g in (0, 1)}
    assert {(lv, o) for ln, lv, s, g, o in C.GRID if o} == {(lv, o) for lv in (4, 3)
                                                            for o in ("separate_cols", "separate_icol")}
    for log_n in C.GRID_RINGS:
        c = C.grid_case(log_n, 4)
        p = _plan(c)
        assert (p["nrot"], p["nid"], len(p["baby_runs"])) == (1, 1, 1) and c["batch"] == 1 and c["present"].count(0) == 1


@pytest.fixture
def host_bsgs(monkeypatch):
    """Bsgs without a device: the upload is the identity"""
    monkeypatch.setattr(T, "dev", lambda x: x)
    return T.Bsgs


@pytest.mark.parametrize("name", C.CHUNKED)
def test_last_chunk_changes_every_tower(host_bsgs, name):
    """The reference with the last chunk marked absent (the diagonals of the last term chunk, or of
    the last launch's giants) differs from the true one in every tower of both outputs, so a kernel
    that skipped the later chunk could not pass."""
    i = C.CHUNKED.index(name)
    c = C.DIRECTED[i]
    p = _plan(c)
    assert p["term_chunks"] > 1 or max(p["nrot"], p["nid"]) > CAP
    bs = C.build(c, host_bsgs, None, C.directed_seed(i))
    want = C.reference(bs, c["t"])
    short = C.reference(bs, c["t"], absent=c["absent_last"])
    for w, s in zip(want, short):
        assert w.shape == (c["batch"], c["level"], 1 << c["log_n"])
        assert (w != s).any(axis=2).all(), name
    # the reduced indices change nothing for the reference's own composition
    assert all(np.array_equal(a, b) for a, b in zip(want, bs.ref(c["t"])))
