"""CPU: the committed seed ranges of tests/test_gpu_fuzz_tier3.py reach what
that fuzz exists for.  A condition on the generator (tests/tier3_cases.py),
not a measurement: if a change to the draws loses one of these, pin a seed in
tier3_cases.PINS rather than relax the count."""
from collections import Counter
from functools import lru_cache

import keyswitch as K
import tier2_cases as C2
import tier3_cases as C
from test_tier2_cases import _at_least_twice, _log_n_class

CLASSES = ("<12", "12", "13-15", "16", "17")
CAP = C.KS_ROT_CAP


@lru_cache(maxsize=None)
def _cases(kind):
    return [C.case(kind, seed) for seed in range(C.SEEDS[kind])]


def test_seed_ranges_and_shared_helpers():
    assert C.SEEDS == {"rotation": 48, "bfv_mult": 40, "scale_round": 32, "switch_exact": 32}
    assert C.SCALE is C2.SCALE and not set(C.BASE.values()) & set(C2.BASE.values())
    for name in ("_moduli", "_log_n", "_plan_options", "valid_splits", "valid_dnums", "keyswitch_draw"):
        assert not hasattr(C, name), name + " is tier2_cases' own, not copied"


def test_draws_are_deterministic_and_valid():
    for kind in C.SEEDS:
        for seed, c in enumerate(_cases(kind)):
            assert c["seed"] == seed and c["kind"] == kind and c == C.case(kind, seed)
            m = 2 << c["log_n"]
            mods = c["q"] + c.get("p", []) + c.get("r", [])
            assert len(set(mods)) == len(mods) and all(q % m == 1 and 3 <= q < 1 << 60 for q in mods)
            assert 1 <= c["batch"] <= 4
            if kind == "rotation":
                assert 4 <= c["log_n"] <= 17 and all(q.bit_length() >= 30 for q in mods)
                assert c["split"] in C2.valid_splits(c["log_n"]) and c["dnum"] in C2.valid_dnums(c["size_q"])
                kp = K.KeySwitchParams(1 << c["log_n"], c["q"], c["rq"], c["p"], c["rp"], c["dnum"])
                assert kp.beta(c["level"]) == c["beta"] and 1 <= c["nrot"] <= 2 * CAP + 1
                assert 0 <= c["column"] < 1 << c["log_n"]
            else:
                assert 1 <= c["log_n"] <= 17 and all(q.bit_length() >= max(22, c["log_n"] + 4) for q in mods)
            if kind == "bfv_mult":
                assert 1 <= c["size_q"] <= 6 and c["size_r"] - c["size_q"] in (0, 1)
                assert c["technique"] == C.HPS or c["size_r"] == c["size_q"]
                assert (c["kernels"]["q_to_r_neg"] is None) == (c["technique"] == C.HPS)
                for split, generic in c["plans"].values():
                    assert split in C2.valid_splits(c["log_n"]) and generic in (0, 1)
            if kind == "scale_round":
                assert 1 <= c["size_i"] <= 20 and 1 <= c["size_o"] <= 20
                assert (len(c["p"]), len(c["q"])) == ((c["size_i"], c["size_o"]) if c["out_is_q"]
                                                      else (c["size_o"], c["size_i"]))
            if kind == "switch_exact":
                assert c["kernel"] != "BCONV_KERNEL_LIMB" or c["size_q"] <= 16


def test_rotation_coverage():
    cs = _cases("rotation")
    _at_least_twice(Counter(_log_n_class(c["log_n"]) for c in cs), CLASSES, "ring size class")
    for log_n in (16, 17):
        _at_least_twice(Counter(c["split"] for c in cs if c["log_n"] == log_n), C2.valid_splits(log_n),
                        f"split at 2^{log_n}")
    _at_least_twice(Counter(c["generic_moduli"] for c in cs), (0, 1), "generic_moduli")
    _at_least_twice(Counter(min(c["beta"], 5) for c in cs), (1, 2, 3, 4, 5), "beta (5 = five or more)")
    _at_least_twice(Counter(c["add_first"] for c in cs), (True, False), "addFirst")
    _at_least_twice(Counter(c["t"] for c in cs), (0, 65537), "t")
    # the third launch of a call (r0 = 2 CAP), by the narrow and by the wide inner product, on a small ring
    third = [c for c in cs if c["nrot"] > 2 * CAP and c["log_n"] <= 6]
    assert {c["beta"] >= 5 for c in third} == {True, False}
    assert len([c for c in cs if CAP < c["nrot"] <= 2 * CAP]) >= 2, "a ragged second launch"
    _at_least_twice(Counter(c["nrot"] == 1 for c in cs), (True,), "one rotation")
    # the digits of ModUp on the device, with the options that change how it runs
    pre = [c for c in cs if c["from_precompute"]]
    _at_least_twice(Counter(c["from_precompute"] for c in cs), (True, False), "digits from precompute")
    ragged = [c for c in pre if 0 < c["chunk"] < c["batch"] and c["batch"] % c["chunk"]]
    assert len(ragged) >= 2, "precompute in chunks with a ragged last chunk"
    for opt in ("single_stream", "separate_cols", "generic_moduli"):
        _at_least_twice(Counter(c[opt] for c in pre), (0, 1), opt + " with digits from precompute")
    # the non-Ext call's ModDown over nrot * batch entries
    _at_least_twice(Counter(c["single_stream"] for c in cs), (0, 1), "single_stream")
    full17 = [c for c in cs if c["log_n"] == 17 and c["level"] == c["size_q"]]
    for opt in ("separate_cols", "separate_icol"):
        _at_least_twice(Counter(c[opt] for c in full17), (0, 1), opt + " at 2^17, full level")
    assert len([c for c in cs if len({q.bit_length() for q in c["q"] + c["p"]}) >= 3]) >= 16, "mixed sizes"


def test_bfv_mult_coverage():
    cs = _cases("bfv_mult")
    _at_least_twice(Counter(_log_n_class(c["log_n"]) for c in cs), CLASSES, "ring size class")
    assert {c["log_n"] for c in cs} == set(range(1, 18))
    _at_least_twice(Counter(c["technique"] for c in cs), (C.HPS, C.HPSPOVERQ), "technique")
    _at_least_twice(Counter(c["size_r"] - c["size_q"] for c in cs if c["technique"] == C.HPS), (0, 1), "HPS: R - Q")
    _at_least_twice(Counter(c["size_q"] for c in cs), range(1, 7), "Q")
    _at_least_twice(Counter(c["batch"] for c in cs), (1, 2, 3), "batch")
    for name in ("q_to_r", "r_to_q", "q_to_r_neg"):
        _at_least_twice(Counter(c["kernels"][name] for c in cs), C.KERNELS, name + " kernel")
    for log_n in (16, 17):
        for plan in ("plan_q", "plan_r", "plan_qr"):
            got = {c["plans"][plan][0] for c in cs if c["log_n"] == log_n}
            assert got >= {"SPLIT_AUTO", "SPLIT_COLS"}, f"{plan} at 2^{log_n}: {got}"
        allp = {c["plans"][p][0] for c in cs if c["log_n"] == log_n for p in c["plans"]}
        assert allp == set(C2.valid_splits(log_n)), f"splits at 2^{log_n}: {allp}"
    for plan in ("plan_q", "plan_r", "plan_qr"):
        _at_least_twice(Counter(c["plans"][plan][1] for c in cs), (0, 1), plan + " generic_moduli")
    assert any(len(set(c["plans"].values())) > 1 for c in cs), "the three plans' options differ somewhere"
    mixed = [c for c in cs if min(m.bit_length() for m in c["q"] + c["r"]) < 32
             and max(m.bit_length() for m in c["q"] + c["r"]) == 60]
    assert len(mixed) >= 2, "a tower below 32 bits and one of 60 in one chain"
    _at_least_twice(Counter(c["eval_form"] for c in cs), (True, False), "ExpandCRTBasis form")


def test_scale_round_coverage():
    cs = _cases("scale_round")
    _at_least_twice(Counter(c["size_o"] % 4 for c in cs), (0, 1, 2, 3), "size_o mod 4")
    _at_least_twice(Counter(c["out_is_q"] for c in cs), (True, False), "out_is_q")
    _at_least_twice(Counter(c["size_i"] > 16 for c in cs), (True, False), "more than 16 summed towers")
    _at_least_twice(Counter(c["size_i"] == 1 or c["size_o"] == 1 for c in cs), (True,), "a single tower")
    _at_least_twice(Counter(c["log_n"] < 8 for c in cs), (True, False), "below one block")
    narrow = [c for c in cs if min(m.bit_length() for m in (c["q"] if c["out_is_q"] else c["p"])) < 32]
    assert len(narrow) >= 4, "an output modulus below 32 bits"


def test_switch_exact_coverage():
    cs = _cases("switch_exact")
    _at_least_twice(Counter(c["kernel"] for c in cs), C.KERNELS, "kernel")
    auto = [c for c in cs if c["kernel"] == "BCONV_KERNEL_AUTO"]
    mma = [c for c in auto if c["log_n"] >= 5 and c["size_q"] <= 64]
    _at_least_twice(Counter(c["ks"] > 8 for c in mma), (True, False), "matrix-core kernel: WIDE combine")
    _at_least_twice(Counter(c["spq"] for c in mma), (True, False), "matrix-core kernel: special-prime reduction")
    assert len({c["ks"] for c in mma}) >= 6, "K-step counts"
    assert any(c["chunks"] > 1 for c in mma), "a second target chunk"
    assert any(c["log_n"] < 5 for c in auto) and any(c["size_q"] > 64 for c in auto), "AUTO off the matrix cores"
    assert {c["log_n"] for c in cs} >= set(range(1, 11))
