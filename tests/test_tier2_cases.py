"""CPU: the committed seed ranges of tests/test_gpu_fuzz_tier2.py reach what
that fuzz exists for.  A condition on the generator (tests/tier2_cases.py),
not a measurement: if a change to the draws loses one of these, pin a seed in
tier2_cases.PINS rather than relax the count."""
from collections import Counter
from functools import lru_cache

import keyswitch as K
import tier2_cases as C


@lru_cache(maxsize=None)
def _cases(kind):
    return [C.case(kind, seed) for seed in range(C.SEEDS[kind])]


def _log_n_class(log_n):
    return "<12" if log_n < 12 else "12" if log_n == 12 else "13-15" if log_n <= 15 else str(log_n)


def _at_least_twice(counter, keys, what):
    for k in keys:
        assert counter[k] >= 2, f"{what}: {k!r} drawn {counter[k]} times"


def test_seed_ranges():
    assert C.SEEDS == {"rescale": 48, "bv": 32, "keyswitch": 64}


def test_draws_are_deterministic_valid_and_never_skipped():
    for kind in C.SEEDS:
        for seed, c in enumerate(_cases(kind)):
            assert c is not None and c["seed"] == seed and c == C.case(kind, seed)
            m = 2 << c["log_n"]
            mods = c["q"] + c.get("p", [])
            assert len(set(mods)) == len(mods) and all(q % m == 1 and 3 <= q < 1 << 60 for q in mods)
            assert c["split"] in C.valid_splits(c["log_n"]) and c["generic_moduli"] in (0, 1)
            if kind == "keyswitch":
                assert 4 <= c["log_n"] <= 17 and 1 <= c["size_p"] <= 6 and 1 <= c["batch"] <= 4
                assert 1 <= c["size_q"] <= (6 if c["log_n"] >= 15 else 12) and 1 <= c["level"] <= c["size_q"]
                assert all(q.bit_length() >= 30 for q in mods)
                kp = K.KeySwitchParams(1 << c["log_n"], c["q"], c["rq"], c["p"], c["rp"], c["dnum"])  # accepts dnum
                assert kp.beta(c["level"]) == c["beta"]
                assert c["chunk"] in (0, 1, 2, c["batch"], c["batch"] + 1)
            else:
                assert 1 <= c["log_n"] <= 17 and c["towers"] <= c["plan_towers"] == len(c["q"])
                assert all(q.bit_length() >= max(22, c["log_n"] + 4) for q in mods)
                if kind == "rescale":
                    assert 2 <= c["towers"] and c["plan_towers"] <= (4 if c["log_n"] >= 15 else 8)
                    assert 1 <= c["batch"] <= 3 and (c["t"] % 2 == 1 or c["t"] == 2)
                    assert c["t"] < min(c["q"])  # invertible modulo the dropped tower
                else:
                    assert 1 <= c["towers"] <= 5 and 1 <= c["batch"] <= 2


def test_rescale_and_bv_coverage():
    for kind in ("rescale", "bv"):
        cs = _cases(kind)
        _at_least_twice(Counter(r for c in cs for r in c["regimes"]), ("up", "down_small", "down_big"),
                        kind + " switch regime")
        _at_least_twice(Counter(_log_n_class(c["log_n"]) for c in cs), ("<12", "12", "13-15", "16", "17"),
                        kind + " ring size class")
        _at_least_twice(Counter(c["generic_moduli"] for c in cs), (0, 1), kind + " generic_moduli")
        for log_n in (16, 17):
            _at_least_twice(Counter(c["split"] for c in cs if c["log_n"] == log_n), C.valid_splits(log_n),
                            f"{kind} split at 2^{log_n}")
    cs = _cases("rescale")
    _at_least_twice(Counter(c["op"] for c in cs), ("drop_last", "mod_reduce"), "rescale op")
    _at_least_twice(Counter(c["eval_form"] for c in cs), (True, False), "rescale form")
    _at_least_twice(Counter(c["in_place"] for c in cs), (True, False), "rescale in place")
    _at_least_twice(Counter(c["towers"] < c["plan_towers"] for c in cs), (True, False), "rescale lower level")
    _at_least_twice(Counter(c["towers"] < c["plan_towers"] for c in _cases("bv")), (True, False), "bv key towers")


def test_keyswitch_coverage():
    cs = _cases("keyswitch")
    _at_least_twice(Counter(_log_n_class(c["log_n"]) for c in cs), ("<12", "12", "13-15", "16", "17"),
                    "ring size class")
    for log_n in (16, 17):
        _at_least_twice(Counter(c["split"] for c in cs if c["log_n"] == log_n), C.valid_splits(log_n),
                        f"split at 2^{log_n}")
    _at_least_twice(Counter(c["generic_moduli"] for c in cs), (0, 1), "generic_moduli")
    _at_least_twice(Counter(min(c["beta"], 5) for c in cs), (1, 2, 3, 4, 5), "beta (5 = five or more)")
    _at_least_twice(Counter(c["level"] < c["size_q"] for c in cs), (True,), "level < size_q")
    _at_least_twice(Counter(c["t"] > 0 for c in cs), (True, False), "t > 0")
    ragged = [c for c in cs if 0 < c["chunk"] < c["batch"] and c["batch"] % c["chunk"]]
    assert len(ragged) >= 2, "chunk with a ragged last chunk"
    _at_least_twice(Counter(c["single_stream"] for c in cs), (0, 1), "single_stream")
    full17 = [c for c in cs if c["log_n"] == 17 and c["level"] == c["size_q"]]
    for opt in ("separate_cols", "separate_icol"):
        _at_least_twice(Counter(c[opt] for c in full17), (0, 1), opt + " at 2^17, full level")
