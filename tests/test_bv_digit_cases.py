"""CPU: what the GPU cases of tests/bv_digit_cases.py reach, asserted on their own inputs -- every
SwitchModulus regime by some (window, target) pair, a window above q_i / 2 (lifted as a negative number), a
window of at least q_k (the reduction runs), a tower with one window, a digit count above 256, and a chunking
of at least three chunks with a ragged last one."""
import numpy as np

import bv_digit_cases as C
import bv_digits_ref as R
from test_mixed_moduli_oracle import is_special_prime, mixed_chain, regime


def _reach():
    """For every decomposition: the regimes of its (source, target) pairs and which window events occur."""
    seen = {"regimes": set(), "above_half": [], "at_least_target": [], "one_window": []}
    for q, r, coef in C.all_window_cases():
        for i, w in enumerate(R.windows(q, r)):
            if w == 1:
                seen["one_window"].append((q[i], r))
            for j in range(w):
                win = R.window(coef[:, i], j, r)
                assert int(win.max()) < (1 << r)
                if int(win.max()) > q[i] // 2:
                    seen["above_half"].append((q[i], r, j))
                for k, qk in enumerate(q):
                    seen["regimes"].add(regime(q[i], qk))
                    if k != i and int(win.max()) >= qk:
                        seen["at_least_target"].append((q[i], qk, r, j, regime(q[i], qk)))
    return seen


def test_the_gpu_cases_reach_every_branch():
    seen = _reach()
    assert seen["regimes"] == {"up", "equal", "down_small", "down_big"}
    assert seen["one_window"]
    # a window above q_i / 2 on a tower with several windows (not only the tower itself), and on a prime
    # 2^b - d, where only planted words get there
    assert any(R.windows([qi], r)[0] > 1 for qi, r, _ in seen["above_half"])
    assert any(qi.bit_length() == 30 and (1 << 30) - qi < (1 << 20) for qi, r, _ in seen["above_half"])
    # a window of at least q_k under both reductions
    assert {"down_small", "down_big"} >= {x[4] for x in seen["at_least_target"]} and seen["at_least_target"]
    assert any(x[4] == "down_big" for x in seen["at_least_target"])


def test_planted_words_are_in_the_inputs():
    for a in [C.launch_args(10), (13, 29, "special34", 4), (13, 30, "special30", 5), C.CHUNK_CASE]:
        qa, _, _, coef = C.case_input(*a)
        r = a[1]
        for i, qi in enumerate(qa[:a[3]]):
            words = C.plant_words(qi, r)
            if (1 << r) > qi:   # one window, the tower itself: no all-ones word is a residue
                assert not words and R.windows([qi], r) == [1]
                continue
            assert words and all(w < qi for w in words)
            for b in range(coef.shape[0]):
                assert set(words) <= set(int(x) for x in coef[b, i, 1::2])
            # the top planted word fills its windows: window 0 takes the largest r-bit value
            assert int(R.window(coef[:, i], 0, r).max()) == (1 << r) - 1


def test_forms_are_what_their_names_say():
    for log_n in (10, 12, 13):
        assert all(is_special_prime(q) for q in C.chain_of(log_n, "special34")[0])
        assert [is_special_prime(q) for q in C.chain_of(log_n, "special30")[0]].count(False) == 1
        assert not any(is_special_prime(q) for q in C.chain_of(log_n, "generic")[0])
    assert {c[1] for c in C.DIGIT_SIZES} == {1, 13, 29, 30}
    assert {c[0] for c in C.DIGIT_SIZES} == {10, 12, 13}
    assert {c[3] for c in C.DIGIT_SIZES} == {4, 5}  # the top level and one level down on five-tower keys


def test_digit_counts_and_chunkings():
    q, _ = mixed_chain(C.MANY_LOG_N, C.MANY_BITS)
    assert R.digit_count(q, 1) == 298 > 256
    for log_n in (16, 17):
        qa, _, _, _ = C.case_input(*C.launch_args(log_n))
        assert [x.bit_length() for x in qa] == [60, 30] and R.digit_count(qa, C.LAUNCH_R) == 5
    log_n, r, form, T = C.CHUNK_CASE
    n = R.digit_count(C.chain_of(log_n, form)[0][:T], r)
    assert C.chunkings(n) == [0, 1, 2, n - 1, n, n + 5]
    spans = C.chunk_spans(n, 2)
    assert len(spans) >= 3 and spans[-1][1] - spans[-1][0] < 2 and spans[-1][1] == n   # ragged last chunk
    assert len(C.chunk_spans(n, n - 1)) == 2 and len(C.chunk_spans(n, n + 5)) == 1
    # a chunk boundary falls inside a tower's windows and on a tower boundary
    starts = np.cumsum([0] + R.windows(C.chain_of(log_n, form)[0][:T], r))
    cuts = {s[0] for c in (1, 2, n - 1) for s in C.chunk_spans(n, c)}
    assert cuts & set(int(x) for x in starts[1:-1]) and cuts - set(int(x) for x in starts)
