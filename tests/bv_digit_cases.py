"""The cases tests/test_gpu_bv_digits.py runs on the device, with their inputs and
the restatement's outputs (tests/bv_digits_ref.py).  tests/test_bv_digit_cases.py
asserts on the CPU what they reach.

Inputs are built in coefficient form and transformed, so that the words the
device's INTT hands to the window extraction are known: every tower carries
the boundary words of test_mixed_moduli_oracle.with_boundaries in its even
coefficients and, in its first odd ones, the planted words of plant_words --
all-ones windows, which uniform draws do not reach on primes just below a
power of two (a window above q_i / 2, or at least q_k, lies in a gap about
d / 2 wide there)."""
from functools import lru_cache

import numpy as np

import bv_digits_ref as R
import keyswitch as K
from test_mixed_moduli_oracle import bv_chain, mixed_chain, uniform, with_boundaries

# name -> (truly generic chain, bits of the small tower, plan option generic_moduli)
FORMS = {"special30": (False, 30, False), "special34": (False, 34, False), "special34-forced": (False, 34, True),
         "generic": (True, 30, False)}

# Launch paths: (log_n, plan split).  Below 2^16 the chain is bv_chain (60 / 59 / 59 / 30 bits + a 45-bit key
# tower), batch 2, four of the plan's five towers on five-tower keys; at 2^16 and 2^17 two towers (60 and 30
# bits), batch 1.  r = 20 throughout (at 2^16 / 2^17: 3 + 2 = 5 digits).
LAUNCH_PATHS = [(10, "SPLIT_AUTO"), (12, "SPLIT_AUTO"), (13, "SPLIT_AUTO"), (16, "SPLIT_AUTO"), (16, "SPLIT_COLS"),
                (17, "SPLIT_AUTO"), (17, "SPLIT_9_8")]
LAUNCH_R = 20
# Digit sizes on bv_chain: (log_n, r, form, towers used of the plan's five)
DIGIT_SIZES = [(10, 1, "special34", 4), (10, 1, "special34-forced", 4), (12, 13, "special34", 5),
               (12, 13, "special34-forced", 5), (13, 29, "special34", 4), (13, 29, "special34-forced", 4),
               (12, 30, "special34", 5), (12, 30, "special34-forced", 4), (13, 30, "special30", 5),
               (10, 29, "special30", 4), (13, 13, "generic", 4), (10, 30, "generic", 5)]
# Every chunking of the one-call key switch: bv_chain special30 at 2^10, four towers, r = 11 (6 + 6 + 6 + 3 = 21 digits)
CHUNK_CASE = (10, 11, "special30", 4)
CHUNK_BATCHES = (1, 3)
# More than 256 digits: r = 1 on six towers at N = 2^6
MANY_BITS = [60, 59, 59, 30, 45, 45]
MANY_LOG_N = 6


def chunkings(n):
    return [0, 1, 2, n - 1, n, n + 5]


def chunk_spans(n, chunk):
    """[d0, d1) of every chunk the one-call key switch runs for chunk_digits = chunk > 0."""
    c = min(chunk, n)
    return [(d, min(n, d + c)) for d in range(0, n, c)]


def plant_words(qi, r):
    """Residues of q_i whose windows 0..j are all ones, for every j: each window then takes its largest value."""
    if r == 0:
        return []
    w = R.windows([qi], r)[0]
    words = {(1 << ((j + 1) * r)) - 1 for j in range(w)} | {((1 << r) - 1) << (j * r) for j in range(w)}
    return sorted(x for x in words if x < qi)


def planted_input(rng, B, q, rq, n, r):
    """(c in evaluation form, its coefficient form), both [B][T][n]."""
    coef = uniform(rng, B, q, n)
    for i, qi in enumerate(q):
        coef[:, i] = with_boundaries(rng, B, qi, n)
        words = plant_words(qi, r)[:n // 2]
        coef[:, i, 1:2 * len(words):2] = np.array(words, np.uint64)
    return K.set_format(coef, q, rq, True), coef


def chain_of(log_n, form):
    generic, small_bits, _ = FORMS[form]
    return bv_chain(log_n, generic, small_bits, extra=(45,))


def _chain(log_n, form, two_towers, bits):
    if bits is not None:
        return mixed_chain(log_n, list(bits))
    return mixed_chain(log_n, [60, 30]) if two_towers else chain_of(log_n, form)


@lru_cache(maxsize=64)
def case_input(log_n, r, form, towers, B=2, two_towers=False, bits=None):
    """The plan's chain (qa, ra) and the level's c with its coefficient form."""
    qa, ra = _chain(log_n, form, two_towers, bits)
    rng = np.random.default_rng(7000 + 100 * log_n + r)
    c, coef = planted_input(rng, B, qa[:towers], ra[:towers], 1 << log_n, r)
    return qa, ra, c, coef


@lru_cache(maxsize=4)
def reference(log_n, r, form, towers, B=2, two_towers=False, bits=None):
    """Inputs and the restatement's outputs of one case: the plan's chain (qa, ra), the level's q / rq, c, the
    keys over the whole chain's digit count, the digits and (ct0, ct1)."""
    n = 1 << log_n
    qa, ra, c, coef = case_input(log_n, r, form, towers, B, two_towers, bits)
    q, rq = qa[:towers], ra[:towers]
    rng = np.random.default_rng(9000 + 100 * log_n + r)
    nk = R.digit_count(qa, r)  # the keys serve the top level: a lower level uses a prefix of them
    kb = np.stack([uniform(rng, 1, qa, n)[0] for _ in range(nk)])
    ka = np.stack([uniform(rng, 1, qa, n)[0] for _ in range(nk)])
    digits = R.crt_decompose(c, q, rq, r)
    ct0, ct1 = R.bv_fast_core_digits(digits, kb, ka, q)
    return {"qa": qa, "ra": ra, "q": q, "rq": rq, "c": c, "coef": coef, "kb": kb, "ka": ka, "digits": digits,
            "ct0": ct0, "ct1": ct1, "n_digits": digits.shape[1]}


def launch_args(log_n):
    """reference() / case_input() arguments of a launch-path case."""
    if log_n >= 16:
        return (log_n, LAUNCH_R, "special30", 2, 1, True)
    return (log_n, LAUNCH_R, "special30", 4, 2)


def all_window_cases():
    """(q of the level, r, coefficient form) of every decomposition the GPU tests run on planted inputs."""
    out = []
    args = [launch_args(log_n) for log_n, _ in LAUNCH_PATHS] + DIGIT_SIZES + [CHUNK_CASE]
    for a in dict.fromkeys(args):
        qa, _, _, coef = case_input(*a)
        out.append((qa[:a[3]], a[1], coef))
    return out
