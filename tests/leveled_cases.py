"""Shared inputs of the HPSPOVERQLEVELED tests: tests/test_gpu_bfv_leveled.py runs them on the
device, tests/test_bfv_leveled_oracle.py asserts on these very inputs that each scale-round-lift
case can tell a fused double sum from the contract's.  Every reference is computed once and cached."""
import numpy as np

import bfv_leveled_ref as LR
import bfv_tables as BT
import oracle as O
from test_mixed_moduli_oracle import mixed_chain

T_PLAIN = 65537
# The scale-round-lift cases take a 59-bit plaintext modulus.  With one tower (l = 0) the only
# fractional table entry is t / r_0: for a small t the product frac * x stays below 2^17, where
# the product's rounding error is far below that of the sum 0.5 + product and a fused chain
# can never give another floor; for a 59-bit t the product reaches 2^59 (ulp 128) and about one
# uniform input in 256 is sensitive.
SR_T = (1 << 58) + 27
BATCH = 3

# (log_n, l + 1, dropped towers): both sides of k_scale_round_lift's tile of 4 output towers and past
# 16; 0, 1 and 3 zero towers; N from 2 (one coefficient pair) to 2^10 (four blocks)
SR_LIFT_CASES = [(1, 1, 0), (1, 1, 1), (2, 4, 3), (3, 5, 1), (5, 4, 1), (5, 17, 1), (7, 5, 3), (10, 4, 0), (10, 5, 3),
                 (10, 17, 3)]

# 22-60-bit towers in one chain (generic primes: no special-prime kernel path), q then r
MIXED_Q_BITS = [60, 22, 45, 31, 58]
MIXED_R_BITS = [60, 36, 46, 32, 59]

_cache = {}


def cached(key, build):
    if key not in _cache:
        _cache[key] = build()
    return _cache[key]


def level_chain(log_n, sq, mixed=False):
    """(q, rq, r, rr): size_q ciphertext towers and as many auxiliary ones"""
    if mixed:
        assert sq <= len(MIXED_Q_BITS)
        q, rq = mixed_chain(log_n, MIXED_Q_BITS[:sq], generic=True)
        r, rr = mixed_chain(log_n, MIXED_R_BITS[:sq])
        assert not set(q) & set(r)
        return q, rq, r, rr
    m, roots = O.moduli_chain(log_n, 2 * sq)
    return m[:sq], roots[:sq], m[sq:], roots[sq:]


def sr_lift_case(log_n, L, k):
    """(T, x [BATCH][2 L][n] over Q_l R_l, planted): batch entry 0 starts with `planted` coefficients
    on which a fused chain gives another floor(nu), then 0 and q_i - 1 / r_i - 1 columns; the rest is
    uniform"""
    def build():
        q, _, r, _ = level_chain(log_n, L + k)
        T = BT.LeveledTables(q, r, SR_T, L - 1)
        n = 1 << log_n
        x = O.uniform_dcrt(BATCH, 2 * L, n, T.ql + T.rl, 700 + 10 * L + k)
        x[1, :, 0] = 0
        x[1, :, n - 1] = [m - 1 for m in T.ql + T.rl]
        planted = LR.plant_scale_inputs(x, T.rl, T.sr_frac, L, seed=log_n * 100 + L)
        return T, x, planted
    return cached(("srl", log_n, L, k), build)
