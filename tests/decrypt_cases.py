"""Case generator of tests/test_gpu_fuzz_decrypt.py: the seeded draws of the BFV
decryption fuzz and its fixed scale-round and TimesQovert inputs, as plain data.
Needs no GPU, so tests/test_decrypt_cases.py can check on the CPU that the
committed seed range and the fixed inputs reach what the GPU file is there for.

case(seed) works as behz_cases.case does (a draw that cannot be used is drawn
again from the same seed and the next attempt number; PINS fixes single
parameters of a few seeds), and the helpers are tier2_cases' own: _moduli,
_log_n, _plan_options, valid_splits and OFHE_FUZZ_SCALE.  The reference of
everything here is tests/decrypt_ref.py."""
import math

import numpy as np

import bfv_ref as BR
import bfv_tables as BT
import decrypt_ref as D
import oracle as O
import tier2_cases as C2
from test_gpu_fuzz import _edge_inputs
from test_mixed_moduli_oracle import mixed_chain

U64 = np.uint64
SCALE = C2.SCALE
SEEDS = 40  # at scale 1
BASE = 43000  # disjoint from every tier2_cases.BASE, tier3_cases.BASE and behz_cases.BASE
TECHNIQUES = ("BFV_HPS", "BFV_HPSPOVERQ", "BFV_BEHZ")  # ofhe_hip.BFV_*
P45, P55 = (1 << 45) - 55, (1 << 55) - 55  # the primes next below 2^45 and 2^55
T_LIST = (2, 1 << 15, 1 << 31, 65537, 5308417, 3221225473, P45, P55)
# an encryption Delta m + e with |e| <= 3 decrypts where t e / Q stays far below 1 / 2 (decrypt_ref.encryption_sum
# bounds the plaintext's own term): a draw of t keeps Q >= ENC_MARGIN t
ENC_MARGIN = 64

PINS = {
    # a 60-bit q[0] in front of towers down to 24 bits: the split at 30 bits leaves hi = 0 in the narrow towers (G)
    17: {"log_n": 8, "bits": [60, 24, 45, 31, 60], "t": 65537, "technique": "BFV_HPS"},
    # a 27-bit q[0] in front of 60-bit towers, not split, sums reduced mod t (F): u2d of x_i >= 2^53 rounds
    19: {"log_n": 6, "bits": [27, 60, 60, 30, 52, 22, 58], "t": 5308417, "technique": "BFV_HPSPOVERQ"},
    # loop B with a 60-bit tower behind a 30-bit q[0]
    20: {"log_n": 9, "bits": [30, 60], "t": 1 << 31, "technique": "BFV_HPS"},
    # loop A likewise: lo * w wraps, u2d rounds
    22: {"log_n": 5, "bits": [24, 60, 60], "t": 1 << 15, "technique": "BFV_HPS"},
    # the two sides of qMSB + sizeQMSB = 52: 7 towers of 48 bits are F, 8 are G
    23: {"log_n": 7, "bits": [48] * 7, "t": 65537, "technique": "BFV_HPS"},
    25: {"log_n": 13, "bits": [48] * 8, "t": 65537, "technique": "BFV_HPSPOVERQ", "split": "SPLIT_AUTO",
         "generic_moduli": 1},
    # one tower through the decrypt call where the transforms are the column-pass kernels, and above them
    26: {"log_n": 13, "size_q": 1, "split": "SPLIT_AUTO", "generic_moduli": 0},
    28: {"log_n": 16, "size_q": 1},
    # 17 towers: past DEC_TILE and past 16, three tiles of k_dec_scale_round (C, a power-of-two loop)
    29: {"log_n": 10, "bits": [60, 45, 52, 31, 60, 24, 60, 58, 37, 60, 49, 60, 28, 55, 60, 41, 60], "t": 1 << 15,
         "technique": "BFV_HPS", "batch": 2},
    # a 52-bit q[0] splits at 26 bits: hi of a 60-bit tower reaches 2^34 (H)
    31: {"log_n": 8, "bits": [52, 60, 45], "t": 3221225473, "technique": "BFV_HPS"},
    # the loops the free draw leaves to chance: D (60-bit q[0], t = 2^31) and E (30-bit q[0], t = 65537)
    32: {"log_n": 16, "bits": [60, 60, 38], "t": 1 << 31, "technique": "BFV_HPSPOVERQ", "split": "SPLIT_AUTO",
         "generic_moduli": 1},
    34: {"log_n": 4, "bits": [30, 30], "t": 65537, "technique": "BFV_HPS"},
    # the plan options of 2^13, 2^16 and 2^17 that 40 seeds leave out (25, 26, 28 and 32 above take four of them)
    30: {"log_n": 17, "split": "SPLIT_COLS", "generic_moduli": 1},
    35: {"log_n": 13, "split": "SPLIT_COLS", "generic_moduli": 1},
    36: {"log_n": 16, "split": "SPLIT_COLS", "generic_moduli": 1, "size_q": 2},
    37: {"log_n": 17, "split": "SPLIT_8_9", "generic_moduli": 1, "size_q": 2},
    38: {"log_n": 17, "split": "SPLIT_9_8", "generic_moduli": 1, "size_q": 2},
}


def admissible(t, q, technique):
    """ofhe_hip_bfv_decrypt_create takes (q, t) under this technique, t is coprime to every tower, and an
    encryption decrypts"""
    if 2 * len(q) * t >= 1 << 64 or any(math.gcd(t, m) != 1 for m in q):
        return False
    if technique == "BFV_BEHZ" and len(q) > 1 and t >= 1 << 32:
        return False
    return BT.product(q) >= ENC_MARGIN * t


def _draw(rng, seed, pin):
    log_n = C2._log_n(rng, seed, 1, pin)
    big = log_n >= 15  # the CPU reference takes seconds there: fewer towers, one entry
    size_q = pin.get("size_q", int(rng.integers(1, 3 if big else 7)))
    batch = pin.get("batch", 1 if big else int(rng.integers(1, 4)))
    plan = C2._plan_options(rng, seed, log_n, pin)
    technique = pin.get("technique", TECHNIQUES[int(rng.integers(0, 3))])
    elements = pin.get("elements", int(rng.integers(2, 4)))
    eval_form = pin.get("eval_form", bool(rng.integers(0, 2)))
    if "bits" in pin:
        generic = bool(seed % 2)  # special and generic form alternate with the seed, as behz_cases._draw
        q, rq = mixed_chain(log_n, pin["bits"], generic=generic)
        special = [not generic] * len(q)
    else:
        q, rq, special = C2._moduli(rng, log_n, size_q, 22)
    ts = [t for t in T_LIST if admissible(t, q, technique)]
    pick = int(rng.integers(0, 1 << 31))
    if not ts or pin.get("t", ts[0]) not in ts:
        return None
    return dict(seed=seed, log_n=log_n, size_q=len(q), batch=batch, plan_q=plan, technique=technique,
                elements=elements, eval_form=eval_form, t=pin.get("t", ts[pick % len(ts)]), q=q, rq=rq,
                special=special, data_seed=int(rng.integers(0, 1 << 31)))


def case(seed):
    pin = PINS.get(seed, {})
    for attempt in range(64):
        c = _draw(np.random.default_rng([BASE, seed, attempt]), seed, pin)
        if c is not None:
            c["attempt"] = attempt
            return c
    raise AssertionError(f"no valid draw for seed {seed}")


def behz(c):
    return c["technique"] == "BFV_BEHZ"


def branch_name(T, is_behz):
    """the loop ofhe_hip_bfv_decrypt_branch must report: A-H, "BEHZ" or "ONE_TOWER" """
    return "ONE_TOWER" if len(T.q) == 1 else "BEHZ" if is_behz else BT.BRANCHES[T.branch]


def reference_decrypts(T, is_behz):
    """The reference's own error analysis covers (q, t), so an encryption must decrypt under it.  It sizes every
    tower by q[0] (dcrtpoly-impl.h:1547), so no tower may be wider than q[0]: behind a narrower q[0] the loops
    A, B, E, F round double(x_i) of a wide tower and lose whole units of the sum.  In F and H the sum of up to
    2 size_q products below t must stay below 2^52 for double(intSum) to be exact.  Where this is False the
    reference's output is still defined and the library must reproduce it bit for bit; it is not the plaintext."""
    if len(T.q) == 1 or is_behz:
        return True
    if max(T.q).bit_length() > T.q[0].bit_length():
        return False
    return not (T.branch >= 4 and T.branch & 1) or (2 if T.split else 1) * len(T.q) * T.t < 1 << 52


_sweep = {}


def sweep_inputs(c):
    """dict of one case, built once: T, tb (the oracle's transform tables), s_eval [Q][n], elems (the 2 or 3
    elements [batch][Q][n] in evaluation form), plain (the plaintext of batch entry 0), x (the INTT of DecryptCore's
    output: ScaleAndRound's input), tq (TimesQovert's input).

    Batch entry 0 is a synthesised encryption that needs no O(N^2) product: m and the noise as
    decrypt_ref.encryption_sum draws them, c1 (and c2) edge-heavy uniform in evaluation form, a ternary s, and
    c0 = NTT(Delta m + e) - c1 s (- c2 s^2) towerwise.  The other entries are _edge_inputs.  Inputs on which the
    final cast of the loops E-H would be undefined (decrypt_ref.defined) are drawn again; none has been met."""
    if c["seed"] in _sweep:
        return _sweep[c["seed"]]
    q, t, n, batch = c["q"], c["t"], 1 << c["log_n"], c["batch"]
    T, tb = BT.DecryptTables(q, t), O.Tables(n, q, c["rq"])
    for salt in range(64):
        rng = np.random.default_rng([c["data_seed"], salt])
        s = np.array([int(v) for v in rng.integers(-1, 2, size=n)], dtype=object)
        s_eval = O.ntt_fwd(BR.residues(s.reshape(1, n), q), tb)
        elems = [_edge_inputs(rng, batch, q, n) for _ in range(c["elements"])]
        b0, plain = D.encryption_sum(rng, q, t, n)
        acc, sp = O.ntt_fwd(b0, tb), s_eval
        for e in elems[1:]:
            acc = O.eltwise("sub", acc, O.eltwise("mul", e[:1], sp, q), q)
            sp = O.eltwise("mul", sp, s_eval, q)
        elems[0][:1] = acc
        x = O.ntt_inv(D.decrypt_core(O, elems, s_eval[0], q), tb)
        if len(q) == 1 or behz(c) or D.defined(x, T).all():
            break
    else:
        raise AssertionError(f"no defined inputs for seed {c['seed']}")
    tq = _edge_inputs(rng, batch, q, n)
    _sweep[c["seed"]] = dict(T=T, tb=tb, s_eval=s_eval[0], elems=elems, plain=plain, x=x, tq=tq, salt=salt)
    return _sweep[c["seed"]]


def want_decrypt(c, k):
    """the reference's output of the decrypt call in the case's form, [batch][n]"""
    elems = k["elems"] if c["eval_form"] else [O.ntt_inv(e, k["tb"]) for e in k["elems"]]
    return D.decrypt(O, elems, k["s_eval"], k["T"], k["tb"], c["eval_form"], behz(c))


# ---- fixed scale-round inputs ---------------------------------------------------------------------------------
def uniform(rng, moduli, batch, n):
    return np.stack([np.stack([rng.integers(0, int(m), size=n, dtype=U64) for m in moduli]) for _ in range(batch)])


def _columns(values, q):
    """integers -> their residues [len(values)][Q]"""
    return np.array([[int(v) % m for m in q] for v in values], dtype=U64).reshape(len(values), len(q))


def _make_defined(rng, x, T):
    """replace, as decrypt_ref.hps_case does, every coefficient on which the final cast of the loops E-H would be
    undefined by uniform residues -> how many were replaced"""
    replaced = 0
    for _ in range(64):
        bad = ~D.defined(x, T)
        if not bad.any():
            return replaced
        for b, ri in zip(*np.nonzero(bad)):
            x[b, :, ri] = [int(rng.integers(0, m)) for m in T.q]
            replaced += 1
    raise AssertionError("inputs stay undefined")


# name -> (technique, t, the towers' bits or an explicit list of sizes, towers, log_n, batch)
# H at the largest sums create admits (2 size_q t < 2^64; 255 towers are size_q's limit); F with sums past 2^53 --
# 255 t >= 2^53 needs t above 2^45, so the "near 2^45" entry takes 2^46 - 21 with 255 towers and a second one takes
# 2^55 + 3 on five 30-bit towers; BEHZ at the top of t < 2^32, on 60-bit towers and on towers below t 2^26
LARGE_T = {
    "H-2^55+3-60x33": ("BFV_HPS", (1 << 55) + 3, 60, 33, 7, 2),
    "H-2^50+5-55x17": ("BFV_HPSPOVERQ", (1 << 50) + 5, 55, 17, 8, 3),
    "H-2^56-5-60x100": ("BFV_HPS", (1 << 56) - 5, 60, 100, 5, 2),
    "H-2^55+3-60x255": ("BFV_HPS", (1 << 55) + 3, 60, 255, 4, 2),
    "F-2^46-21-40x255": ("BFV_HPS", (1 << 46) - 21, 40, 255, 4, 2),
    "F-2^55+3-30x5": ("BFV_HPS", (1 << 55) + 3, 30, 5, 8, 3),
    "BEHZ-2^32-1-60x5": ("BFV_BEHZ", (1 << 32) - 1, 60, 5, 8, 3),
    "BEHZ-2^32-5-60x2": ("BFV_BEHZ", (1 << 32) - 5, 60, 2, 8, 3),
    "BEHZ-2^32-1-narrow": ("BFV_BEHZ", (1 << 32) - 1, [22, 30, 26, 24, 28, 23], 6, 8, 3),
    "BEHZ-2^32-5-narrow": ("BFV_BEHZ", (1 << 32) - 5, [30, 22, 27], 3, 4, 2),
}
_fixed = {}


def large_t_case(name):
    """dict: T, technique, log_n, n, batch, x, planted (the flat (batch, n) positions that hold planted_values
    boundaries), replaced.  Entry 0 is uniform with q_i - 1 in every tower of coefficient 0; the first half of
    entry 1 is planted on the rounding boundaries of t v / Q, the rest uniform."""
    if name in _fixed:
        return _fixed[name]
    technique, t, bits, towers, log_n, batch = LARGE_T[name]
    n = 1 << log_n
    q = D.towers_below(O, log_n, bits, towers) if isinstance(bits, int) else mixed_chain(log_n, bits)[0]
    assert len(q) == towers
    T = BT.DecryptTables(q, t)
    rng = np.random.default_rng([45000, list(LARGE_T).index(name)])
    x = uniform(rng, q, batch, n)
    x[0, :, 0] = [m - 1 for m in q]
    x[1, :, :n // 2] = _columns(D.planted_values(rng, T.Q, t, n // 2), q).T
    replaced = 0 if technique == "BFV_BEHZ" else _make_defined(rng, x, T)
    _fixed[name] = dict(T=T, technique=technique, log_n=log_n, n=n, batch=batch, x=x, replaced=replaced,
                        planted=np.arange(n, n + n // 2))
    return _fixed[name]


# the rows of decrypt_ref.BRANCH_TABLE: loops E-H under HPS, every row under BEHZ; 5 towers of 30 bits, 2 of the
# wider ones (F at t = 5308417 / 30 bits / 5 towers and H at 5308417 / 55 bits / 2 towers are known to give t)
EQUALS_T = [("BFV_HPS", letter, t, bits, 5 if bits == 30 else 2) for letter, t, bits in D.BRANCH_TABLE
            if letter in "EFGH"] + \
    [("BFV_BEHZ", letter, t, bits, 5 if bits == 30 else 2) for letter, t, bits in D.BRANCH_TABLE]
EQUALS_LOG_N, EQUALS_BATCH, EQUALS_E = 8, 2, 32  # the ring of decrypt_ref.HPS_CASES' towers


def equals_t_case(c):
    """dict as large_t_case: the first 32 coefficients of entry 0 are Q - e, e = 1 .. 32 (a zero plaintext under
    a small negative noise, which rounds up to t), every other one a planted_values boundary"""
    key = ("equals",) + tuple(c)
    if key in _fixed:
        return _fixed[key]
    technique, _, t, bits, towers = c
    n, batch = 1 << EQUALS_LOG_N, EQUALS_BATCH
    q = D.towers_below(O, EQUALS_LOG_N, bits, towers)
    T = BT.DecryptTables(q, t)
    rng = np.random.default_rng([46000, EQUALS_T.index(c)])
    values = [T.Q - e for e in range(1, EQUALS_E + 1)] + D.planted_values(rng, T.Q, t, batch * n - EQUALS_E)
    x = np.ascontiguousarray(_columns(values, q).reshape(batch, n, towers).transpose(0, 2, 1))
    replaced = 0 if technique == "BFV_BEHZ" else _make_defined(rng, x, T)
    _fixed[key] = dict(T=T, technique=technique, log_n=EQUALS_LOG_N, n=n, batch=batch, x=x, replaced=replaced)
    return _fixed[key]


# (q, t) of the one-tower path beyond t < q / 2: q <= 2 t (two csubs), t > q (no reduction, MR(v) >= q, the
# wrapping q - MR(q - v)); scale-round needs only an odd q >= 3.  None stands for the 60-bit prime of towers_below
ONE_TOWER_WIDE = [(17, 5), (17, 9), (17, 16), (17, 19), (97, 65537), (4194217, (1 << 31) - 1), (None, (1 << 61) - 1)]


def one_tower_wide_case(c):
    """dict: T, log_n, n, batch 2, x [2][1][n]: every residue (in order, then again in uniform draws) where
    q <= 256, else 0, 1, q >> 1, (q >> 1) + 1, q - 1 and uniform residues"""
    key = ("wide",) + tuple(c)
    if key in _fixed:
        return _fixed[key]
    q, t = c
    q = q or D.towers_below(O, 4, 60, 1)[0]
    log_n = 5 if q <= 32 else 7 if q <= 128 else 6
    n = 1 << log_n
    rng = np.random.default_rng([47000, ONE_TOWER_WIDE.index(c)])
    x = rng.integers(0, q, size=(2, 1, n), dtype=U64)
    head = list(range(q)) if q <= 256 else [0, 1, q >> 1, (q >> 1) + 1, q - 1]
    x[0, 0, :len(head)] = head
    _fixed[key] = dict(T=BT.DecryptTables([q], t), log_n=log_n, n=n, batch=2, x=x)
    return _fixed[key]


# ---- TimesQovert ----------------------------------------------------------------------------------------------
# name -> (t, towers: bit sizes (mixed_chain) or explicit odd moduli).  ofhe_hip_bfv_decrypt_create admits
# 2 size_q t < 2^64 only, so it must refuse t = 2^62 on two towers (TQT_REFUSED: the reference is checked on the
# CPU, the refusal on the device) and the nearest it admits stand next to it: 2^61 on two towers, 2^62 on one
TQT = {
    "t2-60x3": (2, [60, 60, 60]),
    "t2^31-mixed": (1 << 31, [22, 60, 31, 45]),
    "t65537-above-q": (65537, (17, 97, "22")),
    "tP55-60x2": (P55, [60, 60]),
    "t2^62-60x2": (1 << 62, [60, 60]),
    "t2^61-60x2": (1 << 61, [60, 60]),
    "t2^62-60x1": (1 << 62, [60]),
}
TQT_REFUSED = ("t2^62-60x2",)
TQT_LOG_N, TQT_BATCH = 6, 2


def tqt_case(name):
    """dict: T, log_n, n, batch, x [2][Q][n] of any 64-bit words: 0, t - 1, t, q_i - 1, q_i, 2^63 and 2^64 - 1
    lead entry 0, the rest of it is uniform over 2^64; entry 1 holds values below t (where an exact scaling is
    defined) in its first half and uniform 64-bit words in the second"""
    if name in _fixed:
        return _fixed[name]
    t, towers = TQT[name]
    n = 1 << TQT_LOG_N
    if isinstance(towers, tuple):
        q = [m if isinstance(m, int) else mixed_chain(TQT_LOG_N, [int(m)])[0][0] for m in towers]
    else:
        q = mixed_chain(TQT_LOG_N, towers)[0]
    T = BT.DecryptTables(q, t)
    rng = np.random.default_rng([48000, list(TQT).index(name)])
    x = rng.integers(0, 1 << 64, size=(TQT_BATCH, len(q), n), dtype=U64)
    for i, m in enumerate(q):
        x[0, i, :7] = [0, t - 1, t, m - 1, m, 1 << 63, (1 << 64) - 1]
    below = np.array([int(rng.integers(0, min(t, 1 << 63))) for _ in range(n // 2)], dtype=U64)
    below[:2] = [0, t - 1]
    x[1, :, :n // 2] = below[None, :]
    _fixed[name] = dict(T=T, log_n=TQT_LOG_N, n=n, batch=TQT_BATCH, x=x)
    return _fixed[name]
