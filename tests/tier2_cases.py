"""Case generator of tests/test_gpu_fuzz_tier2.py: the seeded draws of the
rescaling, BV and HYBRID key-switch fuzz, as plain data.  Needs no GPU, so
tests/test_tier2_cases.py can check on the CPU that the committed seed ranges
reach what the fuzz is there for.

case(kind, seed) returns a dict with every parameter and the moduli.  A draw
that cannot be used (for example a digit count HYBRID key switching cannot
distribute) is drawn again from the same seed and the next attempt number, so
no seed is ever skipped.  PINS fixes single parameters of a few seeds where
the free draw would leave a launch path to chance."""
import math
import os

import numpy as np

import oracle as O
from test_gpu_fuzz import _random_prime
from test_mixed_moduli_oracle import regime

# OFHE_FUZZ_SCALE=k multiplies the case counts, as in tests/test_gpu_fuzz.py
SCALE = int(os.environ.get("OFHE_FUZZ_SCALE", "1"))
SEEDS = {"rescale": 48, "bv": 32, "keyswitch": 64}  # at scale 1
BASE = {"rescale": 21000, "bv": 23000, "keyswitch": 25000}
T_FIXED = (2, 3, 65537)

# plan splits by name (ofhe_hip.SPLIT_*), as ofhe_hip_plan_create_ex accepts them
def valid_splits(log_n):
    if log_n <= 12:
        return ["SPLIT_AUTO"]
    if log_n == 16:
        return ["SPLIT_AUTO", "SPLIT_COLS", "SPLIT_8_8"]
    if log_n == 17:
        return ["SPLIT_AUTO", "SPLIT_COLS", "SPLIT_9_8", "SPLIT_8_9"]
    return ["SPLIT_AUTO", "SPLIT_COLS"]


def valid_dnums(size_q):
    """The digit counts KeySwitchParams accepts (rns-cryptoparameters.cpp:75-83)."""
    return [d for d in range(1, size_q + 1) if size_q - math.ceil(size_q / d) * (d - 1) > 0]


# seed -> parameters fixed after the draw, per kind; everything else stays random.  Kept to what the free
# draw (see _log_n and _plan_options) leaves to chance in tests/test_tier2_cases.py.
PINS = {
    "rescale": {
        17: {"log_n": 12},
        19: {"log_n": 17, "split": "SPLIT_COLS"},
    },
    # 32 seeds hold the 17-size walk and two cases of each of the seven splits of 2^16 and 2^17 only with help
    "bv": {
        17: {"log_n": 16, "split": "SPLIT_AUTO"},
        19: {"log_n": 16, "split": "SPLIT_COLS"},
        20: {"log_n": 17, "split": "SPLIT_8_9"},
        22: {"log_n": 17, "split": "SPLIT_9_8"},
        23: {"log_n": 17, "split": "SPLIT_AUTO"},
        25: {"log_n": 17, "split": "SPLIT_COLS"},
        26: {"log_n": 17, "split": "SPLIT_COLS"},
    },
    "keyswitch": {
        # N = 2^17 at full level with a k_cols split: the options that choose between k_bconv_cols and the
        # unfused conversion (SPLIT_9_8 / SPLIT_8_9 always take the unfused one)
        14: {"log_n": 17, "split": "SPLIT_AUTO", "full_level": True, "separate_cols": 1, "separate_icol": 0},
        15: {"log_n": 17, "split": "SPLIT_AUTO", "full_level": True, "separate_cols": 1, "separate_icol": 1},
        16: {"log_n": 17, "split": "SPLIT_AUTO", "full_level": True, "separate_cols": 0, "separate_icol": 1},
        17: {"log_n": 17, "split": "SPLIT_COLS", "full_level": True, "separate_cols": 0, "separate_icol": 0},
        22: {"log_n": 12, "batch": 3, "chunk": 2},
        24: {"log_n": 10, "size_q": 10, "dnum": 5, "full_level": True},
        25: {"log_n": 13, "size_q": 6, "dnum": 6, "full_level": True},
        28: {"log_n": 9, "size_q": 8, "dnum": 4, "full_level": True},
        29: {"log_n": 14, "size_q": 12, "dnum": 4, "full_level": True},
    },
}


def _moduli(rng, log_n, count, lo_bits):
    """count distinct primes = 1 mod 2N of max(lo_bits, log_n + 4) .. 60 bits,
    each of the special form 2^L - d or generic at random."""
    m = 2 << log_n
    qs, special, sizes = [], [], []
    while len(qs) < count:
        bits = int(rng.integers(max(lo_bits, log_n + 4), 61))
        # one tower in three takes the size of an earlier one, as the equal-sized scaling primes of a real
        # chain do: neighbours within a factor of two are SwitchModulus's "two subtractions" branch
        if sizes and rng.integers(0, 3) == 0:
            bits = sizes[int(rng.integers(0, len(sizes)))]
        sp = bool(rng.integers(0, 2))
        q = _random_prime(O, rng, bits, m, sp)
        while q in qs:  # the special form of a size is one prime: step down from it
            q = O.previous_prime(q, m)
        if q >= 1 << (max(lo_bits, log_n + 4) - 1):
            qs.append(q)
            special.append(sp)
            sizes.append(bits)
    return qs, [O.root_of_unity(m, q) for q in qs], special


def _log_n(rng, seed, lo, pin):
    # the first seeds walk every ring size once; of the rest, two in three are drawn from all sizes and every
    # third alternates between 2^16 and 2^17, the two sizes with more than two plan splits
    span = 18 - lo
    drawn = int(rng.integers(lo, 18))
    if seed >= span and seed % 3 == 0:
        drawn = 16 + (seed // 3) % 2
    return pin.get("log_n", lo + seed if seed < span else drawn)


def _plan_options(rng, seed, log_n, pin):
    # the split rotates with the seed where the ring size has more than two (so a short seed range meets each),
    # and is drawn elsewhere
    splits = valid_splits(log_n)
    drawn = int(rng.integers(0, len(splits)))
    split = splits[(seed // 6) % len(splits) if len(splits) > 2 and seed % 3 == 0 else drawn]
    generic = int(rng.integers(0, 2))
    return pin.get("split", split), pin.get("generic_moduli", generic)


def _draw(kind, seed, attempt):
    rng = np.random.default_rng([BASE[kind], seed, attempt])
    pin = PINS[kind].get(seed, {})
    if kind in ("rescale", "bv"):
        log_n = _log_n(rng, seed, 1, pin)
        big = log_n >= 15
        if kind == "rescale":
            plan_towers = int(rng.integers(2, 5 if big else 9))
            towers = int(rng.integers(2, plan_towers + 1))
            batch = int(rng.integers(1, 4))
        else:
            towers = int(rng.integers(1, 6))
            plan_towers = towers + int(rng.integers(0, 3))  # the keys' towers
            batch = int(rng.integers(1, 3))
        split, generic = _plan_options(rng, seed, log_n, pin)
        q, r, special = _moduli(rng, log_n, plan_towers, 22)
        c = dict(kind=kind, seed=seed, log_n=log_n, plan_towers=plan_towers, towers=towers, batch=batch, split=split,
                 generic_moduli=generic, q=q, r=r, special=special)
        if kind == "rescale":
            t_choice = int(rng.integers(0, 4))
            t_odd = int(rng.integers(1, 1 << 19)) * 2 + 1  # a random odd below 2^20 (every modulus is larger)
            c.update(eval_form=bool(rng.integers(0, 2)), op=("drop_last", "mod_reduce")[int(rng.integers(0, 2))],
                     t=T_FIXED[t_choice] if t_choice < 3 else t_odd, in_place=bool(rng.integers(0, 2)),
                     pad=int(rng.integers(0, 2)))
            c["regimes"] = sorted({regime(q[towers - 1], q[i]) for i in range(towers - 1)})
        else:
            c["regimes"] = sorted({regime(q[i], q[k]) for i in range(towers) for k in range(towers) if i != k})
        c["data_seed"] = int(rng.integers(0, 1 << 31))
        return c
    assert kind == "keyswitch"
    return keyswitch_draw(rng, seed, pin, kind)


def keyswitch_draw(rng, seed, pin, kind="keyswitch"):
    """The HYBRID key-switch draw from rng (None: dnum cannot be distributed, draw again); shared with
    tests/tier3_cases.py, whose rotation cases are this draw plus their own parameters."""
    log_n = _log_n(rng, seed, 4, pin)
    big = log_n >= 15
    size_q = pin.get("size_q", int(rng.integers(1, 7 if big else 13)))
    size_p = int(rng.integers(1, 7))
    dnums = valid_dnums(size_q)
    dnum = pin.get("dnum", dnums[int(rng.integers(0, len(dnums)))])
    if dnum not in dnums:
        return None
    level = int(rng.integers(1, size_q + 1))
    if pin.get("full_level"):
        level = size_q
    t_choice = int(rng.integers(0, 3))
    t_odd = int(rng.integers(1, 1 << 19)) * 2 + 1
    batch = pin.get("batch", int(rng.integers(1, 5)))
    chunk = pin.get("chunk", [0, 1, 2, batch, batch + 1][int(rng.integers(0, 5))])
    split, generic = _plan_options(rng, seed, log_n, pin)
    opts = dict(single_stream=int(rng.integers(0, 2)), separate_cols=int(rng.integers(0, 2)),
                separate_icol=int(rng.integers(0, 2)))
    opts = {k: pin.get(k, v) for k, v in opts.items()}
    m, r, special = _moduli(rng, log_n, size_q + size_p, 30)
    alpha = math.ceil(size_q / dnum)
    return dict(kind=kind, seed=seed, log_n=log_n, size_q=size_q, size_p=size_p, dnum=dnum, level=level,
                beta=min(math.ceil(level / alpha), dnum), t=(0, 65537, t_odd)[t_choice], batch=batch, chunk=chunk,
                split=split, generic_moduli=generic, q=m[:size_q], rq=r[:size_q], p=m[size_q:], rp=r[size_q:],
                special=special, data_seed=int(rng.integers(0, 1 << 31)), **opts)


def case(kind, seed):
    for attempt in range(64):
        c = _draw(kind, seed, attempt)
        if c is not None:
            c["attempt"] = attempt
            return c
    raise AssertionError(f"no valid draw for {kind} seed {seed}")
