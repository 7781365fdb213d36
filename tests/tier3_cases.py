"""Case generator of tests/test_gpu_fuzz_tier3.py: the seeded draws of the
hoisted-rotation, BFV EvalMult, ScaleAndRound and exact-switch fuzz, as plain
data.  Needs no GPU, so tests/test_tier3_cases.py can check on the CPU that the
committed seed ranges reach what the fuzz is there for.

case(kind, seed) works as tier2_cases.case does (a draw that cannot be used is
drawn again from the same seed and the next attempt number; PINS fixes single
parameters of a few seeds), and the helpers are tier2_cases' own: _moduli,
_log_n, _plan_options, valid_splits, valid_dnums, keyswitch_draw and
OFHE_FUZZ_SCALE."""
import numpy as np

import bfv_ref as R
import tier2_cases as C2
from test_mixed_moduli_oracle import mixed_chain

SCALE = C2.SCALE
SEEDS = {"rotation": 48, "bfv_mult": 40, "scale_round": 32, "switch_exact": 32}  # at scale 1
BASE = {"rotation": 31000, "bfv_mult": 33000, "scale_round": 35000, "switch_exact": 37000}
KS_ROT_CAP = 16  # ofhe_hip.KS_ROT_CAP (csrc/ks_kernels.hpp); tests/test_gpu_fuzz_tier3.py asserts they agree
KERNELS = ("BCONV_KERNEL_AUTO", "BCONV_KERNEL_LIMB", "BCONV_KERNEL_WIDE")
HPS, HPSPOVERQ = 0, 1  # bfv_tables.HPS, bfv_tables.HPSPOVERQ
# words of one output set (nrot x batch x towers x N) above which a rotation case takes fewer rotations
ROT_WORDS = 1 << 21

PINS = {
    "rotation": {
        # more than two full launches of k_ks_inner_rot (the third launch's r0 * rot_stride / r0 * per_rot
        # offsets), narrow and wide, on a small ring
        3: {"log_n": 5, "nrot": 2 * KS_ROT_CAP + 1, "batch": 2},
        4: {"log_n": 6, "size_q": 10, "dnum": 5, "full_level": True, "nrot": 2 * KS_ROT_CAP + 1, "batch": 1},
        # N = 2^17 at full level with a k_cols split: the options that choose between k_bconv_cols and the
        # unfused conversion in the non-Ext call's ModDown over nrot * batch entries
        14: {"log_n": 17, "split": "SPLIT_AUTO", "full_level": True, "separate_cols": 1, "separate_icol": 0,
             "batch": 1},
        15: {"log_n": 17, "split": "SPLIT_AUTO", "full_level": True, "separate_cols": 1, "separate_icol": 1,
             "batch": 1},
        16: {"log_n": 17, "split": "SPLIT_AUTO", "full_level": True, "separate_cols": 0, "separate_icol": 1,
             "batch": 1},
        17: {"log_n": 17, "split": "SPLIT_COLS", "full_level": True, "separate_cols": 0, "separate_icol": 0,
             "batch": 1},
        # ModUp in ragged chunks feeding the rotation
        22: {"log_n": 12, "batch": 3, "chunk": 2, "from_precompute": True},
        23: {"log_n": 9, "batch": 4, "chunk": 3, "from_precompute": True},
        24: {"log_n": 10, "size_q": 10, "dnum": 5, "full_level": True},
        25: {"log_n": 13, "size_q": 6, "dnum": 6, "full_level": True},
        28: {"log_n": 9, "size_q": 8, "dnum": 4, "full_level": True},
        29: {"log_n": 14, "size_q": 12, "dnum": 4, "full_level": True, "batch": 1},
        27: {"log_n": 17, "split": "SPLIT_9_8"},
        36: {"log_n": 16, "split": "SPLIT_COLS"},
        44: {"log_n": 16, "split": "SPLIT_AUTO"},
    },
    "bfv_mult": {
        # a tower below 32 bits next to one of 60 in one chain
        18: {"log_n": 8, "bits": [60, 24, 45, 31, 60]},
        19: {"log_n": 11, "bits": [27, 60, 60, 30, 52, 22, 58]},
        22: {"size_q": 6},  # HPSPOVERQ with Q = R = 6
        36: {"plan_qr": ("SPLIT_COLS", 1)},  # the column-pass plan over Q + R towers at 2^16
    },
    "scale_round": {},
    "switch_exact": {},
}


def _pinned_moduli(log_n, bits, seed):
    """a chain of the given sizes, special and generic form alternating with the seed"""
    generic = bool(seed % 2)
    m, r = mixed_chain(log_n, bits, generic=generic)
    return m, r, [not generic] * len(bits)


def _rotation(rng, seed, pin):
    c = C2.keyswitch_draw(rng, seed, pin, "rotation")
    if c is None:
        return None
    n, towers = 1 << c["log_n"], c["level"] + c["size_p"]
    big = c["log_n"] >= 15
    batch = pin.get("batch", min(c["batch"], 2) if big else c["batch"])
    c["chunk"] = pin.get("chunk", min(c["chunk"], batch + 1))
    nrot = int(rng.integers(1, 2 * KS_ROT_CAP + 2))
    nrot = pin.get("nrot", max(1, min(nrot, ROT_WORDS // (batch * towers * n))))
    c.update(batch=batch, nrot=nrot, add_first=bool(rng.integers(0, 2)),
             from_precompute=pin.get("from_precompute", bool(rng.integers(0, 2))),
             column=int(rng.integers(0, n)),
             rot_seed=int(rng.integers(0, 1 << 31)))
    return c


def _bfv_mult(rng, seed, pin):
    log_n = C2._log_n(rng, seed, 1, pin)
    # the CPU reference works with Python integers: fewer towers and entries on the large rings
    qmax, bmax = (2, 1) if log_n >= 15 else (3, 2) if log_n >= 13 else (6, 3)
    tech = int(rng.integers(0, 2))
    size_q = pin.get("size_q", int(rng.integers(1, qmax + 1)))
    size_r = size_q + (int(rng.integers(0, 2)) if tech == HPS else 0)
    batch = int(rng.integers(1, bmax + 1))
    plans = {"plan_q": C2._plan_options(rng, seed, log_n, pin)}
    for name in ("plan_r", "plan_qr"):  # separate handles: their options are drawn, not rotated with the seed
        plans[name] = pin.get(name, C2._plan_options(rng, 1, log_n, {}))
    kernels = {name: KERNELS[int(rng.integers(0, 3))] for name in ("q_to_r", "r_to_q", "q_to_r_neg")}
    if tech == HPS:
        kernels["q_to_r_neg"] = None
    if "bits" in pin:
        bits = pin["bits"]
        size_q = len(bits) // 2
        size_r = len(bits) - size_q
        tech = HPS if size_r > size_q else tech
        if tech == HPS:
            kernels["q_to_r_neg"] = None
        m, r, special = _pinned_moduli(log_n, bits, seed)
    else:
        m, r, special = C2._moduli(rng, log_n, size_q + size_r, 22)
    return dict(kind="bfv_mult", seed=seed, log_n=log_n, technique=tech, size_q=size_q, size_r=size_r, batch=batch,
                eval_form=bool(rng.integers(0, 2)), plans=plans, kernels=kernels, q=m[:size_q], rq=r[:size_q],
                r=m[size_q:], rr=r[size_q:], special=special, data_seed=int(rng.integers(0, 1 << 31)))


def _scale_round(rng, seed, pin):
    log_n = pin.get("log_n", int(rng.integers(1, 11)))
    size_i, size_o = int(rng.integers(1, 21)), int(rng.integers(1, 21))
    out_is_q = bool(rng.integers(0, 2))
    size_q, size_p = (size_o, size_i) if out_is_q else (size_i, size_o)
    m, _, special = C2._moduli(rng, log_n, size_q + size_p, 22)
    return dict(kind="scale_round", seed=seed, log_n=log_n, size_i=size_i, size_o=size_o, out_is_q=out_is_q,
                batch=int(rng.integers(1, 4)), q=m[:size_q], p=m[size_q:], special=special,
                data_seed=int(rng.integers(0, 1 << 31)))


def _switch_exact(rng, seed, pin):
    log_n = pin.get("log_n", 1 + seed if seed < 10 else int(rng.integers(1, 11)))
    # sources: one case in eight above the matrix-core kernel's 64, the rest spread over its K-step counts
    size_q = int(rng.integers(65, 81)) if rng.integers(0, 8) == 0 else int(rng.integers(1, 65))
    size_p = int(rng.integers(1, 33))
    q, _, _ = C2._moduli(rng, log_n, size_q, 22)
    if rng.integers(0, 3) == 0:  # every target 2^b - d, 54 .. 60 bits: the special-prime reduction
        p, _ = mixed_chain(log_n, [int(b) for b in rng.integers(54, 61, size=size_p)])
    else:
        p, _, _ = C2._moduli(rng, log_n, size_p, 22)
    if set(p) & set(q):
        return None
    kernel = KERNELS[int(rng.integers(0, 3))]
    if size_q > 16 and kernel == "BCONV_KERNEL_LIMB":
        kernel = "BCONV_KERNEL_AUTO"
    tiles, tpc = R.mma_tpc(size_q, size_p) if size_q <= 64 else (0, 1)
    return dict(kind="switch_exact", seed=seed, log_n=log_n, size_q=size_q, size_p=size_p,
                batch=int(rng.integers(1, 4)), kernel=kernel, q=q, p=p, ks=R.mma_ks(size_q) if size_q <= 64 else 0,
                chunks=-(-tiles // tpc), spq=R.mma_spq(p), data_seed=int(rng.integers(0, 1 << 31)))


_DRAW = {"rotation": _rotation, "bfv_mult": _bfv_mult, "scale_round": _scale_round, "switch_exact": _switch_exact}


def case(kind, seed):
    pin = PINS[kind].get(seed, {})
    for attempt in range(64):
        c = _DRAW[kind](np.random.default_rng([BASE[kind], seed, attempt]), seed, pin)
        if c is not None:
            c.update(kind=kind, attempt=attempt)
            return c
    raise AssertionError(f"no valid draw for {kind} seed {seed}")
