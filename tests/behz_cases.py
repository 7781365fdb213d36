"""Case generator of tests/test_gpu_fuzz_behz.py: the seeded draws of the BFV
(BEHZ) fuzz, its fixed shapes past the kernels' caps and the synthetic tables of
its extreme-sum cases, as plain data.  Needs no GPU, so
tests/test_behz_cases.py can check on the CPU that the committed seed range and
the fixed inputs reach what the GPU file is there for.

case(seed) works as tier3_cases.case does (a draw that cannot be used is drawn
again from the same seed and the next attempt number; PINS fixes single
parameters of a few seeds), and the helpers are tier2_cases' own: _moduli,
_log_n, _plan_options, valid_splits and OFHE_FUZZ_SCALE."""
import numpy as np

import behz_ref as Z
import bfv_ref as BR
import bfv_tables as BT
import oracle as O
import tier2_cases as C2
from test_mixed_moduli_oracle import mixed_chain

SCALE = C2.SCALE
SEEDS = 40  # at scale 1
BASE = 39000  # disjoint from every tier2_cases.BASE and tier3_cases.BASE
MODES = ("BEHZ_AUTO", "BEHZ_FUSED", "BEHZ_TWO_LAUNCHES")  # ofhe_hip.BEHZ_*: ofhe_hip_behz_floor_sk's `fused`
FUSED_MAX_B = Z.FUSED_MAX_B  # ofhe_hip.BEHZ_FUSED_MAX_B; tests/test_gpu_fuzz_behz.py asserts they agree
LIMB_QMAX = 16  # BCONV_LIMB_QMAX (csrc/eltwise_kernels.hpp): most sources of k_behz_q_to_bsk_limb
FAST_LOG_N = 13  # behz_ref's word path from this ring size up, as tests/test_gpu_fuzz_tier3.py

PINS = {
    # mixed-size chains past both caps on a small ring: more than 16 sources (k_behz_q_to_bsk's 128-bit sums
    # inside expand) with a fused floor -> SK, and more than 16 B towers (the multiplication's two-launch branch)
    # (BEHZ_FUSED with 18 B towers: floor_sk must refuse it)
    3: {"log_n": 5, "batch": 2, "sizes": (17, 18), "eval_form": True, "mode": "BEHZ_FUSED"},
    4: {"log_n": 6, "batch": 2, "sizes": (18, 16), "eval_form": True},
    # a tower below 32 bits next to one of 60 in q, and a 60-bit msk: q towers below msk / 2
    18: {"log_n": 8, "size_q": 3, "bits": [24, 60, 45, 52, 31, 60, 60]},
    19: {"log_n": 11, "size_q": 4, "bits": [60, 27, 30, 58, 60, 22, 41, 60]},
}


def _draw(rng, seed, pin):
    log_n = C2._log_n(rng, seed, 1, pin)
    # the CPU reference works with Python integers: fewer towers and entries on the large rings
    qmax, bmax = (2, 1) if log_n >= 15 else (3, 2) if log_n >= FAST_LOG_N else (6, 3)
    size_q = pin.get("size_q", int(rng.integers(1, qmax + 1)))
    size_b = max(1, size_q + int(rng.integers(-1, 2)))
    batch = pin.get("batch", int(rng.integers(1, bmax + 1)))
    plans = {"plan_q": C2._plan_options(rng, seed, log_n, pin)}
    for name in ("plan_bsk", "plan_qbsk"):  # separate handles: their options are drawn, not rotated with the seed
        plans[name] = pin.get(name, C2._plan_options(rng, 1, log_n, {}))
    eval_form = pin.get("eval_form", bool(rng.integers(0, 2)))
    mode = pin.get("mode", MODES[int(rng.integers(0, 3))])
    if "sizes" in pin:
        size_q, size_b = pin["sizes"]
        bits = [int(v) for v in rng.integers(22, 61, size=size_q + size_b + 1)]
    else:
        bits = pin.get("bits")
    if bits is not None:
        size_b = len(bits) - size_q - 1
        generic = bool(seed % 2)  # special and generic form alternate with the seed, as tier3_cases._pinned_moduli
        m, r = mixed_chain(log_n, bits, generic=generic)
        special = [not generic] * len(bits)
    else:
        m, r, special = C2._moduli(rng, log_n, size_q + size_b + 1, 22)
    if len(set(m)) != len(m):  # ofhe_hip_behz_create refuses a repeated modulus
        return None
    return dict(seed=seed, log_n=log_n, size_q=size_q, size_b=size_b, batch=batch, plans=plans, eval_form=eval_form,
                mode=mode, q=m[:size_q], rq=r[:size_q], b=m[size_q:size_q + size_b], msk=m[size_q + size_b],
                special=special, data_seed=int(rng.integers(0, 1 << 31)))


def case(seed):
    pin = PINS.get(seed, {})
    for attempt in range(64):
        c = _draw(np.random.default_rng([BASE, seed, attempt]), seed, pin)
        if c is not None:
            c["attempt"] = attempt
            return c
    raise AssertionError(f"no valid draw for seed {seed}")


def tables(c):
    return BT.BehzTables(c["q"], c["b"], c["msk"], Z.T_PLAIN)


def uniform(rng, moduli, batch, n):
    return np.stack([np.stack([rng.integers(0, int(m), size=n, dtype=np.uint64) for m in moduli])
                     for _ in range(batch)])


_standalone = {}


def standalone_inputs(c):
    """(xq [batch][Q][n], xqb [batch][Q + Bsk][n], xb [batch][Bsk][n]) of one case, built as behz_ref.case builds
    them from the case's data seed: the first min(4, batch n) coefficients of the flattened (batch, n) order planted
    with r = R_TARGETS (xq) and alpha = alpha_targets(msk) (xb), the rest uniform; with more than 8 coefficients the
    seed is advanced until the unplanted ones hold both sides of r >= 2^15 and both signs of the centred alpha"""
    if c["seed"] in _standalone:
        return _standalone[c["seed"]]
    T, n, batch, fast = tables(c), 1 << c["log_n"], c["batch"], c["log_n"] >= FAST_LOG_N
    planted = min(len(Z.R_TARGETS), batch * n)
    for salt in range(64):
        rng = np.random.default_rng([c["data_seed"], salt])
        xq, xqb, xb = (uniform(rng, mods, batch, n) for mods in (T.q, T.q + T.bsk, T.bsk))
        if batch * n <= 8:
            break
        r = Z.q_to_bsk(xq, T, want_r=True, fast=fast)[1].reshape(-1)[planted:]
        a = Z.conv_sk(xb, T, want_alpha=True, fast=fast)[1].reshape(-1)[planted:]
        if (r >= 0x8000).any() and (r < 0x8000).any() and (a > T.msk // 2).any() and (a <= T.msk // 2).any():
            break
    else:
        raise AssertionError(f"no inputs with both signs for seed {c['seed']}")
    for k in range(planted):
        xq[k // n, :, k % n] = Z.plant_r(T, xq[k // n, :, k % n], Z.R_TARGETS[k], rng)
        xb[k // n, :, k % n] = Z.plant_alpha(T, Z.alpha_targets(T.msk)[k], rng)
    _standalone[c["seed"]] = (xq, xqb, xb)
    return _standalone[c["seed"]]


# ---- the multiplication past the caps -------------------------------------------------------------------
# (size_q, size_b): 17 sources take k_behz_q_to_bsk (128-bit sums) inside expand, 17 B towers the two-launch branch
PAST_CAPS = [(17, 17), (17, 16), (16, 17)]
PAST_LOG_N = (5, 10)
PAST_BATCH = 3
_past = {}


def past_caps_case(sq, sb, log_n):
    """dict of one past-the-caps shape, built once: T, ring, the secret s and plaintexts ms of batch entry 0 (a real
    encryption; entries 1 and 2 are uniform towers), cts = [c0, c1, d0, d1] each [3][Q][n], and want, the three
    reference outputs (exact integers).  60-bit chain of sq + sb + 1 towers split as behz_ref's "uneven" case; at
    (17, 17) B and msk are behz_bases' choice."""
    key = (sq, sb, log_n)
    if key in _past:
        return _past[key]
    m, r = O.moduli_chain(log_n, sq + sb + 1)
    q, rq, b, msk = m[:sq], r[:sq], m[sq:sq + sb], m[sq + sb]
    if sq == sb:
        b, msk, _ = Z.behz_bases(O, log_n, q, Z.T_PLAIN)
    T = BT.BehzTables(q, b, msk, Z.T_PLAIN)
    ring = Z.Ring(O, log_n, T, rq)
    rng = np.random.default_rng([900, sq, sb, log_n])
    n = 1 << log_n
    s = np.array([int(v) for v in rng.integers(-1, 2, size=n)], dtype=object)
    ms = [np.array([int(v) for v in rng.integers(0, Z.T_PLAIN, size=n)], dtype=object) for _ in range(2)]
    cts = list(BR.encrypt(O, rng, ms[0], s, q, ring.tb_q, Z.T_PLAIN)) + \
        list(BR.encrypt(O, rng, ms[1], s, q, ring.tb_q, Z.T_PLAIN))
    cts = [np.concatenate([c, uniform(rng, q, PAST_BATCH - 1, n)]) for c in cts]
    _past[key] = dict(T=T, ring=ring, s=s, ms=ms, cts=cts, want=Z.eval_mult_behz(O, T, ring, *cts))
    return _past[key]


# ---- synthetic tables: the largest sums the kernels can be handed ---------------------------------------------
class SynthTables:
    """The attributes of bfv_tables.BehzTables with tables no real basis has: the twists (tQHatInvModq,
    mtildeQHatInvModq, BHatInvModb) are 1, so y = x and z = x, and every multiplier is its column's modulus
    minus 1 (0xFFFF mod mtilde): with x = modulus - 1 every sum is the largest its kernel can meet.  The
    moduli need be neither prime nor coprime; only the standalone calls (no plans) make sense on it."""

    TABLES = BT.BehzTables.TABLES
    flat = BT.BehzTables.flat

    def __init__(self, q, b, msk, t=Z.T_PLAIN):
        self.q, self.b, self.msk, self.t = [int(v) for v in q], [int(v) for v in b], int(msk), int(t)
        self.bsk = self.b + [self.msk]
        nq, nb = len(self.q), len(self.b)
        self.tQHatInvModq, self.mtildeQHatInvModq, self.BHatInvModb = [1] * nq, [1] * nq, [1] * nb
        self.QHatModbsk = [[m - 1 for m in self.bsk] for _ in range(nq)]
        self.qInvModbsk = [[m - 1 for m in self.bsk] for _ in range(nq)]
        self.BHatModq = [[m - 1 for m in self.q] for _ in range(nb)]
        self.BHatModmsk = [self.msk - 1] * nb
        self.QModbsk = [m - 1 for m in self.bsk]
        self.mtildeInvModbsk = [m - 1 for m in self.bsk]
        self.tQInvModbsk = [m - 1 for m in self.bsk]
        self.BModq = [m - 1 for m in self.q]
        self.BInvModmsk = self.msk - 1
        self.QHatModmtilde = [0xFFFF] * nq
        self.negQInvModmtilde = 0xFFFF


TOP = (1 << 60) - 1
# all-large: (size_q, size_b, log_n); moduli 2^60 - 1 - 2k, q first, then B, then msk.  16 sources are the limb
# kernel's most (its a1 + a2 carries, a3 = 2^64 - 2^35 + 16), 17 the first of the 128-bit sums, 255 their limit;
# 2^9 coefficients are two workgroups
ALL_LARGE = [(1, 1, 5), (15, 15, 5), (16, 16, 5), (17, 17, 5), (16, 40, 5), (64, 3, 5), (255, 255, 5), (16, 16, 9)]
# spread, 8 + 8 towers: the smallest moduli ofhe_hip_behz_create admits (3 in q, 65537 in Bsk) and ones just
# above 2^31 / 2^32 next to the largest.  A modulus may not repeat in one handle, so 2^32 + 15 is in Bsk in the
# first case (q holds 2^32 + 17) and in q in the second (Bsk holds 2^32 + 17)
W32 = (1 << 32) + 15
SPREAD_Q = [3, (1 << 31) + 1, W32 + 2, TOP - 2, 5, (1 << 44) + 3, (1 << 59) + 3, (1 << 20) + 7]
SPREAD_B = [65537, W32, (1 << 45) + 7, (1 << 59) + 1, (1 << 52) + 1, 65539, (1 << 33) + 1, (1 << 22) + 1]
SPREAD = {"spread": (SPREAD_Q, SPREAD_B, TOP),  # msk the largest modulus there is
          # msk the smallest, below most of q
          "spread-msk": (SPREAD_Q[:2] + [W32] + SPREAD_Q[3:], [TOP, W32 + 2] + SPREAD_B[2:], 65537)}
MAX_SUM_IDS = [f"{sq}-{sb}" + ("" if log_n == 5 else f"-n{log_n}") for sq, sb, log_n in ALL_LARGE] + list(SPREAD)
_max_sum = {}


def max_sum_case(name):
    """(T, log_n, xq, xqb, xb), batch 1: the modulus minus 1 in every tower at the even coefficients, uniform at
    the odd ones"""
    if name in _max_sum:
        return _max_sum[name]
    if name in SPREAD:
        q, b, msk = SPREAD[name]
        log_n = 5
    else:
        sq, sb, log_n = ALL_LARGE[MAX_SUM_IDS.index(name)]
        q = [TOP - 2 * k for k in range(sq)]
        b = [TOP - 2 * (sq + k) for k in range(sb)]
        msk = TOP - 2 * (sq + sb)
    T = SynthTables(q, b, msk)
    n = 1 << log_n
    rng = np.random.default_rng([41000, MAX_SUM_IDS.index(name)])
    xs = []
    for mods in (T.q, T.q + T.bsk, T.bsk):
        x = uniform(rng, mods, 1, n)
        x[0, :, 0::2] = (np.array(mods, dtype=np.uint64) - np.uint64(1))[:, None]
        xs.append(x)
    _max_sum[name] = (T, log_n) + tuple(xs)
    return _max_sum[name]
