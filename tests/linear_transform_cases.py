"""Case data of tests/test_gpu_fuzz_linear_transform.py: the directed cases, the seeded draws and
the fixed grid of the BSGS linear transform's second test tier, as plain data.  Needs no GPU, so
tests/test_linear_transform_cases.py can check on the CPU that the cases reach what they are there
for.

launch_plan(baby, giant, n, beta) restates the host's chunking of ofhe_hip_ks_bsgs_transform
(csrc/keyswitch.hip) in a few lines, so that the CPU test can state what each case reaches; it is
not compared with the device.

case(seed) works as tier2_cases.case does (a draw that cannot be used is drawn again from the same
seed and the next attempt number; PINS fixes single parameters of a few seeds), and the helpers are
tier2_cases' own: keyswitch_draw, _moduli, valid_splits, valid_dnums and OFHE_FUZZ_SCALE."""
import numpy as np

import keyswitch as K
import linear_transform_ref as LT
import tier2_cases as C2
from test_gpu_linear_transform import EXTREME_CHAINS, _named_chain, nonid

SCALE = C2.SCALE
SEEDS = 48  # at scale 1
BASE = 45000  # disjoint from every BASE of tier2_cases, tier3_cases, behz_cases and decrypt_cases
KS_ROT_CAP = 16   # ofhe_hip.KS_ROT_CAP (csrc/ks_kernels.hpp); tests/test_gpu_fuzz_linear_transform.py asserts it
LT_SUM_CAP = 16   # csrc/lt_kernels.hpp: sums per launch of k_lt_inner
LT_TERM_CAP = 16  # and terms per sum (16 products per limb sum)
# words of the largest array of a drawn case (the diagonals, or the baby steps' outputs of one element)
# above which it takes fewer steps, then a smaller batch: tier3_cases.ROT_WORDS
LT_WORDS = 1 << 21


def launch_plan(baby, giant, n, beta):
    """What ofhe_hip_ks_bsgs_transform launches for these index lists at a level with beta digits."""
    ident = [LT.is_identity(k, n) for k in baby]
    runs, i = [], 0  # (first baby, length) of every k_ks_inner_rot call
    while i < len(baby):
        if ident[i]:
            i += 1
            continue
        m = 0
        while i + m < len(baby) and m < KS_ROT_CAP and not ident[i + m]:
            m += 1
        runs.append((i, m))
        i += m
    nid = sum(LT.is_identity(k, n) for k in giant)
    nrot = len(giant) - nid

    def inner(nsum):  # (g0, i0) of every k_lt_inner launch over nsum rows
        return [(g0, i0) for g0 in range(0, nsum, LT_SUM_CAP) for i0 in range(0, len(baby), LT_TERM_CAP)]

    outer = [min(KS_ROT_CAP, nrot - j0) for j0 in range(0, nrot, KS_ROT_CAP)] or [0]  # sets per k_lt_outer launch
    # k_lt_outer reduces its limb sums after every 16th product: inside a digit set unless beta divides 16 m
    mid_set = any((16 * m) % beta for ns in outer for m in range(1, ns * beta // 16 + 1))
    return dict(nrot=nrot, nid=nid, baby_runs=runs, term_chunks=-(-len(baby) // LT_TERM_CAP),
                sum_chunks_rot=-(-nrot // LT_SUM_CAP), sum_chunks_id=-(-nid // LT_SUM_CAP),
                inner_rot=inner(nrot), inner_id=inner(nid), outer=outer, first=len(outer),
                mod_down_polys=2 + nid, mid_set_reduction=mid_set)


# ---- A. directed cases of the fused call ---------------------------------------------------------
Q_BITS, P_BITS = [60, 22, 45, 31, 58], [59, 36, 60]  # the mixed chain the directed cases take their towers from


def _ks(n, count, start=0):
    return [nonid(n, r) for r in range(start, start + count)]


def _directed(name, log_n, baby, giant, present=None, absent_last=None, sq=4, sp=2, dnum=2, level=None, batch=2,
              t=0, pad=0, chain="mixed"):
    return dict(name=name, log_n=log_n, sq=sq, sp=sp, dnum=dnum, level=level or sq, batch=batch, baby=baby,
                giant=giant, present=present, absent_last=absent_last, t=t, pad=pad, chain=chain)


def _chunk_of_babies(nb, ng, first, last):
    """the diagonals of babies [first, last) of every giant"""
    return [j * nb + i for j in range(ng) for i in range(first, last)]


def _directed_cases():
    n3, n4 = 8, 16
    k3 = nonid(n3, 0)
    cs = []
    # A1: baby runs past KS_ROT_CAP, two and three term chunks
    cs.append(_directed("a1_babies_18", 3, _ks(n3, 18), [1, nonid(n3, 2)], absent_last=_chunk_of_babies(18, 2, 16, 18),
                        t=65537))
    cs.append(_directed("a1_babies_17_id_2", 4, [nonid(n4, 1)] * 17 + [1] + [nonid(n4, 2)] * 2, [1, nonid(n4, 0)],
                        absent_last=_chunk_of_babies(20, 2, 16, 20)))
    # giant 0 without its whole second term chunk, giant 1 without its whole first one
    present = [0 if 16 <= i < 32 else 1 for i in range(33)] + [0 if i < 16 else 1 for i in range(33)]
    cs.append(_directed("a1_babies_33", 3, _ks(n3, 33), [k3, 1], present=present,
                        absent_last=_chunk_of_babies(33, 2, 32, 33), t=65537))
    # A3: identity giants past the sum and addend caps
    cs.append(_directed("a3_giants_17_id", 3, [1, k3], [1 + 2 * n3 * j for j in range(17)], absent_last=[32, 33]))
    g = _ks(n4, 17)
    cs.append(_directed("a3_giants_17_rot_2_id", 4, [nonid(n4, 2), 1], g[:5] + [1] + g[5:12] + [2 * n4 + 1] + g[12:],
                        absent_last=[36, 37], t=65537))
    ids = [1 + 2 * n3 * j for j in range(17)]
    cs.append(_directed("a3_giants_2_rot_17_id", 3, [1, k3], ids[:4] + [nonid(n3, 1)] + ids[4:16] + [nonid(n3, 2)]
                        + ids[16:], absent_last=[36, 37]))
    # A4: three launches of k_lt_outer and k_lt_first, the last diagonal absent
    cs.append(_directed("a4_giants_33", 3, [1, k3], _ks(n3, 33), present=[1] * 65 + [0], absent_last=[64, 65],
                        t=65537))
    # sum chunks and term chunks in one call: g0 != 0 with i0 != 0 (acc = 1) in the fused call's k_lt_inner
    cs.append(_directed("a4_giants_17_babies_17", 3, [1] + _ks(n3, 16), _ks(n3, 17, 1),
                        absent_last=list(range(16 * 17, 17 * 17))))
    return cs


DIRECTED = _directed_cases()
# A5: the fused call with a runtime digit count and a reduction inside the fourth giant's digit set
FUSED_BETA5 = _directed("a5_fused_beta_5", 4, [1, nonid(16, 0)], _ks(16, 4, 1), sq=5, dnum=5, t=65537)
CHUNKED = [c["name"] for c in DIRECTED]  # every one of A1-A4 has a last chunk


def directed_seed(i):
    return 5000 + i


def chain_of(c):
    """(q, rq, p, rp) of a directed or grid case"""
    if c["chain"] == "mixed":
        return _named_chain(c["log_n"], Q_BITS[:c["sq"]], P_BITS[:c["sp"]])
    if c["chain"] == "grid":
        return grid_chain(c["log_n"])
    q, rq, p, rp = EXTREME_CHAINS[c["chain"]](c["log_n"])
    return q[:c["sq"]], rq[:c["sq"]], p[:c["sp"]], rp[:c["sp"]]


def params_of(c):
    q, rq, p, rp = chain_of(c)
    return K.KeySwitchParams(1 << c["log_n"], q, rq, p, rp, c["dnum"])


def build(c, Bsgs, ks, seed, **over):
    """The Bsgs (tests/test_gpu_linear_transform.py, passed in: this module stays off the device) of a
    directed case or a draw on engine ks; the same seed gives the same inputs wherever it is built."""
    c = {**c, **over}
    kp = params_of(c) if "chain" in c else K.KeySwitchParams(1 << c["log_n"], c["q"], c["rq"], c["p"], c["rp"],
                                                             c["dnum"])
    return Bsgs(np.random.default_rng(seed), ks, kp, kp.q, kp.p, c["level"], 1 << c["log_n"], c["dnum"], c["batch"],
                c["baby"], c["giant"], c["present"], pad=c["pad"])


def reference(bs, t=0, absent=()):
    """LT.bsgs_ref on the indices reduced mod 2N (the device gets them as they are); absent:
    diagonals marked absent on top of the case's own."""
    red = lambda ks: [k % (2 * bs.n) for k in ks]  # noqa: E731
    present = bs.present
    if absent:
        present = list(present) if present is not None else [1] * (len(bs.baby) * len(bs.giant))
        for d in absent:
            present[d] = 0
    return LT.bsgs_ref(bs.kp, bs.c0, bs.c1, red(bs.baby), red(bs.giant), bs.bkeys, bs.gkeys, bs.diag, present, t)


# ---- A2 / A5. the stage calls -------------------------------------------------------------------------
def stage_present(nterm, nsum):
    """A present pattern in which sums have all-absent term chunks: sum j lacks chunk j mod (chunks + 1)
    (none when that is past the last chunk), sum 3 and the last sum lack every diagonal, and every
    seventh diagonal is absent besides."""
    chunks = -(-nterm // LT_TERM_CAP)
    pr = []
    for j in range(nsum):
        for i in range(nterm):
            gone = i // LT_TERM_CAP == j % (chunks + 1) or j in (3, nsum - 1) or (j * nterm + i) % 7 == 0
            pr.append(0 if gone else 1)
    return pr


STAGE_SUMS = [(17, 17), (33, 17), (2, 33)]  # (nterm, nsum) of mult_ext_sum
# (Q = dnum = beta, digit sets) of fast_rotation_ext_sum at the largest limb sums
EXTREME_SETS = [(5, 3), (5, 4), (5, 7), (6, 3), (6, 6)]


def products_to_set_end(beta):
    """products k_lt_outer would sum in one limb sum if it reduced only where a digit set ends"""
    return -(-16 // beta) * beta


def top_limb_sum(mods, products):
    """the largest limb sum of that many products of words q_t - 1 (30-bit limbs, the high limbs' sum)"""
    return max(products * ((m - 1) >> 30) ** 2 for m in mods)


# ---- B. the seeded sweep ----------------------------------------------------------------------------------
PINS = {
    # N = 2^17 at full level with a k_cols split: the options that choose between k_bconv_cols and the unfused
    # conversion, in the batched ModDown over nrot * batch entries (as tier3_cases' rotation pins)
    14: {"log_n": 17, "split": "SPLIT_AUTO", "full_level": True, "separate_cols": 1, "separate_icol": 0},
    15: {"log_n": 17, "split": "SPLIT_COLS", "full_level": True, "separate_cols": 0, "separate_icol": 1},
    # 48 seeds hold two cases of each of the seven splits of 2^16 and 2^17 only with help
    33: {"log_n": 17, "split": "SPLIT_9_8"},
    # beta = 4, the widest templated k_lt_outer, with rotated giants a second time
    26: {"size_q": 8, "dnum": 4, "full_level": True, "giant_ids": "some"},
}
BABY_IDS = ("none", "first", "some")
GIANT_IDS = ("none", "first", "some", "all")
DENSITY = ("all", "half", "one", "none")


def _draw(rng, seed, pin):
    c = C2.keyswitch_draw(rng, seed, pin, "linear_transform")
    if c is None:
        return None
    log_n, sq, sp, l = c["log_n"], c["size_q"], c["size_p"], c["level"]
    n = 1 << log_n
    m, r, special = C2._moduli(rng, log_n, sq + sp, 22)  # 22 .. 60 bits in place of the key switch's 30 .. 60
    c.update(q=m[:sq], rq=r[:sq], p=m[sq:], rp=r[sq:], special=special)
    batch = pin.get("batch", int(rng.integers(1, 4)))
    nb, ng = pin.get("nbaby", int(rng.integers(1, 21))), pin.get("ngiant", int(rng.integers(1, 21)))
    words = lambda: max(nb * ng, nb * batch) * (l + sp) * n  # noqa: E731
    while words() > LT_WORDS and max(nb, ng) > 1:
        if nb >= ng:
            nb -= 1
        else:
            ng -= 1
    while words() > LT_WORDS and batch > 1:
        batch -= 1
    baby_ids = pin.get("baby_ids", BABY_IDS[int(rng.integers(0, 3))])
    giant_ids = pin.get("giant_ids", GIANT_IDS[int(rng.integers(0, 4))])
    unreduced = bool(rng.integers(0, 4) == 0)

    def indices(count, ids):
        out = []
        for i in range(count):
            k = 2 * int(rng.integers(1, n)) + 1  # odd, 3 .. 2N - 1
            if ids == "all" or (ids == "first" and i == 0) or (ids == "some" and rng.integers(0, 3) == 0):
                k = 1
            if unreduced and rng.integers(0, 2):
                k += 2 * n * int(rng.integers(1, (1 << 32) // (2 * n)))
            out.append(k)
        return out

    baby, giant = indices(nb, baby_ids), indices(ng, giant_ids)
    density = [DENSITY[int(rng.integers(0, 4))] for _ in range(ng)]
    present = []
    for d in density:
        row = {"all": [1] * nb, "half": [int(v) for v in rng.integers(0, 2, size=nb)], "none": [0] * nb}.get(d)
        if row is None:
            row = [0] * nb
            row[int(rng.integers(0, nb))] = 1
        present += row
    if all(present) and rng.integers(0, 2):
        present = None  # the NULL array: every diagonal present
    pad = (0, 0, 3, 8)[int(rng.integers(0, 4))]
    c.update(batch=batch, baby=baby, giant=giant, baby_ids=baby_ids, giant_ids=giant_ids, unreduced=unreduced,
             density=density, present=present, pad=pad)
    return c


def case(seed):
    pin = PINS.get(seed, {})
    for attempt in range(64):
        c = _draw(np.random.default_rng([BASE, seed, attempt]), seed, pin)
        if c is not None:
            c.update(attempt=attempt)
            return c
    raise AssertionError(f"no valid draw for seed {seed}")


# ---- C. the fixed grid on the large rings ------------------------------------------------------------------
GRID_RINGS = (13, 16, 17)


def grid_case(log_n, level):
    """4 + 2 mixed towers (60, 22, 45, 31 | 59, 36; 23 bits at N = 2^17, which has no 22-bit prime = 1 mod 2N
    below its first one), dnum 2, 2 x 2 steps with one identity in each list, one absent diagonal, batch 1"""
    n = 1 << log_n
    c = _directed(f"grid_{log_n}_{level}", log_n, [1, nonid(n, 0)], [nonid(n, 1), 2 * n + 1], present=[1, 1, 1, 0],
                  level=level, batch=1, t=65537 if level < 4 else 0)
    c["chain"] = "grid"
    return c


def grid_chain(log_n):
    narrow = 22 if log_n < 17 else 23
    return _named_chain(log_n, [60, narrow, 45, 31], [59, 36])


def grid_engines(log_n):
    """(split, generic_moduli, option) of every engine of the grid at this ring size"""
    es = [(s, g, None) for s in C2.valid_splits(log_n) for g in (0, 1)]
    if log_n == 17:
        es += [("SPLIT_AUTO", 0, "separate_cols"), ("SPLIT_AUTO", 0, "separate_icol")]
    return es


GRID = [(log_n, level, s, g, o) for log_n in GRID_RINGS for level in (4, 3) for s, g, o in grid_engines(log_n)]
