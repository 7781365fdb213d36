"""The lazy-reduction helpers of csrc/arith.hpp, csrc/ntt_kernels.hpp and
bm_reduce of csrc/bconv_mma.hpp, run on the device by tests/hip_arith (one
small kernel per helper, the project's headers included unchanged) and checked
word by word against Python integers.  No tolerance: every assertion is an
equality, a congruence or a strict range, each taken from the helper's own
comment.

Operands per helper and modulus: the extremes of the stated domain (0, 1,
k q - 1, k q, k q + 1 up to the top of the lazy range, 2^32 - 1, 2^32, values
whose low word borrows against the modulus, 2^63 and 2^64 - 1 where the
contract says "any 64-bit"), the twiddles 1, 2, q - 1, (q + 1) / 2, and seeded
uniform draws.  Moduli: boundary_cases.probe_moduli() -- the smallest the
library admits, the largest NTT prime below 2^60 at N = 2^17, sparse low words,
and every admitted prime at the kernel cut-offs.

Not on the shipped path (built with their switches off by default), covered
all the same: mulhi_approx<QA = true> and shoup_lazy<.., QA = true>, mont_mul2.

Each test prints "ARITH <helper> ..." lines with the largest r / q it saw;
DESIGN.md quotes them."""
import os
import random
import subprocess
import time

import numpy as np
import pytest
from conftest import ROOT

import boundary_cases as BC

M64 = (1 << 64) - 1
M32 = (1 << 32) - 1
BIG, SMALL = 2048, 128  # uniform draws per modulus: the named moduli and the N = 2^3 boundary primes / the rest


@pytest.fixture(scope="module")
def probe_bin():
    d = os.path.join(ROOT, "tests", "hip_arith")
    subprocess.run(["make", "-s", "-C", d], check=True)
    return os.path.join(d, "arith_probe_bin")


def test_arith_probe_builds(probe_bin):
    """The probe compiles against the library's headers (no device needed)
    and lists the helpers this module drives."""
    r = subprocess.run([probe_bin, "--list"], capture_output=True, text=True, timeout=60, check=True)
    names = {ln.split()[0] for ln in r.stdout.splitlines()}
    assert {"shoup_lazy_spq", "fold_spq", "canon_spq", "bm_reduce_lazy_spq_wide", "csub_s", "barrett128"} <= names


# ---- moduli ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def moduli(O):
    """[(name, q, draws)]"""
    out = []
    for name, q in BC.probe_moduli().items():
        big = not name.startswith(("ntt_", "mma_")) or "_n3_" in name
        out.append((name, q, BIG if big else SMALL))
    return out


def spq_sh(q):
    return q.bit_length() - 32 if BC.ntt_admits(q) else 0


def mod_k(q, k3=0, k4=0):
    """the probe's K for a Mod<SPQ>: (q, L - 32 or 0, 1, two helper-specific words)"""
    return [q, spq_sh(q), 1, k3, k4, 0, 0, 0]


# ---- operands -------------------------------------------------------------------------
def edges(q, bound):
    """extremes of [0, bound) for a helper whose ranges are multiples of q"""
    v = {0, 1, 2, M32 - 1, M32, M32 + 1, M32 + 2, bound - 1, bound - 2, bound >> 1}
    for k in range(0, 17):
        v |= {k * q - 1, k * q, k * q + 1}
    L = q.bit_length()
    for k in range(1, 17):  # around the bits fold_spq / canon_spq split at
        v |= {(k << L) - 1, k << L, (k << L) + 1}
    for m in (q, 2 * q, 4 * q, 8 * q):  # the low word borrows / does not borrow against m's
        hi, lo = m >> 32, m & M32
        for h in (hi - 1, hi, hi + 1, 2 * hi + 1):
            for l_ in (0, lo - 1, lo, lo + 1, M32):
                v.add((max(h, 0) << 32) | (l_ & M32))
    return sorted(x for x in v if 0 <= x < bound)


EDGE64 = [0, 1, 2, M32 - 1, M32, M32 + 1, (1 << 63) - 1, 1 << 63, (1 << 63) + 1, M64 - M32, M64 - M32 - 1,
          0x00000001FFFFFFFF, 0xFFFFFFFE00000001, M64 - 1, M64]


def twiddles(q):
    return [1, 2, q - 1, (q + 1) // 2]


def shoup_pre(w, q):
    return (w << 64) // q


def draws(rng, n, *bounds):
    return [[rng.randrange(b) for b in bounds] for _ in range(n)]


# ---- running the probe ------------------------------------------------------------------
def run_probe(probe_bin, tmp_path, helper, groups, out_words):
    """groups: [(K, tuples)]; returns the results per group as lists of tuples"""
    flat = [0x54495241454846, len(groups)]
    for K, tuples in groups:
        flat += [k & M64 for k in K] + [len(tuples)]
        for t in tuples:
            flat += [x & M64 for x in t]
    fin, fout = str(tmp_path / (helper + ".in")), str(tmp_path / (helper + ".out"))
    np.array(flat, dtype=np.uint64).tofile(fin)
    t0 = time.perf_counter()
    r = subprocess.run(["timeout", "-k", "10", "120", probe_bin, helper, fin, fout], capture_output=True, text=True)
    dt = time.perf_counter() - t0
    assert r.returncode == 0, f"{helper}: exit {r.returncode}\n{r.stdout}{r.stderr}"
    res = np.fromfile(fout, dtype=np.uint64).tolist()
    assert len(res) == out_words * sum(len(t) for _, t in groups)
    print(f"ARITH {helper}: {sum(len(t) for _, t in groups)} tuples, {len(groups)} launches, {dt:.2f} s")
    out, at = [], 0
    for _, tuples in groups:
        n = len(tuples) * out_words
        rows = res[at:at + n]
        out.append([tuple(rows[i:i + out_words]) for i in range(0, n, out_words)] if out_words > 1 else rows)
        at += n
    return out


def report(helper, ratio, where):
    print(f"ARITH {helper}: max r/q = {ratio:.9f} at {where}")


# ---- multiplies ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_mulhi_and_mul128(probe_bin, tmp_path):
    """mulhi_approx = floor(ab / 2^64) - e, e in {0, 1, 2} (0 is reached; the
    largest e seen is printed); mulhi_exact and mul128 are exact.  Any 64-bit
    operands."""
    rng = random.Random(101)
    ops = [[a, b] for a in EDGE64 for b in EDGE64] + draws(rng, 4096, 1 << 64, 1 << 64)
    ops += [[a, rng.randrange(1 << 64)] for a in EDGE64] + draws(rng, 512, 1 << 33, 1 << 64)
    K = [0, 0, 1, 0, 0, 0, 0, 0]
    for helper in ("mulhi_approx", "mulhi_approx_qa"):
        (res,) = run_probe(probe_bin, tmp_path, helper, [(K, ops)], 1)
        seen = set()
        for (a, b), r in zip(ops, res):
            e = ((a * b) >> 64) - r
            assert 0 <= e <= 2, (helper, hex(a), hex(b), hex(r), e)
            seen.add(e)
        print(f"ARITH {helper}: e values seen {sorted(seen)}, largest {max(seen)}")
        assert 0 in seen
    (res,) = run_probe(probe_bin, tmp_path, "mulhi_exact", [(K, ops)], 1)
    assert res == [(a * b) >> 64 for a, b in ops]
    (res,) = run_probe(probe_bin, tmp_path, "mul128", [(K, ops)], 2)
    assert res == [((a * b) & M64, (a * b) >> 64) for a, b in ops]


# ---- conditional subtracts ------------------------------------------------------------------
@pytest.mark.gpu
def test_csub(probe_bin, tmp_path, moduli):
    """csub(x, m) and csub_s(x, m) = x - m if x >= m else x, for any 64-bit x
    and the subtrahends the kernels use (q, 2q, 4q, 8q; csub also any m).
    csub_s gets m as a kernel argument: it must be wave-uniform."""
    rng = random.Random(102)
    want = lambda x, m: x - m if x >= m else x  # noqa: E731
    ops = [[x, m] for x in EDGE64 for m in EDGE64[1:]] + draws(rng, 2048, 1 << 64, 1 << 64)
    for _, q, _n in moduli:
        for m in (q, 2 * q, 4 * q, 8 * q):
            ops += [[x, m] for x in (m - 1, m, m + 1, (m & ~M32) | ((m - 1) & M32), m + (1 << 32) - 1, m ^ M32)]
    (res,) = run_probe(probe_bin, tmp_path, "csub", [([0] * 8, ops)], 1)
    assert res == [want(x, m) for x, m in ops]
    groups = []
    for _, q, n in moduli:
        for m in (q, 2 * q, 4 * q, 8 * q):
            xs = edges(q, 1 << 64) + EDGE64 + [rng.randrange(1 << 64) for _ in range(n // 4)]
            xs += [rng.randrange(2 * m) for _ in range(n // 4)]
            groups.append(([m] + [0] * 7, [[x] for x in xs]))
    res = run_probe(probe_bin, tmp_path, "csub_s", groups, 1)
    for (K, tuples), rows in zip(groups, res):
        assert rows == [want(x, K[0]) for (x,) in tuples], hex(K[0])


# ---- Shoup ------------------------------------------------------------------------------------
def shoup_groups(moduli, rng, spq_only):
    groups = []
    for _, q, n in moduli:
        if spq_only and not BC.ntt_admits(q):
            continue
        tw = twiddles(q) + [rng.randrange(q) for _ in range(4)]
        avals = EDGE64 + edges(q, 16 * q)[::7] + [q - 1, q, 4 * q - 1, 12 * q - 1, 16 * q - 1]
        t = [[a, w, shoup_pre(w, q), rng.choice(EDGE64 + [8 * q - 1, 12 * q - 1])] for a in avals for w in tw]
        for a, w, acc in draws(rng, n, 1 << 64, q, 12 * q):
            t.append([a, w, shoup_pre(w, q), acc])
        groups.append((mod_k(q), t))
    return groups


@pytest.mark.gpu
@pytest.mark.parametrize("qa", ["", "_qa"])
def test_shoup_lazy(probe_bin, tmp_path, moduli, qa):
    """shoup_lazy(a, w, w') == a w (mod q) and < 4q for ANY 64-bit a, w < q;
    shoup_lazy_acc == acc + shoup_lazy (mod 2^64); on special-form q the SPQ
    instantiation returns the generic one's words.  qa: the QA = true quotient
    (not on the shipped path)."""
    rng = random.Random(103)
    g_all = shoup_groups(moduli, rng, False)
    g_spq = [g for g in g_all if g[0][1]]
    assert len(g_spq) >= 35 and len(g_all) > len(g_spq)
    tri = lambda gs: [(K, [t[:3] for t in ts]) for K, ts in gs]  # noqa: E731
    gen = run_probe(probe_bin, tmp_path, "shoup_lazy" + qa, tri(g_all), 1)
    worst = (-1.0, "")
    for (K, ts), rows in zip(g_all, gen):
        q = K[0]
        for (a, w, _wp, _acc), r in zip(ts, rows):
            assert r < 4 * q and (r - a * w) % q == 0, (hex(q), hex(a), hex(w), hex(r))
            worst = max(worst, (r / q, hex(q)))
    report("shoup_lazy" + qa, *worst)
    spq = run_probe(probe_bin, tmp_path, "shoup_lazy_spq" + qa, tri(g_spq), 1)
    gen_spq = [rows for (K, _), rows in zip(g_all, gen) if K[1]]
    assert spq == gen_spq, "SPQ and generic shoup_lazy differ on a special-form modulus"
    if qa:
        return
    acc = run_probe(probe_bin, tmp_path, "shoup_lazy_acc", g_all, 1)
    for (K, ts), rows, base in zip(g_all, acc, gen):
        assert rows == [(t[3] + b) & M64 for t, b in zip(ts, base)], hex(K[0])
    acc_spq = run_probe(probe_bin, tmp_path, "shoup_lazy_acc_spq", g_spq, 1)
    assert acc_spq == [rows for (K, _), rows in zip(g_all, acc) if K[1]]


# ---- single-operand reductions --------------------------------------------------------------------
# helper -> (input bound in q (None: 2^(L+4)), output bound in q, special-form moduli only)
REDUCTIONS = {
    "fold_spq": (None, 2, True),
    "canon_spq": (None, 1, True),
    "canon4": (4, 1, False),
    "canon8": (8, 1, False),
    "canon_fwd": (16, 1, False),
    "canon_fwd_spq": (16, 1, True),
    "red8": (8, 4, False),
    "red8_spq": (8, 4, True),
    "red16": (16, 8, False),
    "red16_spq": (16, 8, True),
    "red16_gs": (16, 8, False),
    "red16_gs_spq": (16, 8, True),
}


@pytest.mark.gpu
@pytest.mark.parametrize("helper", sorted(REDUCTIONS))
def test_reductions(probe_bin, tmp_path, moduli, helper):
    """Same residue, result strictly below the bound the helper's comment
    states, over its whole stated input range: fold_spq / canon_spq any
    x < 2^(L+4) -> < 2q / < q; canon4 / canon8 / canon_fwd [0, 4q) / [0, 8q) /
    [0, 16q) -> [0, q); red8 [0, 8q) -> [0, 4q); red16, red16_gs [0, 16q) ->
    [0, 8q)."""
    in_q, out_q, spq_only = REDUCTIONS[helper]
    rng = random.Random(104)
    groups = []
    for _, q, n in moduli:
        if spq_only and not BC.ntt_admits(q):
            continue
        bound = in_q * q if in_q else 1 << (q.bit_length() + 4)
        xs = edges(q, bound) + [rng.randrange(bound) for _ in range(n)]
        xs += [bound - 1 - rng.randrange(1 << 20) for _ in range(16)]
        groups.append((mod_k(q), [[x] for x in xs]))
    assert len(groups) >= (35 if spq_only else 45)
    res = run_probe(probe_bin, tmp_path, helper, groups, 1)
    worst = (-1.0, "")
    for (K, ts), rows in zip(groups, res):
        q = K[0]
        for (x,), r in zip(ts, rows):
            assert r < out_q * q and (r - x) % q == 0, (helper, hex(q), hex(x), hex(r))
            worst = max(worst, (r / q, hex(q)))
    report(helper, *worst)


# ---- butterflies --------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("spq", ["", "_spq"])
def test_butterflies(probe_bin, tmp_path, moduli, spq):
    """ct_bfly_cs: (x + w y, x - w y) on residues; a CS stage takes
    [0, 16q) to [0, 12q), the others [0, 12q) to [0, 16q).  gs_bfly:
    (x + y, (x - y) w), [0, 4q) to [0, 4q).  Inputs include the top of each
    range (16q - 1, 12q - 1, 4q - 1) on both operands."""
    rng = random.Random(105)
    for helper, cs, in_q, out_q in (("ct_bfly_cs", 1, 16, 12), ("ct_bfly_cs", 0, 12, 16), ("gs_bfly", 0, 4, 4)):
        groups = []
        for _, q, n in moduli:
            if spq and not BC.ntt_admits(q):
                continue
            top = in_q * q
            ext = [0, 1, q - 1, q, top - q, top - 2, top - 1, (top - 1) & ~M32, ((top >> 32) << 32) - 1]
            ext = [x for x in ext if 0 <= x < top]
            ts = [[x, y, w, shoup_pre(w, q)] for x in ext for y in ext for w in twiddles(q)]
            ts += [[x, y, w, shoup_pre(w, q)] for x, y, w in draws(rng, n, top, top, q)]
            groups.append((mod_k(q, cs), ts))
        res = run_probe(probe_bin, tmp_path, helper + spq, groups, 2)
        worst = (-1.0, "")
        for (K, ts), rows in zip(groups, res):
            q = K[0]
            for (x, y, w, _), (rx, ry) in zip(ts, rows):
                if helper == "gs_bfly":
                    wx, wy = x + y, (x - y) * w
                else:
                    wx, wy = x + w * y, x - w * y
                assert rx < out_q * q and ry < out_q * q, (helper, cs, hex(q), hex(x), hex(y), hex(w), hex(rx), hex(ry))
                assert (rx - wx) % q == 0 and (ry - wy) % q == 0, (helper, cs, hex(q), hex(x), hex(y), hex(w))
                worst = max(worst, (max(rx, ry) / q, hex(q)))
        report(f"{helper}{spq} cs={cs}", *worst)


# ---- Barrett / Montgomery products -------------------------------------------------------------------
def barrett_ref_py(a, b, q):
    """NativeIntegerT::ModMulFastEq with mu = ComputeMu(): 2^(2 msb + 3) / q"""
    mb = q.bit_length()
    mu = (1 << (2 * mb + 3)) // q
    n = mb - 2
    prod = a * b
    est = ((((prod >> n) & M64) * mu) >> (n + 7)) & M64
    r = (prod - est * q) & M64
    return r - q if r >= q else r


@pytest.mark.gpu
def test_barrett_ref_and_mont_mul(probe_bin, tmp_path, moduli):
    """barrett_ref equals ModMulFastEq's formula and a b mod q for canonical
    a, b; mont_mul(a, b) == a b 2^-64 (mod q) in (0, 2q) for a < 12q, b < q
    (mont_mul2, not on the shipped path, likewise)."""
    rng = random.Random(106)
    gb, gm = [], []
    for _, q, n in moduli:
        mb = q.bit_length()
        ext = sorted({0, 1, 2, q - 2, q - 1, (q + 1) // 2, q >> 1, min(M32, q - 1), min(M32 + 1, q - 1)})
        ts = [[a, b] for a in ext for b in ext] + draws(rng, n, q, q)
        gb.append((mod_k(q, (1 << (2 * mb + 3)) // q, mb - 2), ts))
        exta = sorted(set(ext) | {q, 4 * q - 1, 8 * q, 12 * q - 1, 12 * q - 2, (12 * q - 1) & ~M32})
        tm = [[a, b] for a in exta for b in ext] + draws(rng, n, 12 * q, q)
        gm.append((mod_k(q, pow(q, -1, 1 << 64)), tm))
    res = run_probe(probe_bin, tmp_path, "barrett_ref", gb, 1)
    for (K, ts), rows in zip(gb, res):
        q = K[0]
        assert rows == [barrett_ref_py(a, b, q) for a, b in ts], hex(q)
        assert rows == [a * b % q for a, b in ts], hex(q)
    for helper in ("mont_mul", "mont_mul2"):
        res = run_probe(probe_bin, tmp_path, helper, gm, 1)
        worst = (-1.0, "")
        for (K, ts), rows in zip(gm, res):
            q = K[0]
            for (a, b), r in zip(ts, rows):
                assert 0 < r < 2 * q and ((r << 64) - a * b) % q == 0, (helper, hex(q), hex(a), hex(b), hex(r))
                worst = max(worst, (r / q, hex(q)))
        report(helper, *worst)


def barrett128_py(a, m):
    """BarrettUint128ModUint64 step by step: (result, iterations of its final loop)"""
    mu = ((1 << 128) - 1) // m  # floor(2^128 / m) for odd m, as the host computes it
    a_lo, a_hi, mu_lo, mu_hi = a & M64, a >> 64, mu & M64, mu >> 64
    left_hi = (a_lo * mu_lo) >> 64
    mid = a_lo * mu_hi
    tmp1 = ((mid & M64) + left_hi) & M64
    tmp2 = ((mid >> 64) + (1 if tmp1 < (mid & M64) else 0)) & M64
    mid = a_hi * mu_lo
    s = ((mid & M64) + tmp1) & M64
    left_hi = ((mid >> 64) + (1 if s < (mid & M64) else 0)) & M64
    tmp1 = (a_hi * mu_hi + tmp2 + left_hi) & M64
    r = (a_lo - tmp1 * m) & M64
    it = 0
    while r >= m:
        r -= m
        it += 1
        assert it <= 8
    return r, it


@pytest.mark.gpu
def test_barrett128(probe_bin, tmp_path, moduli):
    """barrett128(a, m) = a mod m, canonical.  Input range, read off the
    callers: the base-conversion kernels (k_bconv, k_bconv_wide, the BFV and
    BEHZ exact switches) reduce sums of at most 256 products y c with
    y < q_i < 2^60 and c < m (size_q <= 256): a < 2^68 m; the key-switch inner
    products sum at most 256 products of two residues below m.  Both lie in
    [0, 2^128), which is tested whole, with the sub-range a < 2^68 m drawn
    separately.  The final subtract loop's trip count is taken from a
    step-by-step Python restatement BEFORE anything is launched (at most 8)."""
    rng = random.Random(107)
    groups = []
    for _, q, n in moduli:
        cap = min(1 << 128, q << 68)
        ext = [0, 1, q - 1, q, q + 1, M64, 1 << 64, (1 << 64) + 1, q << 64, (q << 64) - 1, cap - 1, (1 << 128) - 1,
               (1 << 127), q * q - 1, 256 * (q - 1) * ((1 << 60) - 1)]
        ext = [a for a in ext if a < (1 << 128)]
        avals = ext + [rng.randrange(cap) for _ in range(n)] + [rng.randrange(1 << 128) for _ in range(n)]
        assert max(barrett128_py(a, q)[1] for a in avals) <= 8
        mu = ((1 << 128) - 1) // q
        groups.append((mod_k(q, mu & M64, mu >> 64), [[a & M64, a >> 64] for a in avals]))
    res = run_probe(probe_bin, tmp_path, "barrett128", groups, 1)
    for (K, ts), rows in zip(groups, res):
        assert rows == [((hi << 64) | lo) % K[0] for lo, hi in ts], hex(K[0])


def switch_modulus_py(v, om, nm):
    """NativeVectorT::SwitchModulus of one value"""
    half = om >> 1
    if nm > om:
        return v + (nm - om) if v > half else v
    if v > half:
        v += nm - om % nm
    return v % nm if v >= nm else v


@pytest.mark.gpu
def test_switch_mod1(probe_bin, tmp_path, moduli):
    """switch_mod1 against NativeVectorT::SwitchModulus's three branches: new
    modulus larger; smaller with old <= 2 new (two conditional subtracts);
    smaller in general (the remainder)."""
    rng = random.Random(108)
    qs = sorted({q for _, q, _ in moduli})
    pairs = [(qs[0], qs[-1]), (qs[-1], qs[0]), (qs[-1], qs[-2]), (qs[-2], qs[-1]), (qs[-1], qs[-1])]
    pairs += [(qs[-1], (qs[-1] + 1) // 2 + 8), (qs[-1], (qs[-1] >> 1) - 7), (qs[-1], 2), (3, qs[-1])]
    pairs += [tuple(rng.sample(qs, 2)) for _ in range(40)]
    branches = set()
    groups = []
    for om, nm in pairs:
        branches.add("up" if nm > om else "small" if om <= 2 * nm else "general")
        half = om >> 1
        ext = {0, 1, half - 1, half, half + 1, om - 2, om - 1, nm - 1, nm, nm + 1, om - nm, om - nm + 1, M32, M32 + 1}
        vs = sorted(v for v in ext if 0 <= v < om) + [rng.randrange(om) for _ in range(256)]
        groups.append(([om, nm] + [0] * 6, [[v] for v in vs]))
    assert branches == {"up", "small", "general"}
    res = run_probe(probe_bin, tmp_path, "switch_mod1", groups, 1)
    for (K, ts), rows in zip(groups, res):
        assert rows == [switch_modulus_py(v, K[0], K[1]) for (v,) in ts], (hex(K[0]), hex(K[1]))


# ---- bm_reduce ----------------------------------------------------------------------------------
def bm_red_consts(p, spq):
    """BmRed as bconv_mma_table fills it: (p, 2^64 - p, r60, r60', mu1, blo, bhi, 2p)"""
    r60 = (1 << 60) % p
    r60p = (r60 << 64) // p
    mu1 = (1 << 64) // p
    bias = (((1 << 80) + p - 1) // p) * p
    bhi = (bias >> 32) - (1 << 16)
    blo = (bias & M32) + (1 << 48)
    if spq:
        L = p.bit_length()
        r60 = (1 << L) - p
        r60p = (L - 32) | (((1 << (L - 32)) - 1) << 32)
    return [p, (1 << 64) - p, r60, r60p, mu1, blo, bhi, 2 * p]


@pytest.mark.gpu
@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("spq", [False, True])
@pytest.mark.parametrize("lazy", [False, True])
def test_bm_reduce(probe_bin, tmp_path, moduli, lazy, spq, wide):
    """bm_reduce<LAZY, SPQ, WIDE>(C) == sum_b C_b 2^(8b) (mod p): canonical, or
    below 4p when LAZY, for |C_b| up to AND INCLUDING the stated cap (2^22,
    2^23 when WIDE), both signs, all eight at the cap together.  SPQ runs on
    the targets mma_admits passes (the admitted boundary primes among them),
    with the constants bconv_mma_table builds for them; the generic reduction
    on every modulus."""
    rng = random.Random(109)
    cap = 1 << (23 if wide else 22)
    fixed = [[s * c] * 8 for s in (1, -1) for c in (0, 1, cap - 1, cap)]
    for hi_sign in (1, -1):  # the two halves at opposite extremes, and alternating signs
        fixed.append([hi_sign * cap] * 4 + [-hi_sign * cap] * 4)
        fixed.append([hi_sign * cap * (-1) ** b for b in range(8)])
    for b in range(8):  # one digit at the cap, the rest zero / at the opposite cap
        for s in (1, -1):
            fixed.append([s * cap if i == b else 0 for i in range(8)])
            fixed.append([s * cap if i == b else -s * cap for i in range(8)])
    groups = []
    for _, p, n in moduli:
        if spq and not BC.mma_admits(p):
            continue
        ts = fixed + [[rng.randint(-cap, cap) for _ in range(8)] for _ in range(n)]
        ts += [[rng.choice((-cap, cap, rng.randint(-cap, cap))) for _ in range(8)] for _ in range(n // 2)]
        groups.append((bm_red_consts(p, spq), ts))
    assert len(groups) >= (9 if spq else 45)
    helper = "bm_reduce" + ("_lazy" if lazy else "") + ("_spq" if spq else "") + ("_wide" if wide else "")
    res = run_probe(probe_bin, tmp_path, helper, groups, 1)
    worst = (-1.0, "")
    for (K, ts), rows in zip(groups, res):
        p = K[0]
        for C, r in zip(ts, rows):
            want = sum(c << (8 * b) for b, c in enumerate(C)) % p
            if lazy:
                assert r < 4 * p and (r - want) % p == 0, (helper, hex(p), C, hex(r))
            else:
                assert r == want, (helper, hex(p), C, hex(r), hex(want))
            worst = max(worst, (r / p, hex(p)))
    report(helper, *worst)
