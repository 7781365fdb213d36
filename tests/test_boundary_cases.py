"""CPU checks of tests/boundary_cases.py: the moduli that
tests/test_gpu_boundary.py and tests/test_gpu_arith.py run sit where they are
meant to -- one prime on each side of every admission inequality, at every ring
dimension and size listed, each within one prime step of the threshold.

Both predicates are restated here a second time, straight from the host code
(ofhe_hip.hip: plan creation and bconv_mma_table), in the C expressions' own
terms (msb, the high word compared with all-ones, 128-bit products), so that a
slip in boundary_cases' arithmetic form does not go unnoticed."""
import pytest

import boundary_cases as BC
import oracle as O


def host_ntt_spq(qt):
    """spq of build() in ofhe_hip_plan_create_ex"""
    mb = qt.bit_length()
    return (mb >= 33 and (qt >> 32) == (1 << (mb - 32)) - 1 and (qt & 0xFFFFFFFF) != 0 and
            ((((1 << mb) - qt) << 4) & ((1 << 64) - 1)) < qt)


def host_mma_spq(p):
    """spq of bconv_mma_table for one target"""
    L = p.bit_length()
    d = (1 << L) - p if 33 <= L <= 60 else 0
    return d != 0 and d < (1 << 32) and ((1 << (81 - L)) + 1) * d + (1 << 49) + 2 * d < (1 << L)


HOST = {"ntt": host_ntt_spq, "mma": host_mma_spq}
# (predicate, log N, L) without an admitted prime: proved by enumeration in test_no_case_dropped
EMPTY = {("mma", 16, 50)}


def is_prime(x):
    return O.next_prime(x - 2, 2) == x  # NextPrime(x - 2, 2) starts at x


@pytest.mark.parametrize("pred", ["ntt", "mma"])
def test_one_prime_on_each_side(pred):
    """every ring dimension and every L has an admitted and a refused prime of
    exactly L bits, = 1 mod 2N, classified alike by both restatements"""
    rows = BC.cases(pred)
    rings, ls = (BC.NTT_RINGS, BC.NTT_LS) if pred == "ntt" else (BC.MMA_RINGS, BC.MMA_LS)
    assert [(lg, L) for lg, L, _, _ in rows] == [(lg, L) for lg in rings for L in ls]
    for lg, L, adm, ref in rows:
        m = 2 << lg
        assert ref is not None
        assert (adm is None) == ((pred, lg, L) in EMPTY), (pred, lg, L)
        for q, want in ((adm, True), (ref, False)):
            if q is None:
                continue
            assert q.bit_length() == L and q % m == 1 and is_prime(q), (pred, lg, L, q)
            assert BC.PREDICATES[pred](q) == want and HOST[pred](q) == want, (pred, lg, L, q)
            assert O.root_of_unity(m, q) != 0


@pytest.mark.parametrize("pred", ["ntt", "mma"])
def test_within_one_prime_step_of_the_threshold(pred):
    """No prime of the residue class lies between a chosen prime and the
    threshold: the admitted one is the first prime above the largest refused
    value 2^L - d_thr, the refused one the last prime at or below it; and d_thr
    itself is the exact threshold of both restatements."""
    for lg, L, adm, ref in BC.cases(pred):
        m = 2 << lg
        d_thr = BC.d_threshold(pred, L)
        for f in (BC.PREDICATES[pred], HOST[pred]):
            assert not f((1 << L) - d_thr) and (d_thr == 1 or f((1 << L) - (d_thr - 1))), (pred, L)
        lo = (ref if ref is not None else 0) + m
        hi = adm if adm is not None else 1 << L
        assert lo - m <= (1 << L) - d_thr < hi
        # every value of the class strictly between the two is composite
        between = range(lo, hi, m)
        assert len(between) < 20000
        assert not any(is_prime(x) for x in between), (pred, lg, L)


def test_reach():
    """L = 33 and L = 60 are present, and each limiting term of the NTT
    predicate is the binding one somewhere: refused primes that fail 16 d < q
    alone (L = 33..36) and ones that fail d < 2^32 alone (L >= 37)."""
    assert {33, 60} <= set(BC.NTT_LS) and {50, 60} <= set(BC.MMA_LS)
    binding = set()
    for _lg, _L, _adm, ref in BC.cases("ntt"):
        t = BC.ntt_terms(ref)
        assert list(t.values()).count(False) == 1, "exactly one term refuses a boundary prime"
        binding.add(next(k for k, v in t.items() if not v))
    assert binding == {"16d<q", "d<2^32"}
    # the admitted primes come within a few prime steps of 2.0 q in fold_spq: q + 16 d - 1 over q
    tight = max((q + 16 * ((1 << L) - q) - 1) / q for _lg, L, q, _ in BC.cases("ntt") if L == 33)
    assert tight > 1.9999


def test_no_case_dropped():
    """The only empty slot is the admitted side of the matrix-core predicate at
    N = 2^16, L = 50: d < 2^18 there, and 2^50 - d = 1 mod 2^17 leaves d = 2^17 - 1
    and 2^18 - 1, both composite.  The GPU tests' tower pairs and target sets cover
    every L listed."""
    for pred, lg, L in EMPTY:
        m = 2 << lg
        cands = [d for d in range(1, BC.d_threshold(pred, L)) if ((1 << L) - d) % m == 1]
        assert cands == [m - 1, 2 * m - 1] and not any(is_prime((1 << L) - d) for d in cands)
    import test_gpu_boundary as G

    assert {L for pair in G.NTT_PAIRS for L in pair} == set(BC.NTT_LS)
    for lg in BC.MMA_RINGS:
        assert G.mma_ls(lg) == [L for L in BC.MMA_LS if ("mma", lg, L) not in EMPTY]
        assert G.bconv_whiches(lg) == ["adm"] + [f"ref{L}" for L in G.mma_ls(lg)]
        for which in G.bconv_whiches(lg):
            p = G.mma_targets(lg, which)
            assert [BC.mma_admits(v) for v in p].count(False) == (0 if which == "adm" else 1)
    for lg in BC.NTT_RINGS:
        for pair in G.NTT_PAIRS:
            for form in G.FORMS:
                q = G.ntt_towers(lg, pair, form)
                assert all(BC.ntt_admits(v) for v in q) == (form in ("spq", "forced"))


def test_probe_moduli():
    """the probe's moduli: the 22-bit minimum, the largest 60-bit NTT prime at
    N = 2^17, sparse low words, and every admitted boundary prime"""
    pm = BC.probe_moduli()
    assert pm["min22"].bit_length() == 22 and pm["top60_n17"].bit_length() == 60
    assert pm["top60_n17"] == O.moduli_chain(17, 1)[0][0]
    assert pm["sparse59"] >> 59 == 1 and bin(pm["sparse59"]).count("1") <= 6
    assert pm["sparse_lo1"] & 0xFFFFFFFF == 1
    adm = {q for pred in ("ntt", "mma") for _, _, q, _ in BC.cases(pred) if q is not None}
    assert adm <= set(pm.values())
    assert all(is_prime(q) for q in pm.values())
