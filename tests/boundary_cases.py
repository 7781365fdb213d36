"""Moduli at the cut-offs by which the host code picks a kernel instantiation,
as plain data (no GPU): tests/test_boundary_cases.py checks on the CPU that the
primes sit where they should, tests/test_gpu_boundary.py and
tests/test_gpu_arith.py run them.

Two predicates, restated from the host code (both on q = 2^L - d, L = the bit
length of q):

  ntt_admits  (ofhe_hip.hip, plan creation: TowerConst.spq_sh != 0, the
              special-prime NTT kernels when every tower of the plan passes):
              L >= 33, d < 2^32, lo32(q) != 0, 16 d < q.  (lo32(q) != 0 only
              excludes d = 2^32, an even q: no prime can test it.)
  mma_admits  (ofhe_hip.hip, bconv_mma_table: bm_reduce<.., SPQ> when every
              target of the converter passes): 33 <= L <= 60, 0 < d < 2^32,
              (2^(81-L) + 1) d + 2^49 + 2 d < 2^L.

Both are monotone in d at a fixed L, so each has one threshold d_thr(L) = the
smallest refused d.  For a ring dimension N the usable primes are = 1 mod 2N;
boundary(pred, L, m) returns the admitted prime with the largest d < d_thr and
the refused prime with the smallest d >= d_thr in that residue class, found
with the oracle's NextPrime / PreviousPrime from the threshold itself -- so
there is no prime of the class between either of them and the threshold."""
import functools

import oracle as O

NTT_RINGS = (3, 12, 13, 16, 17)  # log N: k_small, block pass only, k_cols, k_tcols, 2^17
NTT_LS = (33, 34, 35, 36, 37, 48, 60)
MMA_RINGS = (13, 16)
MMA_LS = (50, 51, 52, 56, 60)


def ntt_admits(q):
    L = q.bit_length()
    d = (1 << L) - q
    return L >= 33 and d < (1 << 32) and (q & 0xFFFFFFFF) != 0 and 16 * d < q


def ntt_terms(q):
    """which inequalities of ntt_admits hold for q (L >= 33 assumed)"""
    L = q.bit_length()
    d = (1 << L) - q
    return {"16d<q": 16 * d < q, "d<2^32": d < (1 << 32)}


def mma_admits(p):
    L = p.bit_length()
    d = (1 << L) - p
    return 33 <= L <= 60 and 0 < d < (1 << 32) and ((1 << (81 - L)) + 1) * d + (1 << 49) + 2 * d < (1 << L)


PREDICATES = {"ntt": ntt_admits, "mma": mma_admits}


def d_threshold(pred, L):
    """smallest d >= 1 with 2^L - d refused (the predicates are monotone in d: found by bisection)"""
    admits = PREDICATES[pred]
    lo, hi = 0, 1 << (L - 1)  # lo: admitted (or 0), hi: refused (d = 2^(L-1) has 2^32 <= d or 16 d >= q)
    assert not admits((1 << L) - hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if admits((1 << L) - mid):
            lo = mid
        else:
            hi = mid
    return hi


@functools.lru_cache(maxsize=None)
def boundary(pred, L, m):
    """(admitted, refused): the L-bit primes = 1 mod m nearest the threshold of
    `pred` on either side; None where the class has no such L-bit prime."""
    q_thr = (1 << L) - d_threshold(pred, L)  # the largest refused value
    base = q_thr - (q_thr - 1) % m  # largest value = 1 mod m that is <= q_thr
    adm = O.next_prime(base, m)
    ref = O.previous_prime(base + m, m)
    admits = PREDICATES[pred]
    if adm.bit_length() != L or not admits(adm):
        adm = None
    if ref.bit_length() != L or admits(ref):
        ref = None
    return adm, ref


def cases(pred):
    """[(log_n, L, admitted, refused)] over the rings and sizes of `pred`"""
    rings, ls = (NTT_RINGS, NTT_LS) if pred == "ntt" else (MMA_RINGS, MMA_LS)
    return [(lg, L) + boundary(pred, L, 2 << lg) for lg in rings for L in ls]


def root(q, log_n):
    return O.root_of_unity(2 << log_n, q)


# ---- the probe's moduli (tests/test_gpu_arith.py) ----------------------------------
def probe_moduli():
    """Moduli for the helper probe, as {name: q}: the smallest the library
    admits (22 bits), the largest NTT prime below 2^60 for N = 2^17, moduli with
    a sparse low word, and every admitted boundary prime above."""
    out = {}
    m17 = 2 << 17
    out["min22"] = O.next_prime((1 << 21) + 1, 2 << 3)  # first 22-bit prime = 1 mod 16
    out["top60_n17"] = O.previous_prime((1 << 60) + 1, m17)
    out["sparse59"] = O.next_prime((1 << 59) + 1, m17)  # 2^59 + k 2^18 + 1: low word nearly empty
    out["sparse_lo1"] = O.next_prime((1 << 40) + 1, 1 << 32)  # lo32(q) == 1
    out["generic45"] = O.next_prime((11 << 41) + 1, m17)
    for pred in ("ntt", "mma"):
        for lg, L, adm, _ in cases(pred):
            if adm is not None:
                out[f"{pred}_n{lg}_L{L}"] = adm
    return out
