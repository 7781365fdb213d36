"""Parity on both sides of the inequalities by which the host picks a kernel
instantiation from the moduli (tests/boundary_cases.py draws the primes,
tests/test_boundary_cases.py checks on the CPU that they sit at the
thresholds), bit-exact against the oracle.

NTT plans (ntt_admits: the special-prime kernels when every tower passes).
Two towers, batch 2, at N = 2^3 (k_small), 2^12 (block pass only), 2^13
(k_cols), 2^16 (k_tcols) and 2^17; per ring every L of boundary_cases.NTT_LS
appears in a tower pair.  Forms:
  spq      both towers admitted boundary primes: the special-prime kernels
           (fold_spq / canon_spq with 16 d < q at its tightest, d < 2^32 at
           its largest);
  forced   the same towers with generic_moduli: identical words;
  mixed,   one admitted and one refused tower: the whole plan takes the
  mixed-r  generic kernels (a refused prime run through the special-prime
           kernels would break the fold's range argument).
Ops: forward, inverse, ntt_mul_intt out of place and in place, forward_range /
inverse_range on strided views, and one approx_mod_down whose Q plan holds
the towers (the MODE_FWD_SUB block pass from N = 2^12 up).

Base conversion (mma_admits: bm_reduce<.., SPQ> when every target passes) at
N = 2^13 and 2^16, targets at L = 50, 51, 52, 56, 60 (no prime = 1 mod 2^17 is
admitted at L = 50, so N = 2^16 starts at 51): "adm" = every target an admitted
boundary prime (the SPQ reduction), "ref<L>" = the same with the target at L
replaced by its refused neighbour (the generic reduction for the whole
converter).  3, 7 and 33 sources: one K-step, two, and the WIDE combine.  The
handle is created with BCONV_KERNEL_AUTO, which takes the matrix-core kernel
for every N >= 32 and at most 64 sources (bconv_use_mma), so the instantiation
is the one the Python predicate names.  Callers of bm_reduce<.., SPQ>, from
reading ofhe_hip.hip, keyswitch.hip, bfv.hip, bconv_cols.hpp:
  k_bconv_mma<KS, LAZY, SPQ>   BaseConverter.switch (LAZY = 0); approx_mod_up,
                               approx_mod_down and the key switch's ModUp /
                               ModDown (LAZY = 1: a forward NTT follows)
  k_switch_mma<KS, SPQ>        BaseConverter.switch_exact, expand_crt_basis and
                               the BFV multiplication's exact switches
  k_bconv_cols<KS, SPQ, ..>    approx_mod_up / approx_mod_down at N = 2^17 under
                               SPLIT_COLS, only when the converter's and the
                               plan's admissions agree (bconv_cols_ok)
The first two are run here through switch, switch_exact, approx_mod_up in
evaluation form and expand_crt_basis; k_bconv_cols at N = 2^17 with admitted
targets in test_bconv_cols_boundary."""
from functools import lru_cache

import numpy as np
import pytest

import bfv_ref as R
import boundary_cases as BC
import keyswitch as K
import oracle as O
from test_gpu_parity import dev, host, stream

pytestmark = pytest.mark.gpu

B = 2
# tower pairs by L: every L of BC.NTT_LS is in one, 33 and 60 share a plan
NTT_PAIRS = [(33, 60), (34, 48), (35, 37), (36, 60)]
FORMS = ("spq", "forced", "mixed", "mixed-r")


def planted(rng, batch, moduli, n):
    """uniform residues with 0, 1, q - 1 planted at random places of every row"""
    x = np.stack([np.stack([rng.integers(0, q, size=n, dtype=np.uint64) for q in moduli]) for _ in range(batch)])
    for b in range(batch):
        for t, q in enumerate(moduli):
            idx = rng.choice(n, size=min(n, 6), replace=False)
            x[b, t, idx] = np.array([0, 1, q - 1, q - 1, 0, 1], np.uint64)[:len(idx)]
    return x


def extremes(moduli, n):
    """[2][T][n]: all q - 1, and alternating (q - 1, 0)"""
    top = np.array(moduli, np.uint64)[:, None] - np.uint64(1)
    full = np.broadcast_to(top, (len(moduli), n)).copy()
    alt = full.copy()
    alt[:, 1::2] = 0
    return np.stack([full, alt])


def ntt_towers(log_n, pair, form):
    m = 2 << log_n
    (a0, r0), (a1, r1) = BC.boundary("ntt", pair[0], m), BC.boundary("ntt", pair[1], m)
    q = {"spq": (a0, a1), "forced": (a0, a1), "mixed": (a0, r1), "mixed-r": (r0, a1)}[form]
    assert None not in q and q[0] != q[1]
    return q


@lru_cache(maxsize=4)
def ntt_ref(log_n, q):
    n = 1 << log_n
    r = tuple(BC.root(x, log_n) for x in q)
    tb = O.Tables(n, q, r)
    rng = np.random.default_rng(log_n * 1000 + q[0] % 997)
    ins = [planted(rng, B, q, n), extremes(q, n)]
    other = planted(rng, B, q, n)
    return {"r": r, "in": ins, "other": other, "fwd": [O.ntt_fwd(x, tb) for x in ins],
            "inv": [O.ntt_inv(x, tb) for x in ins], "mul": [O.ntt_mul_intt(x, other, tb) for x in ins]}


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("pair", NTT_PAIRS, ids=lambda p: f"L{p[0]}-L{p[1]}")
@pytest.mark.parametrize("log_n", BC.NTT_RINGS)
def test_ntt_boundary(hip, log_n, pair, form):
    import torch

    H, ctx = hip
    q = ntt_towers(log_n, pair, form)
    admitted = [BC.ntt_admits(x) for x in q]
    assert admitted == {"spq": [True, True], "forced": [True, True], "mixed": [True, False],
                        "mixed-r": [False, True]}[form]
    ref = ntt_ref(log_n, q)
    n, T = 1 << log_n, 2
    plan = H.NTTPlan(ctx, log_n, list(q), list(ref["r"]), generic_moduli=(form == "forced"))
    for k, x in enumerate(ref["in"]):
        d = dev(x)
        plan.forward(d.data_ptr(), B, stream())
        assert np.array_equal(host(d), ref["fwd"][k]), f"forward, input set {k}"
        plan.inverse(d.data_ptr(), B, stream())
        assert np.array_equal(host(d), x), f"inverse of forward, input set {k}"
        plan.inverse(d.data_ptr(), B, stream())
        assert np.array_equal(host(d), ref["inv"][k]), f"inverse, input set {k}"
        # the fused pipeline out of place, then in place over its first operand
        da, db = dev(x), dev(ref["other"])
        dc = torch.zeros_like(da)
        plan.ntt_mul_intt(da.data_ptr(), db.data_ptr(), dc.data_ptr(), B, stream())
        assert np.array_equal(host(dc), ref["mul"][k]), f"ntt_mul_intt, input set {k}"
        assert np.array_equal(host(da), x) and np.array_equal(host(db), ref["other"])
        plan.ntt_mul_intt(da.data_ptr(), db.data_ptr(), da.data_ptr(), B, stream())
        assert np.array_equal(host(da), ref["mul"][k]), f"ntt_mul_intt in place, input set {k}"
        # tower 1 alone, from a 2-tower source into a 3-tower-wide buffer at tower 2, and back
        src = dev(x)
        wide = torch.zeros((B, 3, n), dtype=torch.int64, device="cuda")
        plan.forward_range(1, 1, src[:, 1].data_ptr(), wide[:, 2].data_ptr(), T * n, 3 * n, B, stream())
        got = host(wide)
        assert np.array_equal(got[:, 2], ref["fwd"][k][:, 1]) and not got[:, :2].any(), f"forward_range, set {k}"
        back = torch.zeros((B, 1, n), dtype=torch.int64, device="cuda")
        plan.inverse_range(1, 1, wide[:, 2].data_ptr(), back.data_ptr(), 3 * n, n, B, stream())
        assert np.array_equal(host(back)[:, 0], x[:, 1]), f"inverse_range, set {k}"
        # both towers in place
        plan.forward_range(0, 2, src.data_ptr(), src.data_ptr(), T * n, T * n, B, stream())
        assert np.array_equal(host(src), ref["fwd"][k]), f"forward_range in place, set {k}"
    plan.close()


@lru_cache(maxsize=4)
def moddown_ref(log_n, q):
    n = 1 << log_n
    rq = tuple(BC.root(x, log_n) for x in q)
    p, rp = O.moduli_chain(log_n, 2, bits=59)
    assert not set(p) & set(q)
    rng = np.random.default_rng(7 * log_n + q[1] % 991)
    x = planted(rng, B, list(q) + p, n)
    x[1, :2] = extremes(q, n)[0]  # the Q part of entry 1: all q - 1
    return {"rq": rq, "p": p, "rp": rp, "x": x, "want": K.approx_mod_down(x, list(q), list(rq), p, rp)}


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("pair", [NTT_PAIRS[0], NTT_PAIRS[2]], ids=lambda p: f"L{p[0]}-L{p[1]}")
@pytest.mark.parametrize("log_n", BC.NTT_RINGS)
def test_approx_mod_down_boundary_q(hip, log_n, pair, form):
    """ApproxModDown into a Q plan of boundary towers: from N = 2^12 up the Q
    towers' forward transform ends in the MODE_FWD_SUB block pass."""
    import torch

    H, ctx = hip
    q = ntt_towers(log_n, pair, form)
    ref = moddown_ref(log_n, q)
    p, rp = ref["p"], ref["rp"]
    pq = H.NTTPlan(ctx, log_n, list(q), list(ref["rq"]), generic_moduli=(form == "forced"))
    pp = H.NTTPlan(ctx, log_n, p, rp)
    T = K.moddown_tables(list(q), p)
    bc = H.BaseConverter(ctx, log_n, p, list(q), T["phinv"], [v for row in T["phmodq"] for v in row])
    dx = dev(ref["x"])
    out = torch.zeros((B, 2, 1 << log_n), dtype=torch.int64, device="cuda")
    H.approx_mod_down(pq, pp, bc, T["pinv_modq"], 0, dx.data_ptr(), out.data_ptr(), B, stream())
    assert np.array_equal(host(out), ref["want"])
    assert np.array_equal(host(dx), ref["x"])
    for o in (bc, pp, pq):
        o.close()


# ---- base conversion --------------------------------------------------------------------
BCONV_B = 3
SOURCES = (3, 7, 33)  # K-steps 1, 2, and 9 -> 10 (more than 32 sources: the WIDE combine)


def mma_ls(log_n):
    return [L for L in BC.MMA_LS if BC.boundary("mma", L, 2 << log_n)[0] is not None]


def mma_targets(log_n, which):
    """"adm": the admitted boundary prime of every L; "ref<L>": the refused neighbour at L instead"""
    m = 2 << log_n
    p = [BC.boundary("mma", L, m)[0] for L in mma_ls(log_n)]
    if which != "adm":
        L = int(which[3:])
        p[mma_ls(log_n).index(L)] = BC.boundary("mma", L, m)[1]
    assert None not in p and len(set(p)) == len(p)
    return p


def bconv_whiches(log_n):
    return ["adm"] + [f"ref{L}" for L in mma_ls(log_n)]


@lru_cache(maxsize=2)
def bconv_sources(log_n, sq):
    q, rq = O.moduli_chain(log_n, sq, bits=58)
    n = 1 << log_n
    rng = np.random.default_rng(100 * log_n + sq)
    x = np.concatenate([planted(rng, 1, q, n), extremes(q, n)])
    return q, rq, x


@lru_cache(maxsize=2)
def bconv_ref(log_n, sq, which):
    q, rq, x = bconv_sources(log_n, sq)
    p = mma_targets(log_n, which)
    rp = [BC.root(v, log_n) for v in p]
    qhinv, qhmodp = K.switch_tables(q, p)
    xe = K.set_format(x, q, rq, True)
    tb_q, tb_p = O.Tables(1 << log_n, q, rq), O.Tables(1 << log_n, p, rp)
    return {"q": q, "rq": rq, "p": p, "rp": rp, "x": x, "xe": xe, "tabs": (qhinv, [v for row in qhmodp for v in row]),
            "switch": K._switch_basis(x, q, p, qhinv, qhmodp), "exact": R.switch_crt_basis(x, q, p, fast=True),
            "modup": K.approx_mod_up(xe, q, rq, p, rp, True),
            "expand": R.expand_crt_basis(O, xe, q, p, tb_q, tb_p, True, fast=True)}


BCONV_CASES = [pytest.param(log_n, sq, which, id=f"{log_n}-{sq}-{which}") for log_n in BC.MMA_RINGS for sq in SOURCES
               for which in bconv_whiches(log_n)]


@pytest.mark.parametrize("log_n,sq,which", BCONV_CASES)
def test_bconv_boundary(hip, log_n, sq, which):
    import torch

    H, ctx = hip
    ref = bconv_ref(log_n, sq, which)
    q, p = ref["q"], ref["p"]
    spq = R.mma_spq(p)
    assert spq == all(BC.mma_admits(v) for v in p) == (which == "adm")  # bm_reduce<.., SPQ> or the generic reduction
    assert [BC.mma_admits(v) for v in p].count(False) == (0 if spq else 1)
    assert R.mma_ks(sq) == {3: 1, 7: 2, 33: 10}[sq]
    n, sp = 1 << log_n, len(p)
    bc = H.BaseConverter(ctx, log_n, q, p, *ref["tabs"], kernel=H.BCONV_KERNEL_AUTO)
    dx = dev(ref["x"])
    out = torch.zeros((BCONV_B, sp, n), dtype=torch.int64, device="cuda")
    bc.switch(dx.data_ptr(), out.data_ptr(), BCONV_B, stream())  # k_bconv_mma<KS, 0, SPQ>
    got = host(out)
    assert np.array_equal(got, ref["switch"]), f"switch: {np.count_nonzero(got != ref['switch'])} words differ"
    out.zero_()
    bc.switch_exact(dx.data_ptr(), out.data_ptr(), BCONV_B, stream())  # k_switch_mma<KS, SPQ>
    got = host(out)
    assert np.array_equal(got, ref["exact"]), f"switch_exact: {np.count_nonzero(got != ref['exact'])} words differ"
    assert np.array_equal(host(dx), ref["x"])
    # evaluation-form callers: k_bconv_mma<KS, 1, SPQ> feeding the P plan's forward transform
    pq, pp = H.NTTPlan(ctx, log_n, q, ref["rq"]), H.NTTPlan(ctx, log_n, p, ref["rp"])
    dxe = dev(ref["xe"])
    up = torch.zeros((BCONV_B, sq + sp, n), dtype=torch.int64, device="cuda")
    H.approx_mod_up(pq, pp, bc, True, dxe.data_ptr(), up.data_ptr(), BCONV_B, stream())
    got = host(up)
    assert np.array_equal(got, ref["modup"]), f"approx_mod_up: {np.count_nonzero(got != ref['modup'])} words differ"
    up.zero_()
    H.expand_crt_basis(pq, pp, bc, True, dxe.data_ptr(), up.data_ptr(), BCONV_B, stream())
    got = host(up)
    assert np.array_equal(got, ref["expand"]), f"expand_crt_basis: {np.count_nonzero(got != ref['expand'])} differ"
    for o in (bc, pp, pq):
        o.close()


def test_bconv_cols_boundary(hip):
    """k_bconv_cols<KS, SPQ> (N = 2^17, SPLIT_COLS): approx_mod_up whose P plan
    holds the admitted matrix-core boundary primes = 1 mod 2^18 -- admitted by
    ntt_admits too, so the converter's and the plan's admissions agree and the
    fused column kernel runs with SPQ on both its reduction and its
    butterflies; then one refused target, where they disagree (the plan is
    still special-prime, the converter generic) and the unfused path runs."""
    import torch

    H, ctx = hip
    log_n, sq = 17, 3
    n = 1 << log_n
    adm = [BC.boundary("mma", L, 2 << log_n) for L in BC.MMA_LS]
    p_adm = [a for a, _ in adm if a is not None]
    assert len(p_adm) >= 3 and all(BC.mma_admits(v) and BC.ntt_admits(v) for v in p_adm)
    ref_p = next(r for a, r in adm if a is not None and BC.ntt_admits(r))  # refused by mma_admits alone
    q, rq = O.moduli_chain(log_n, sq, bits=58)
    rng = np.random.default_rng(1717)
    x = np.concatenate([planted(rng, 1, q, n), extremes(q, n)[:1]])
    xe = K.set_format(x, q, rq, True)
    pq = H.NTTPlan(ctx, log_n, q, rq, split=H.SPLIT_COLS)
    for p in (p_adm, p_adm[:-1] + [ref_p]):
        assert len(set(p)) == len(p)
        rp = [BC.root(v, log_n) for v in p]
        assert all(BC.ntt_admits(v) for v in p) and R.mma_spq(p) == (p is p_adm)
        qhinv, qhmodp = K.switch_tables(q, p)
        bc = H.BaseConverter(ctx, log_n, q, p, qhinv, [v for row in qhmodp for v in row])
        pp = H.NTTPlan(ctx, log_n, p, rp, split=H.SPLIT_COLS)
        dxe = dev(xe)
        up = torch.zeros((2, sq + len(p), n), dtype=torch.int64, device="cuda")
        H.approx_mod_up(pq, pp, bc, True, dxe.data_ptr(), up.data_ptr(), 2, stream())
        assert np.array_equal(host(up), K.approx_mod_up(xe, q, rq, p, rp, True))
        bc.close()
        pp.close()
    pq.close()
