"""GPU parity for the rescaling callers, BV key switching and EvalMultCore on
modulus chains of mixed size, through every launch path the ring size and the
plan options select, bit-exact against oracle/keyswitch.py (pinned on such
chains by tests/test_mixed_moduli_oracle.py).

The other tests of these ops draw their moduli from O.moduli_chain: strictly
decreasing primes just below 2^60, so that SwitchModulus inside the fused
kernels (switch_mod1, csrc/arith.hpp) only ever lifts into a slightly larger
modulus.  Here one chain makes the dropped tower face a 60-bit tower (up,
large difference), a prime just above it (up, small difference), a prime just
below it (down, two conditional subtractions) and a tower of at most 30 bits
(down by more than a factor of two: the general remainder), with boundary
words 0, 1, q/2, q/2 + 1, q - 1 in half of its coefficients.

Launch paths (PATHS): k_small + k_sub_scale (N < 2^12), the block
forward-subtract pass (2^12), the switch-loading column pass k_cols<K>
(launch_cols_sw<1>, <3>, <4> under SPLIT_COLS at 2^16, <5>), k_tcols'
switch-load at 2^16 and, under SPLIT_8_9, at 2^17, and the unfused kernels of
SPLIT_9_8.  Modulus forms (FORMS): a plan only takes the special-prime
kernels (q = 2^L - d) when every tower has at least 33 bits, so the chain
with a 30-bit tower runs the generic instantiations by itself; the same chain
with a 34-bit small tower (still less than half of the 50-bit dropped tower)
runs the special-prime ones, and with generic_moduli = 1 the generic ones on
identical inputs; the last form is a chain of primes far from any 2^L.  Every
test asserts that its chain is what its form's name says to the plan
(_check_form).  The BV chain is a 60-bit tower, two neighbouring primes below
2^59, the small tower and a 45-bit fifth tower for the keys: its digit ->
tower pairs take all three branches, and in the special34 form every tower
is of the special form."""
from functools import lru_cache

import numpy as np
import pytest

import keyswitch as K
import oracle as O
from test_gpu_evalmult import _ref as evalmult_ref
from test_gpu_parity import dev, host, stream
from test_mixed_moduli_oracle import (bv_chain, is_special_prime, regime, rescale_chain, rescale_input, uniform,
                                      with_boundaries)

pytestmark = pytest.mark.gpu

B = 2
T_MR = (2, 65537)  # ModReduce plaintext moduli: 2 and a 17-bit one

# (log_n, split name): the smallest ring size reaching each launch path
PATHS = [(5, "SPLIT_AUTO"), (12, "SPLIT_AUTO"), (13, "SPLIT_AUTO"), (15, "SPLIT_AUTO"), (16, "SPLIT_AUTO"),
         (16, "SPLIT_COLS"), (17, "SPLIT_AUTO"), (17, "SPLIT_8_9"), (17, "SPLIT_9_8")]
# name -> (truly generic chain, bits of the small tower, plan option generic_moduli)
FORMS = {"special30": (False, 30, False), "special30-forced": (False, 30, True), "special34": (False, 34, False),
         "special34-forced": (False, 34, True), "generic": (True, 30, False)}
# chain-major order, so that each reference is computed once and reused by the cases next to it
CASES = [pytest.param(log_n, split, form, ev, id=f"{log_n}-{split}-{form}-{'eval' if ev else 'coef'}")
         for log_n in sorted({p[0] for p in PATHS}) for chain in ((False, 30), (False, 34), (True, 30))
         for ev in (True, False) for form, f in FORMS.items() if f[:2] == chain
         for (ln, split) in PATHS if ln == log_n]
LOWER_AT = (13, 17)  # ring sizes that also run one level lower (the first 4 of the plan's 5 towers)


def _check_form(form, moduli):
    """The chain is what its name says to the plan: every tower of a special34
    chain passes the plan's special-prime test (so the default plan runs the
    special-prime kernels and generic_moduli = 1 is what turns them off), the
    special30 chain fails it in its 30-bit tower alone, a generic chain in all."""
    special = [is_special_prime(q) for q in moduli]
    if form.startswith("special34"):
        assert all(special), moduli
    elif form.startswith("special30"):
        assert special.count(False) == 1 and min(moduli).bit_length() <= 30, moduli
    else:
        assert not any(special), moduli


def _negtinv(t, ql):
    return (-pow(t, -1, ql)) % ql


@lru_cache(maxsize=2)
def _rescale_ref(log_n, generic, small_bits, ev):
    """Inputs and the oracle's outputs of one (ring, chain, form of the input)."""
    n = 1 << log_n
    q, r = rescale_chain(log_n, generic, small_bits)
    rng = np.random.default_rng(1000 * log_n + small_bits + generic)
    x = rescale_input(rng, B, q, n)
    x[:, 3] = with_boundaries(rng, B, q[3], n)  # the tower dropped one level lower
    if ev:
        x = K.set_format(x, q, r, True)
    ref = {"q": q, "r": r, "x": x, "levels": {}}
    for T in (5, 4) if log_n in LOWER_AT else (5,):
        qt, rt = q[:T], r[:T]
        xt = np.ascontiguousarray(x[:, :T])
        c, a = K.rescale_tables(qt)
        lv = {"c": c, "a": a, "drop": K.drop_last_and_scale(xt, qt, rt, ev, c, a), "mr": {}}
        for t in T_MR if T == 5 else T_MR[:1]:
            lv["mr"][t] = K.mod_reduce(xt, qt, rt, ev, t, _negtinv(t, qt[-1]), a)
        ref["levels"][T] = lv
    return ref


@pytest.mark.parametrize("log_n,split,form,ev", CASES)
def test_rescale_mixed_chain(hip, log_n, split, form, ev):
    import torch

    H, ctx = hip
    generic, small_bits, forced = FORMS[form]
    ref = _rescale_ref(log_n, generic, small_bits, ev)
    q, r, x = ref["q"], ref["r"], ref["x"]
    assert [regime(q[-1], qi) for qi in q[:-1]] == ["up", "up", "down_big", "down_small"]
    _check_form(form, q)
    n, TP = 1 << log_n, len(q)
    plan = H.NTTPlan(ctx, log_n, q, r, split=getattr(H, split), generic_moduli=forced)
    dx = dev(x)
    for T, lv in ref["levels"].items():
        c, a = lv["c"], lv["a"]
        # out of place, packed output
        out = torch.zeros((B, T - 1, n), dtype=torch.int64, device="cuda")
        plan.drop_last_and_scale(T, dx.data_ptr(), TP * n, out.data_ptr(), (T - 1) * n, ev, c, a, B, stream())
        assert np.array_equal(host(out), lv["drop"]), f"drop_last_and_scale level {T}"
        for t, want in lv["mr"].items():
            # padded output stride: one spare tower per batch entry stays untouched
            out = torch.zeros((B, T, n), dtype=torch.int64, device="cuda")
            plan.mod_reduce(T, dx.data_ptr(), TP * n, out.data_ptr(), T * n, ev, t, _negtinv(t, q[T - 1]), a, B,
                            stream())
            got = host(out)
            assert np.array_equal(got[:, :T - 1], want), f"mod_reduce t {t} level {T}"
            assert not got[:, T - 1].any()
    assert np.array_equal(host(dx), x)  # the out-of-place calls left their input alone
    # in place with equal strides (last: it overwrites the input)
    lv = ref["levels"][TP]
    plan.drop_last_and_scale(TP, dx.data_ptr(), TP * n, dx.data_ptr(), TP * n, ev, lv["c"], lv["a"], B, stream())
    assert np.array_equal(host(dx)[:, :TP - 1], lv["drop"]), "drop_last_and_scale in place"
    dx = dev(x)
    t = T_MR[1]
    plan.mod_reduce(TP, dx.data_ptr(), TP * n, dx.data_ptr(), TP * n, ev, t, _negtinv(t, q[-1]), lv["a"], B, stream())
    assert np.array_equal(host(dx)[:, :TP - 1], lv["mr"][t]), "mod_reduce in place"
    plan.close()


# --- BV key switching ---------------------------------------------------------
T_BV = 4


@lru_cache(maxsize=2)
def _bv_ref(log_n, generic, small_bits):
    n = 1 << log_n
    qa, ra = bv_chain(log_n, generic, small_bits, extra=(45,))  # the keys' fifth tower
    q, rq = qa[:T_BV], ra[:T_BV]
    rng = np.random.default_rng(2000 * log_n + small_bits + generic)
    coef = np.stack([with_boundaries(rng, B, qi, n) for qi in q], axis=1)
    c = K.set_format(coef, q, rq, True)
    kb, ka = uniform(rng, T_BV, qa, n), uniform(rng, T_BV, qa, n)
    d = K.crt_decompose0(c, q, rq)
    o0, o1 = K.bv_fast_core(d, kb, ka, q)
    return {"qa": qa, "ra": ra, "c": c, "kb": kb, "ka": ka, "d": d, "o0": o0, "o1": o1}


BV_CASES = [pytest.param(log_n, split, form, id=f"{log_n}-{split}-{form}")
            for log_n in sorted({p[0] for p in PATHS}) for chain in ((False, 30), (False, 34), (True, 30))
            for form, f in FORMS.items() if f[:2] == chain for (ln, split) in PATHS if ln == log_n]


@pytest.mark.parametrize("log_n,split,form", BV_CASES)
def test_bv_mixed_chain(hip, log_n, split, form):
    import torch

    H, ctx = hip
    generic, small_bits, forced = FORMS[form]
    ref = _bv_ref(log_n, generic, small_bits)
    qa, ra, T = ref["qa"], ref["ra"], T_BV
    assert {regime(qa[i], qa[k]) for i in range(T) for k in range(T) if i != k} == {"up", "down_small", "down_big"}
    _check_form(form, qa)
    n = 1 << log_n
    plan = H.NTTPlan(ctx, log_n, qa, ra, split=getattr(H, split), generic_moduli=forced)
    dc = dev(ref["c"])
    dd = torch.zeros((B, T, T, n), dtype=torch.int64, device="cuda")
    plan.bv_precompute(T, dc.data_ptr(), dd.data_ptr(), B, stream())
    assert np.array_equal(host(dd), ref["d"])
    assert np.array_equal(host(dc), ref["c"])
    o0 = torch.zeros((B, T, n), dtype=torch.int64, device="cuda")
    o1 = torch.zeros_like(o0)
    # keys with one tower more than the level (DropLastElements), then keys of exactly T towers
    for kb, ka in ((ref["kb"], ref["ka"]), (ref["kb"][:, :T], ref["ka"][:, :T])):
        dkb, dka = dev(kb), dev(ka)
        plan.bv_core(T, dd.data_ptr(), dkb.data_ptr(), dka.data_ptr(), kb.shape[1], o0.data_ptr(), o1.data_ptr(), B,
                     stream())
        assert np.array_equal(host(o0), ref["o0"]) and np.array_equal(host(o1), ref["o1"]), kb.shape
        o0.zero_()
        o1.zero_()
    plan.close()


@pytest.mark.parametrize("generic", [False, True])
def test_bv_semantic_mixed_chain(hip, generic):
    """Real BV keys (KeySwitchGenInternal, digitSize = 0) on the mixed chain at
    N = 2^12 (special-prime kernels: the chain with the 34-bit tower; generic
    ones: the generic chain): ct0 + ct1 s_new = c s_old - sum_i d_i e_i on the
    device outputs."""
    import torch

    H, ctx = hip
    log_n, T = 12, T_BV
    n = 1 << log_n
    q, rq = bv_chain(log_n, generic, 30 if generic else 34)
    _check_form("generic" if generic else "special34", q)
    rng = np.random.default_rng(17 + generic)
    c = uniform(rng, 1, q, n)
    s_old = K.small_poly_eval(rng.integers(-1, 2, size=n), q, rq)[0]
    s_new = K.small_poly_eval(rng.integers(-1, 2, size=n), q, rq)[0]
    kb, ka, es = K.bv_keygen(q, rq, s_old, s_new, rng)
    plan = H.NTTPlan(ctx, log_n, q, rq)
    dc = dev(c)
    dd = torch.empty((1, T, T, n), dtype=torch.int64, device="cuda")
    plan.bv_precompute(T, dc.data_ptr(), dd.data_ptr(), 1, stream())
    o0 = torch.empty((1, T, n), dtype=torch.int64, device="cuda")
    o1 = torch.empty_like(o0)
    dkb, dka = dev(kb), dev(ka)
    plan.bv_core(T, dd.data_ptr(), dkb.data_ptr(), dka.data_ptr(), T, o0.data_ptr(), o1.data_ptr(), 1, stream())
    d = host(dd)
    lhs = O.eltwise("add", host(o0), O.eltwise("mul", host(o1), s_new[None], q), q)
    noise = O.eltwise("mul", d[:, 0], es[0:1], q)
    for i in range(1, T):
        noise = O.eltwise("add", noise, O.eltwise("mul", d[:, i], es[i:i + 1], q), q)
    assert np.array_equal(lhs, O.eltwise("sub", O.eltwise("mul", c, s_old[None], q), noise, q))
    plan.close()


# --- EvalMultCore ---------------------------------------------------------------
@pytest.mark.parametrize("log_n", [4, 12, 16])
@pytest.mark.parametrize("forced", [False, True])
@pytest.mark.parametrize("edge", [False, True])
def test_eval_mult_core_mixed_chain(hip, log_n, forced, edge):
    """The 60 / 50 / 34 / 50 / 50-bit chain (every tower of the special form, so
    the default plan takes the special-prime kernel and generic_moduli = 1 the
    generic one): random and all-(q - 1) operands against the reference's own
    sequence of ModMul / ModAdd."""
    import torch

    H, ctx = hip
    n = 1 << log_n
    q, rq = rescale_chain(log_n, False, 34)
    _check_form("special34", q)
    T = len(q)
    rng = np.random.default_rng(123 + log_n)
    if edge:
        xs = [np.broadcast_to(np.array(q, np.uint64)[None, :, None] - np.uint64(1), (B, T, n)).copy()
              for _ in range(4)]
    else:
        xs = [uniform(rng, B, q, n) for _ in range(4)]
    plan = H.NTTPlan(ctx, log_n, q, rq, generic_moduli=forced)
    dx = [dev(x) for x in xs]
    outs = [torch.zeros_like(dx[0]) for _ in range(3)]
    plan.eval_mult_core(*(t.data_ptr() for t in dx), *(o.data_ptr() for o in outs), B, stream())
    for o, w in zip(outs, evalmult_ref(*xs, q)):
        assert np.array_equal(host(o), w)
    plan.close()
