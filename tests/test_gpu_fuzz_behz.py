"""Seeded randomized parity of the BFV (BEHZ) calls over every kernel path they
can take, past both of the kernels' caps and at the largest sums the kernels
can be handed, bit-exact against tests/behz_ref.py (Python integers; its 64-bit
word path from N = 2^13 up).

tests/test_gpu_behz.py checks the calls on 60-bit chains that behz_bases picks,
with default plans and uniform inputs, and the multiplication at Q = B = 2 and 4
only; this file sweeps what they are built from.  The draws and the fixed inputs
live in tests/behz_cases.py (plain data, no GPU) and tests/test_behz_cases.py
checks on the CPU that they reach what is listed here:

* the fuzz: ring 2^1 .. 2^17, Q 1 .. 6, B = Q - 1, Q or Q + 1, q, B and msk of
  22-60 bits mixed in one draw (msk smaller than a q tower, q towers below
  msk / 2), separate options for plan_q, plan_bsk and plan_qbsk, both expand
  forms, every floor_sk mode, planted Montgomery remainders and alphas, and two
  pinned chains past the caps (17 + 18 and 18 + 16 towers);
* the multiplication and expand at N = 2^13, 2^16, 2^17 under every plan split
  and generic_moduli;
* the multiplication past the caps: 17 sources (k_behz_q_to_bsk's 128-bit sums
  inside expand, read from out's Q slots at the row stride of Q + Bsk towers)
  and 17 B towers (one k_behz_floor over 3 * batch rows, then k_behz_sk from
  each third of the floors);
* synthetic tables whose sums are the largest possible: 16 sources of the limb
  kernel (its a1 + a2 carries out of 64 bits), 255 sources of the 128-bit sums,
  and the smallest moduli ofhe_hip_behz_create admits next to the largest."""
from functools import lru_cache

import numpy as np
import pytest

import behz_cases as C
import behz_ref as Z
import bfv_ref as BR
import bfv_tables as BT
import oracle as O
from test_gpu_caller_stream import OnStream, delay  # noqa: F401  (delay is a fixture)
from test_gpu_fuzz import _edge_inputs
from test_gpu_fuzz_tier2 import _msg
from test_gpu_fuzz_tier3 import FIXED_BFV, _fixed_options, _plan, zeros
from test_gpu_parity import dev, host, stream

pytestmark = pytest.mark.gpu

PLANS = ("plan_q", "plan_bsk", "plan_qbsk")


class Handles:
    """One Behz handle and its three plans, each plan with its own options"""

    def __init__(self, H, ctx, T, ring, log_n, plans):
        self.n, self.Q, self.K = 1 << log_n, len(T.q), len(T.bsk)
        self.pq = _plan(H, ctx, log_n, T.q, ring.rq, plans["plan_q"])
        self.pb = _plan(H, ctx, log_n, T.bsk, ring.rbsk, plans["plan_bsk"])
        self.pqb = _plan(H, ctx, log_n, T.q + T.bsk, ring.rq + ring.rbsk, plans["plan_qbsk"])
        self.bz = H.Behz(ctx, log_n, T)

    def eval_mult(self, cts, want, msg, batch=None):
        batch = batch or cts[0].shape[0]
        ins = [dev(c[:batch]) for c in cts]
        outs = [zeros(batch, self.Q, self.n) for _ in range(3)]
        self.bz.eval_mult(self.pq, self.pb, self.pqb, *[t.data_ptr() for t in ins + outs], batch, stream())
        got = [host(o) for o in outs]
        for k, (g, w) in enumerate(zip(got, want)):
            assert np.array_equal(g, w[:batch]), f"EvalMult out{k}: {np.count_nonzero(g != w[:batch])} words differ: " + msg
        for t, c in zip(ins, cts):
            assert np.array_equal(host(t), c[:batch]), "EvalMult changed its input: " + msg
        return got

    def expand(self, x, eval_form, want, msg):
        batch = x.shape[0]
        dx, out = dev(x), zeros(batch, self.Q + self.K, self.n)
        self.bz.expand(self.pq, self.pb, eval_form, dx.data_ptr(), out.data_ptr(), batch, stream())
        assert np.array_equal(host(out), want[:batch]), f"expand, eval_form {eval_form}: " + msg
        assert np.array_equal(host(dx), x), "expand changed its input: " + msg

    def close(self):
        for h in (self.bz, self.pqb, self.pb, self.pq):
            h.close()


def _standalone(H, bz, T, n, xq, xqb, xb, fast, msg, modes):
    """q_to_bsk, floor, conv_sk and floor_sk in `modes` (refused where BEHZ_FUSED does not fit) against behz_ref;
    every input is read back unchanged"""
    batch, Q, K = xq.shape[0], len(T.q), len(T.bsk)
    floor = Z.floor_q(xqb, T, fast=fast)
    for which, x, towers, call, want in (("q_to_bsk", xq, K, bz.q_to_bsk, Z.q_to_bsk(xq, T, fast=fast)),
                                         ("floor", xqb, K, bz.floor, floor),
                                         ("conv_sk", xb, Q, bz.conv_sk, Z.conv_sk(xb, T, fast=fast))):
        dx, out = dev(x), zeros(batch, towers, n)
        call(dx.data_ptr(), out.data_ptr(), batch, stream())
        got = host(out)
        assert np.array_equal(got, want), f"{which}: {np.count_nonzero(got != want)} words differ: " + msg
        assert np.array_equal(host(dx), x), which + " changed its input: " + msg
    want = Z.conv_sk(floor, T, fast=fast)
    dx = dev(xqb)
    for mode in modes:
        out = zeros(batch, Q, n)
        if mode == "BEHZ_FUSED" and len(T.b) > H.BEHZ_FUSED_MAX_B:
            with pytest.raises(H.MathError, match="too many B towers"):
                bz.floor_sk(dx.data_ptr(), out.data_ptr(), batch, stream(), fused=H.BEHZ_FUSED)
            assert not host(out).any(), "a refused floor_sk wrote its output: " + msg
        else:
            bz.floor_sk(dx.data_ptr(), out.data_ptr(), batch, stream(), fused=getattr(H, mode))
            assert np.array_equal(host(out), want), f"floor_sk {mode}: " + msg
    assert np.array_equal(host(dx), xqb), "floor_sk changed its input: " + msg


# --- the sweep ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(C.SEEDS * C.SCALE))
def test_fuzz_behz(hip, seed):
    H, ctx = hip
    assert H.BEHZ_FUSED_MAX_B == C.FUSED_MAX_B
    c = C.case(seed)
    log_n, batch, fast = c["log_n"], c["batch"], c["log_n"] >= C.FAST_LOG_N
    n, msg = 1 << log_n, _msg(c)
    T = C.tables(c)
    ring = Z.Ring(O, log_n, T, c["rq"])
    h = Handles(H, ctx, T, ring, log_n, c["plans"])
    _standalone(H, h.bz, T, n, *C.standalone_inputs(c), fast, msg, [c["mode"]])
    rng = np.random.default_rng(c["data_seed"])
    cts = [_edge_inputs(rng, batch, T.q, n) for _ in range(4)]
    ev = c["eval_form"]
    h.expand(cts[0], ev, Z.behz_expand(O, cts[0], T, ring, ev, fast=fast), msg)
    h.eval_mult(cts, Z.eval_mult_behz(O, T, ring, *cts, fast=fast), msg)
    h.close()


# --- every plan split and generic_moduli at the large rings ------------------------------------------------
_fixed = {}


def _fixed_case(log_n):
    """(T, ring, four inputs) of one ring: a 60-bit chain with Q = 2, B and msk from behz_bases, batch 2 at
    N = 2^13 and 1 above; built once"""
    if log_n not in _fixed:
        q, rq = O.moduli_chain(log_n, 2)
        b, msk, _ = Z.behz_bases(O, log_n, q, Z.T_PLAIN)
        T = BT.BehzTables(q, b, msk, Z.T_PLAIN)
        rng = np.random.default_rng(1800 + log_n)
        cts = [_edge_inputs(rng, 2 if log_n == 13 else 1, q, 1 << log_n) for _ in range(4)]
        _fixed[log_n] = (T, Z.Ring(O, log_n, T, rq), cts)
    return _fixed[log_n]


@lru_cache(maxsize=None)
def _fixed_mult_ref(log_n):
    T, ring, cts = _fixed_case(log_n)
    return Z.eval_mult_behz(O, T, ring, *cts, fast=log_n >= 16)  # 64-bit words where Python integers take seconds


@lru_cache(maxsize=None)
def _fixed_expand_ref(log_n, eval_form):
    T, ring, cts = _fixed_case(log_n)
    return Z.behz_expand(O, cts[0], T, ring, eval_form, fast=log_n >= 16)


def _behz_options(log_n, split, generic):
    """plan_qbsk takes the named options, plan_q and plan_bsk the next splits (test_gpu_fuzz_tier3._fixed_options)"""
    o = _fixed_options(log_n, split, generic)
    return {"plan_qbsk": o["plan_qr"], "plan_q": o["plan_q"], "plan_bsk": o["plan_r"]}


@pytest.mark.parametrize("log_n,split,generic", FIXED_BFV)
def test_bfv_eval_mult_behz_plan_options(hip, log_n, split, generic):
    """The multiplication at N = 2^13, 2^16 and 2^17 with every plan split of the ring size (the column-pass and
    the two-pass plans under plan_ntt_range's strided in-place and out-of-place calls, over 3 * batch entries for
    plan_qbsk) and with generic_moduli, one reference per ring."""
    H, ctx = hip
    T, ring, cts = _fixed_case(log_n)
    plans = _behz_options(log_n, split, generic)
    h = Handles(H, ctx, T, ring, log_n, plans)
    h.eval_mult(cts, _fixed_mult_ref(log_n), f"log_n {log_n} {plans}")
    h.close()


@pytest.mark.parametrize("eval_form", [False, True])
@pytest.mark.parametrize("log_n,split,generic", FIXED_BFV)
def test_behz_expand_plan_options(hip, log_n, split, generic, eval_form):
    """ofhe_hip_behz_expand, both input forms, over the same plans (it runs plan_q and plan_bsk, which take the next splits:
    over the grid each meets every split)"""
    H, ctx = hip
    T, ring, cts = _fixed_case(log_n)
    plans = _behz_options(log_n, split, generic)
    h = Handles(H, ctx, T, ring, log_n, plans)
    h.expand(cts[0], eval_form, _fixed_expand_ref(log_n, eval_form), f"log_n {log_n} {plans}")
    h.close()


# --- past the caps ---------------------------------------------------------------------------------------
AUTO = {name: ("SPLIT_AUTO", 0) for name in PLANS}


@pytest.mark.parametrize("batch", [1, C.PAST_BATCH])
@pytest.mark.parametrize("log_n", C.PAST_LOG_N)
@pytest.mark.parametrize("sq,sb", C.PAST_CAPS)
def test_bfv_eval_mult_behz_past_the_caps(hip, sq, sb, log_n, batch):
    """(17, 16): 128-bit sums in expand (k_behz_q_to_bsk reading out's Q slots) with the fused floor -> SK;
    (16, 17): the limb kernel with the two-launch branch (k_behz_floor over 3 * batch rows, k_behz_sk from
    F + k * batch * K * N); (17, 17): both, batch entry 0 a real encryption that decrypts to the product"""
    H, ctx = hip
    c = C.past_caps_case(sq, sb, log_n)
    T = c["T"]
    assert (len(T.q) > C.LIMB_QMAX) == (sq == 17) and (len(T.b) > H.BEHZ_FUSED_MAX_B) == (sb == 17)
    h = Handles(H, ctx, T, c["ring"], log_n, AUTO)
    got = h.eval_mult(c["cts"], c["want"], f"Q {sq} B {sb} log_n {log_n} batch {batch}", batch)
    if (sq, sb) == (17, 17):
        product = BR.negacyclic(c["ms"][0], c["ms"][1]) % Z.T_PLAIN
        assert (BR.decrypt3([g[:1] for g in got], c["s"], T.q, Z.T_PLAIN) == product).all()
    h.close()


@pytest.mark.parametrize("eval_form", [False, True])
def test_behz_expand_wide_sources(hip, eval_form):
    """expand with 17 sources at N = 2^10, batch 3: k_behz_q_to_bsk (128-bit sums) inside behz_expand_run; an
    evaluation-form input is read from out's Q slots at the row stride of Q + Bsk towers, not the dense Q"""
    H, ctx = hip
    c = C.past_caps_case(17, 16, 10)
    T, x = c["T"], c["cts"][0]
    assert len(T.q) > C.LIMB_QMAX and x.shape[0] == 3
    h = Handles(H, ctx, T, c["ring"], 10, AUTO)
    h.expand(x, eval_form, Z.behz_expand(O, x, T, c["ring"], eval_form), f"17 sources, eval_form {eval_form}")
    h.close()


def test_bfv_eval_mult_behz_two_launches_on_caller_stream(hip, delay):  # noqa: F811
    """the two-launch multiplication (17 B towers: the floors of 3 * batch rows in the stream-ordered scratch)
    ordered on the caller's stream alone"""
    H, ctx = hip
    sq, sb, log_n, batch = 16, 17, 10, C.PAST_BATCH
    c = C.past_caps_case(sq, sb, log_n)
    assert len(c["T"].b) > H.BEHZ_FUSED_MAX_B
    h = Handles(H, ctx, c["T"], c["ring"], log_n, AUTO)
    run = OnStream(delay)
    ins = [run.input(x) for x in c["cts"]]
    outs = [run.output(batch, sq, 1 << log_n) for _ in range(3)]
    run.begin()
    h.bz.eval_mult(h.pq, h.pb, h.pqb, *[t.data_ptr() for t in ins + outs], batch, run.h)
    run.fetch(*outs)
    got = run.wait()
    for g, w in zip(got, c["want"]):
        assert np.array_equal(g, w)
    import torch

    torch.cuda.synchronize()
    h.close()


# --- the largest sums ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.MAX_SUM_IDS)
def test_behz_max_sums(hip, name):
    """The standalone calls on behz_cases.SynthTables (twists 1, every multiplier its modulus minus 1) with the
    modulus minus 1 in every tower at the even coefficients: 16 sources carry out of the limb kernel's a1 + a2
    and bring a3 to 2^64 - 2^35 + 16, 255 fill the 128-bit sums; the spread cases hold the smallest moduli
    ofhe_hip_behz_create admits.  Expected values are behz_ref's exact path on the same object."""
    H, ctx = hip
    T, log_n, xq, xqb, xb = C.max_sum_case(name)
    bz = H.Behz(ctx, log_n, T)
    _standalone(H, bz, T, 1 << log_n, xq, xqb, xb, False, name, C.MODES)
    bz.close()
