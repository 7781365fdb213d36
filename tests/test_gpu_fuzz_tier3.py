"""Seeded randomized parity of the hoisted rotations and of the BFV (HPS family)
multiplication over every kernel path their engines can take, bit-exact against
tests/rotation_ref.py and tests/bfv_ref.py.

tests/test_gpu_rotation.py and tests/test_gpu_bfv.py check the two features on
60-bit chains with default plans, default converters and uniform inputs; this
file sweeps what the engines are built from.  The draws live in
tests/tier3_cases.py (plain data, no GPU) and tests/test_tier3_cases.py checks
on the CPU that the committed seed ranges reach what is listed here:

* rotations: the key-switch draw of tests/tier2_cases.py (ring 2^4 .. 2^17,
  mixed 30-60-bit moduli, dnum, level, t, batch, plan split, generic_moduli,
  separate_cols, separate_icol, chunk, single_stream) plus 1 .. 2 CAP + 1
  rotations (the second and third launch of a call), addFirst, edge-heavy
  digits, c0 and keys with one column of q - 1 in every word, and in half the
  cases digits that ModUp produced on the device;
* EvalMult / ExpandCRTBasis: ring 2^1 .. 2^17, Q 1 .. 6, R = Q or Q + 1, towers
  of 22-60 bits mixed in one chain, separate options for plan_q, plan_r and
  plan_qr, every converter kernel on every converter, both techniques;
* ScaleAndRound: 1 .. 20 summed and output towers of 22-60 bits, both
  directions, real tables;
* the exact switch: 1 .. 80 sources, 1 .. 32 targets, every kernel.

Fixed shapes that do not depend on the draw follow each sweep."""
from functools import lru_cache

import numpy as np
import pytest

import bfv_ref as B
import bfv_tables as BT
import keyswitch as K
import oracle as O
import rotation_ref as R
import tier2_cases as C2
import tier3_cases as C
from test_gpu_bfv import converter
from test_gpu_caller_stream import OnStream, delay  # noqa: F401  (delay is a fixture)
from test_gpu_fuzz import _edge_inputs
from test_gpu_fuzz_tier2 import FIXED_BITS, FIXED_DNUM, _ks_options, _msg
from test_gpu_parity import dev, host, stream
from test_gpu_rotation import Rot, _same, indices_for
from test_mixed_moduli_oracle import mixed_chain

pytestmark = pytest.mark.gpu

T_PLAIN = 65537


def zeros(*shape):
    import torch

    return torch.zeros(shape, dtype=torch.int64, device="cuda")


def _top_column(x, moduli, col):
    """q - 1 in every tower of coefficient col: the words that bound the inner product's limb sums"""
    x[..., col] = np.array(moduli, dtype=np.uint64) - np.uint64(1)
    return x


# --- hoisted rotations ----------------------------------------------------------------------------
def _rotation_inputs(rng, kp, l, n, batch, nrot, col, with_digits=True):
    """(digits or the polynomial ModUp takes, c0, keys), edge-heavy, coefficient col all q - 1"""
    q, p, dnum = kp.q, kp.p, kp.num_part_q
    ql = q[:l]
    if with_digits:
        first = np.stack([_top_column(_edge_inputs(rng, kp.beta(l), ql + p, n), ql + p, col) for _ in range(batch)])
    else:
        first = _top_column(_edge_inputs(rng, batch, ql, n), ql, col)
    c0 = _top_column(_edge_inputs(rng, batch, ql, n), ql, col)
    keys = [tuple(_top_column(_edge_inputs(rng, dnum, q + p, n), q + p, col) for _ in range(2)) for _ in range(nrot)]
    return first, c0, keys


def _device_digits(ks, kp, l, x, msg):
    """ModUp on the device, checked against the oracle's; -> (device tensor, host copy)"""
    batch, n = x.shape[0], x.shape[2]
    want = K.ks_precompute(kp, x)
    d = zeros(batch, kp.beta(l), l + len(kp.p), n)
    dx = dev(x)
    ks.precompute(l, dx.data_ptr(), d.data_ptr(), batch, stream())
    assert np.array_equal(host(d), want), "precompute: " + msg
    return d, want


@pytest.mark.parametrize("seed", range(C.SEEDS["rotation"] * C.SCALE))
def test_fuzz_rotation(hip, seed):
    H, ctx = hip
    assert H.KS_ROT_CAP == C.KS_ROT_CAP
    c = C.case("rotation", seed)
    log_n, l, batch, nrot = c["log_n"], c["level"], c["batch"], c["nrot"]
    n, sp = 1 << log_n, c["size_p"]
    kp = K.KeySwitchParams(n, c["q"], c["rq"], c["p"], c["rp"], c["dnum"])
    msg = _msg(c)
    rng = np.random.default_rng(c["rot_seed"])
    first, c0, keys = _rotation_inputs(rng, kp, l, n, batch, nrot, c["column"], not c["from_precompute"])
    ks = H.KeySwitch(ctx, log_n, c["q"], c["rq"], c["p"], c["rp"], c["dnum"], _ks_options(H, c))
    assert ks.digits(l) == (kp.alpha, c["beta"])
    idx = indices_for(n, nrot)
    if c["from_precompute"]:
        d_digits, digits = _device_digits(ks, kp, l, first, msg)
        rot = Rot(ks, l, sp, n, digits, c0, keys, idx)
        rot.d_digits = d_digits  # the device's own digits feed the rotation
    else:
        digits = first
        rot = Rot(ks, l, sp, n, digits, c0, keys, idx)
    cts = R.inner_products(kp, digits, keys)
    want_ext = R.fast_rotation_ext_ref(kp, digits, c0 if c["add_first"] else None, idx, keys, cts=cts)
    want = R.fast_rotation_ref(kp, digits, c0, idx, keys, c["t"], cts=cts)
    assert _same(rot.ext(nrot, batch, c["add_first"]), want_ext), "Ext: " + msg
    assert _same(rot.plain(nrot, batch, c["t"]), want), "non-Ext: " + msg
    assert rot.inputs_unchanged(), "inputs changed: " + msg
    ks.close()


def test_rotation_three_launches_on_caller_stream(hip, delay):  # noqa: F811
    """2 CAP + 1 rotations (three launch sets, the non-Ext call's stream-ordered scratch allocated
    and freed once per set) from a caller's stream, waited on through that stream alone."""
    H, ctx = hip
    c = C.case("rotation", 3)
    log_n, l, batch, nrot = c["log_n"], c["level"], c["batch"], c["nrot"]
    assert nrot > 2 * H.KS_ROT_CAP and not c["from_precompute"]
    n, sp = 1 << log_n, c["size_p"]
    kp = K.KeySwitchParams(n, c["q"], c["rq"], c["p"], c["rp"], c["dnum"])
    digits, c0, keys = _rotation_inputs(np.random.default_rng(c["rot_seed"]), kp, l, n, batch, nrot, c["column"])
    idx = indices_for(n, nrot)
    ks = H.KeySwitch(ctx, log_n, c["q"], c["rq"], c["p"], c["rp"], c["dnum"], _ks_options(H, c))
    st = OnStream(delay)
    dd, dc = st.input(digits), st.input(c0)
    dk = [(st.input(kb), st.input(ka)) for kb, ka in keys]
    e0, e1 = st.output(nrot, batch, l + sp, n), st.output(nrot, batch, l + sp, n)
    o0, o1 = st.output(nrot, batch, l, n), st.output(nrot, batch, l, n)
    kb, ka = [b.data_ptr() for b, _ in dk], [a.data_ptr() for _, a in dk]
    st.begin()
    ks.fast_rotation_ext(l, dd.data_ptr(), dc.data_ptr(), idx, kb, ka, e0.data_ptr(), e1.data_ptr(), batch, st.h)
    ks.fast_rotation(l, dd.data_ptr(), dc.data_ptr(), idx, kb, ka, o0.data_ptr(), o1.data_ptr(), c["t"], batch, st.h)
    st.fetch(e0, e1, o0, o1)
    got = st.wait()
    cts = R.inner_products(kp, digits, keys)
    want = R.fast_rotation_ext_ref(kp, digits, c0, idx, keys, cts=cts) + \
        R.fast_rotation_ref(kp, digits, c0, idx, keys, c["t"], cts=cts)
    assert all(np.array_equal(a, b) for a, b in zip(got, want)), _msg(c)
    import torch

    torch.cuda.synchronize()
    ks.close()


FIXED_ROT = {13: (2, 3), 17: (1, 2)}  # log_n -> (batch, nrot)
ROT_OPTIONS = ["chunk2", "single_stream", "separate_cols", "separate_icol"]
ROT_SPLITS_17 = ["SPLIT_9_8", "SPLIT_8_9", "SPLIT_COLS"]


@lru_cache(maxsize=1)
def _fixed_rotation(log_n, l):
    """one reference per (ring, level): the polynomial, its digits, c0, keys, both calls' results"""
    n = 1 << log_n
    batch, nrot = FIXED_ROT[log_n]
    m, r = mixed_chain(log_n, FIXED_BITS)
    kp = K.KeySwitchParams(n, m[:12], r[:12], m[12:], r[12:], FIXED_DNUM)
    rng = np.random.default_rng(700 + log_n + l)
    x, c0, keys = _rotation_inputs(rng, kp, l, n, batch, nrot, n // 3, with_digits=False)
    digits = K.ks_precompute(kp, x)
    idx = indices_for(n, nrot)
    cts = R.inner_products(kp, digits, keys)
    t = 0 if l == 12 else T_PLAIN
    return (kp, x, digits, c0, keys, idx, t, R.fast_rotation_ext_ref(kp, digits, c0, idx, keys, cts=cts),
            R.fast_rotation_ref(kp, digits, c0, idx, keys, t, cts=cts))


@pytest.mark.parametrize("log_n,level,option", [(log_n, level, option) for log_n in (13, 17) for level in (12, 9)
                                                for option in ROT_OPTIONS + (ROT_SPLITS_17 if log_n == 17 else [])])
def test_rotation_engine_options(hip, log_n, level, option):
    """Both hoisted-rotation calls with 12 + 4 mixed towers and dnum 3 under each engine option: at
    N = 2^17 the non-Ext call's ModDown over nrot * batch entries takes k_bconv_cols at full level
    (SPLIT_AUTO / SPLIT_COLS) unless separate_cols / separate_icol or a two-pass split forbid it.
    chunk2 takes the digits from ModUp on the device (batch 2 at 2^13: one chunk of two)."""
    H, ctx = hip
    kp, x, digits, c0, keys, idx, t, want_ext, want = _fixed_rotation(log_n, level)
    batch, nrot = FIXED_ROT[log_n]
    opt = H.KsOptions()
    if option == "chunk2":
        opt.chunk = 2
    elif option.startswith("SPLIT_"):
        opt.plan = H.PlanOptions(getattr(H, option), 0)
    else:
        setattr(opt, option, 1)
    ks = H.KeySwitch(ctx, log_n, kp.q, kp.rq, kp.p, kp.rp, FIXED_DNUM, opt)
    rot = Rot(ks, level, len(kp.p), 1 << log_n, digits, c0, keys, idx)
    msg = f"{option} log_n {log_n} level {level}"
    if option == "chunk2":
        rot.d_digits, _ = _device_digits(ks, kp, level, x, msg)
    assert _same(rot.ext(nrot, batch, True), want_ext), "Ext: " + msg
    assert _same(rot.plain(nrot, batch, t), want), "non-Ext: " + msg
    assert rot.inputs_unchanged(), "inputs changed: " + msg
    ks.close()


# --- BFV: EvalMult and ExpandCRTBasis ------------------------------------------------------------------
def _plan(H, ctx, log_n, moduli, roots, options):
    split, generic = options
    return H.NTTPlan(ctx, log_n, moduli, roots, split=getattr(H, split), generic_moduli=bool(generic))


class Mult:
    """Every handle of one BfvMult: plans with their own options, converters with their own kernels"""

    def __init__(self, H, ctx, T, log_n, rq, rr, plans, kernels):
        q, r = T.q, T.r
        self.pq = _plan(H, ctx, log_n, q, rq, plans["plan_q"])
        self.pr = _plan(H, ctx, log_n, r, rr, plans["plan_r"])
        self.pqr = _plan(H, ctx, log_n, q + r, list(rq) + list(rr), plans["plan_qr"])
        kern = lambda name: getattr(H, kernels.get(name) or "BCONV_KERNEL_AUTO")  # noqa: E731
        self.q_to_r = converter(H, ctx, log_n, q, r, kern("q_to_r"))
        self.r_to_q = converter(H, ctx, log_n, r, q, kern("r_to_q"))
        self.neg = None
        if T.technique == BT.HPSPOVERQ:
            self.neg = H.BaseConverter(ctx, log_n, q, r, T.neg_r_q_hat_inv_modq, T.flat(T.q_inv_modr),
                                       kernel=kern("q_to_r_neg"))
        self.sr = H.ScaleRound(ctx, log_n, q, r, T.out_is_q, T.sr_table, T.sr_frac)
        tech = H.BFV_HPS if T.technique == BT.HPS else H.BFV_HPSPOVERQ
        self.mult = H.BfvMult(ctx, tech, self.pq, self.pr, self.pqr, self.q_to_r, self.r_to_q, self.neg, self.sr)
        self.H, self.n, self.size_q, self.size_r = H, 1 << log_n, len(q), len(r)

    def eval_mult(self, cts, want, msg):
        batch = cts[0].shape[0]
        ins = [dev(c) for c in cts]
        outs = [zeros(batch, self.size_q, self.n) for _ in range(3)]
        self.mult.eval_mult(*[t.data_ptr() for t in ins + outs], batch, stream())
        for k, (o, w) in enumerate(zip(outs, want)):
            assert np.array_equal(host(o), w[:batch]), f"EvalMult out{k}: " + msg
        for t, c in zip(ins, cts):
            assert np.array_equal(host(t), c), "EvalMult changed its input: " + msg

    def expand(self, x, eval_form, want, msg):
        batch = x.shape[0]
        dx, out = dev(x), zeros(batch, self.size_q + self.size_r, self.n)
        self.H.expand_crt_basis(self.pq, self.pr, self.q_to_r, eval_form, dx.data_ptr(), out.data_ptr(), batch,
                                stream())
        assert np.array_equal(host(out), want[:batch]), f"ExpandCRTBasis, eval_form {eval_form}: " + msg
        assert np.array_equal(host(dx), x), "ExpandCRTBasis changed its input: " + msg

    def close(self):
        self.mult.close()
        for h in (self.sr, self.neg, self.r_to_q, self.q_to_r, self.pqr, self.pr, self.pq):
            if h is not None:
                h.close()


@pytest.mark.parametrize("seed", range(C.SEEDS["bfv_mult"] * C.SCALE))
def test_fuzz_bfv_mult(hip, seed):
    H, ctx = hip
    c = C.case("bfv_mult", seed)
    log_n, batch = c["log_n"], c["batch"]
    n, q, r = 1 << log_n, c["q"], c["r"]
    msg = _msg(c)
    T = BT.BfvTables(q, r, T_PLAIN, c["technique"])
    ring = B.Ring(O, log_n, q, c["rq"], r, c["rr"])
    rng = np.random.default_rng(c["data_seed"])
    cts = [_edge_inputs(rng, batch, q, n) for _ in range(4)]
    m = Mult(H, ctx, T, log_n, c["rq"], c["rr"], c["plans"], c["kernels"])
    m.eval_mult(cts, B.eval_mult(O, T, ring, *cts), msg)
    ev = c["eval_form"]
    m.expand(cts[0], ev, B.expand_crt_basis(O, cts[0], q, r, ring.tb_q, ring.tb_r, ev), msg)
    m.close()


def _fixed_options(log_n, split, generic):
    """plan_qr takes the named options; plan_q and plan_r, separate handles, take the next splits of
    the ring size and the other / the same generic_moduli, so the three differ wherever they can"""
    splits = C2.valid_splits(log_n)
    i = splits.index(split)
    return {"plan_qr": (split, generic), "plan_q": (splits[(i + 1) % len(splits)], 1 - generic),
            "plan_r": (splits[(i + 2) % len(splits)], generic)}


FIXED_BFV = [(log_n, split, generic) for log_n in (13, 16, 17) for split in C2.valid_splits(log_n)
             for generic in (0, 1)]
_fixed_bfv = {}


def _fixed_bfv_case(tech, log_n):
    """(T, rq, rr, ring, four inputs) of one (technique, ring): Q 2 / R 3 for HPS, 2 / 2 for
    HPSPOVERQ, 60-bit towers, batch 2 at N = 2^13 and 1 above; built once"""
    key = (tech, log_n)
    if key not in _fixed_bfv:
        sq, sr = (2, 3) if tech == BT.HPS else (2, 2)
        m, rt = O.moduli_chain(log_n, sq + sr)
        q, rq, r, rr = m[:sq], rt[:sq], m[sq:], rt[sq:]
        rng = np.random.default_rng(800 + log_n + tech)
        cts = [_edge_inputs(rng, 2 if log_n == 13 else 1, q, 1 << log_n) for _ in range(4)]
        _fixed_bfv[key] = (BT.BfvTables(q, r, T_PLAIN, tech), rq, rr, B.Ring(O, log_n, q, rq, r, rr), cts)
    return _fixed_bfv[key]


@lru_cache(maxsize=None)
def _fixed_mult_ref(tech, log_n):
    T, _, _, ring, cts = _fixed_bfv_case(tech, log_n)
    return B.eval_mult(O, T, ring, *cts, fast=log_n >= 16)  # 64-bit words where Python integers take seconds


@lru_cache(maxsize=None)
def _fixed_expand_ref(log_n, eval_form):
    T, _, _, ring, cts = _fixed_bfv_case(BT.HPS, log_n)
    return B.expand_crt_basis(O, cts[0], T.q, T.r, ring.tb_q, ring.tb_r, eval_form, fast=log_n >= 16)


@pytest.mark.parametrize("tech", [BT.HPS, BT.HPSPOVERQ])
@pytest.mark.parametrize("log_n,split,generic", FIXED_BFV)
def test_bfv_eval_mult_plan_options(hip, log_n, split, generic, tech):
    """EvalMult at N = 2^13, 2^16 and 2^17 with every plan split of the ring size (the column-pass and
    the two-pass plans under plan_ntt_range's strided in-place and out-of-place calls over 3 * batch
    entries) and with generic_moduli, one reference per (technique, ring)."""
    H, ctx = hip
    T, rq, rr, _, cts = _fixed_bfv_case(tech, log_n)
    plans = _fixed_options(log_n, split, generic)
    m = Mult(H, ctx, T, log_n, rq, rr, plans, {})
    m.eval_mult(cts, _fixed_mult_ref(tech, log_n), f"technique {tech} log_n {log_n} {plans}")
    m.close()


@pytest.mark.parametrize("eval_form", [False, True])
@pytest.mark.parametrize("log_n,split,generic", FIXED_BFV)
def test_expand_crt_basis_plan_options(hip, log_n, split, generic, eval_form):
    """ExpandCRTBasis, both input forms, over the same plans (plan_q and plan_r only)"""
    H, ctx = hip
    T, rq, rr, _, cts = _fixed_bfv_case(BT.HPS, log_n)
    plans = _fixed_options(log_n, split, generic)
    pq, pr = _plan(H, ctx, log_n, T.q, rq, plans["plan_q"]), _plan(H, ctx, log_n, T.r, rr, plans["plan_r"])
    bc = converter(H, ctx, log_n, T.q, T.r)
    x = cts[0]
    dx, out = dev(x), zeros(x.shape[0], len(T.q) + len(T.r), 1 << log_n)
    H.expand_crt_basis(pq, pr, bc, eval_form, dx.data_ptr(), out.data_ptr(), x.shape[0], stream())
    assert np.array_equal(host(out), _fixed_expand_ref(log_n, eval_form)), f"log_n {log_n} {plans}"
    assert np.array_equal(host(dx), x)
    for h in (bc, pr, pq):
        h.close()


@pytest.mark.parametrize("log_n", [5, 10])
@pytest.mark.parametrize("tech,sq,sr", [(BT.HPS, 17, 18), (BT.HPSPOVERQ, 17, 17)])
def test_bfv_eval_mult_large_q(hip, tech, sq, sr, log_n):
    """More than 16 towers inside EvalMult: the limb kernel is out (the exact and the approximate
    conversions run five K-steps on the matrix cores), ScaleAndRound sums 17 towers."""
    H, ctx = hip
    m, rt = O.moduli_chain(log_n, sq + sr)
    q, rq, r, rr = m[:sq], rt[:sq], m[sq:], rt[sq:]
    assert B.mma_ks(sq) == 5 and B.mma_ks(sr) == 5
    T = BT.BfvTables(q, r, T_PLAIN, tech)
    ring = B.Ring(O, log_n, q, rq, r, rr)
    rng = np.random.default_rng(900 + log_n + tech)
    cts = [_edge_inputs(rng, 1, q, 1 << log_n) for _ in range(4)]
    auto = ("SPLIT_AUTO", 0)
    mult = Mult(H, ctx, T, log_n, rq, rr, {"plan_q": auto, "plan_r": auto, "plan_qr": auto}, {})
    mult.eval_mult(cts, B.eval_mult(O, T, ring, *cts), f"technique {tech} log_n {log_n} Q {sq} R {sr}")
    mult.close()


# --- ScaleAndRound ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(C.SEEDS["scale_round"] * C.SCALE))
def test_fuzz_scale_round(hip, seed):
    """real tables (bfv_tables.scale_round_tables) for output moduli of 22-60 bits; coefficients 0, 1
    and 2 hold 0, 1 and modulus - 1 in every tower"""
    H, ctx = hip
    c = C.case("scale_round", seed)
    log_n, batch, q, p, out_is_q = c["log_n"], c["batch"], c["q"], c["p"], c["out_is_q"]
    n = 1 << log_n
    QR = BT.product(q) * BT.product(p)
    if out_is_q:
        table, frac = BT.scale_round_tables(p, q, T_PLAIN, BT.product(q), QR)
    else:
        table, frac = BT.scale_round_tables(q, p, T_PLAIN, BT.product(p), QR)
    rng = np.random.default_rng(c["data_seed"])
    x = _edge_inputs(rng, batch, q + p, n)
    mods = np.array(q + p, dtype=np.uint64)
    for col, val in enumerate((np.zeros_like(mods), np.ones_like(mods), mods - np.uint64(1))[:n]):
        x[:, :, col] = val
    want = B.scale_and_round(x, q, p, out_is_q, table, frac)
    sr = H.ScaleRound(ctx, log_n, q, p, out_is_q, table, frac)
    dx, out = dev(x), zeros(batch, c["size_o"], n)
    sr.run(dx.data_ptr(), out.data_ptr(), batch, stream())
    assert np.array_equal(host(out), want), _msg(c)
    assert np.array_equal(host(dx), x), "input changed: " + _msg(c)
    sr.close()


# --- the exact switch ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(C.SEEDS["switch_exact"] * C.SCALE))
def test_fuzz_switch_exact(hip, seed):
    """bfv_ref.switch_inputs (the planted near-Q/2 coefficients) and, from N = 16 on, the extreme
    columns, on mixed chains of any size with the drawn kernel"""
    H, ctx = hip
    c = C.case("switch_exact", seed)
    log_n, batch, q, p = c["log_n"], c["batch"], c["q"], c["p"]
    n = 1 << log_n
    x, kinds = B.switch_inputs(q, n, batch, c["data_seed"], planted=min(256, max(1, n // 4)))
    if n >= 16:
        x, kinds = B.plant_extremes(x, kinds, q)
    want = B.switch_crt_basis(x, q, p)
    bc = converter(H, ctx, log_n, q, p, getattr(H, c["kernel"]))
    dx, out = dev(x), zeros(batch, len(p), n)
    bc.switch_exact(dx.data_ptr(), out.data_ptr(), batch, stream())
    got = host(out)
    msg = ", ".join(f"{k} {v}" for k, v in c.items() if k not in ("q", "p", "data_seed"))
    assert np.array_equal(got, want), f"{np.count_nonzero(got != want)} words differ: " + msg
    assert np.array_equal(host(dx), x), "input changed: " + msg
    bc.close()
