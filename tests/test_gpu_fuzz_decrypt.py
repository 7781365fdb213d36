"""Seeded randomized parity of BFV decryption and TimesQovert over every kernel
path, parameter edge and plan option they can take, bit-exact against
tests/decrypt_ref.py (numpy float64 and uint64, Python integers behind it).

tests/test_gpu_bfv_decrypt.py checks the calls on towers of one size with small
plaintext moduli, three towers and default plans; this file sweeps what they are
built from.  The draws and the fixed inputs live in tests/decrypt_cases.py
(plain data, no GPU) and tests/test_decrypt_cases.py checks on the CPU that they
reach what is listed here:

* the fuzz: ring 2^1 .. 2^17, 1 .. 6 towers of 22-60 bits mixed in one chain, t
  from 2 to a prime near 2^55, HPS / HPSPOVERQ / BEHZ, 2 or 3 elements in either
  form, every option of plan_q; batch entry 0 a synthesised encryption; pinned
  chains with towers far wider and far narrower than q[0] (the loop and the split
  point come from q[0] alone), the two sides of qMSB + sizeQMSB = 52, one tower
  at 2^13 and 2^16, 17 towers;
* the decrypt call at N = 2^13, 2^16, 2^17 under every plan split and
  generic_moduli, with 9 and 17 towers, with one tower, and on rings of 2, 4 and
  64 coefficients on the caller's stream;
* scale-round at the largest t and tower counts ofhe_hip_bfv_decrypt_create
  admits (intSum up to 64 bits), on inputs whose output equals t, and on the
  one-tower path at q <= 2 t and t > q;
* TimesQovert on any 64-bit word, at t = 2, t > q_i and t up to 2^62.

The reference does not decrypt every chain it is handed: it sizes every tower by
q[0] and keeps intSum in a double (decrypt_cases.reference_decrypts).  Its output
is defined all the same, and the library must reproduce it bit for bit; batch
entry 0 is compared with the plaintext where the reference decrypts.  No input
with an undefined final cast (decrypt_ref.defined) was met in the sweep or in
the fixed inputs: the excluded share is 0.

Not covered: the stride loop of the element-wise grid (grid_for's cap of 2^22
workgroups) needs 2^30 items in one launch, which is not a few-second test."""
from functools import lru_cache

import numpy as np
import pytest

import bfv_tables as BT
import decrypt_cases as C
import decrypt_ref as D
import oracle as O
from test_gpu_caller_stream import OnStream, delay  # noqa: F401  (delay is a fixture)
from test_gpu_fuzz import _edge_inputs
from test_gpu_fuzz_tier2 import _msg
from test_gpu_fuzz_tier3 import FIXED_BFV, _plan
from test_gpu_parity import dev, host, stream

pytestmark = pytest.mark.gpu

U64 = np.uint64
PATTERN = 0x5A5A5A5A5A5A5A5A  # no expected output word: above 2^62, past every t and q_i of this file
T_PLAIN = 65537


def pattern(*shape):
    """an output buffer that starts as a non-zero pattern, so an unwritten word shows"""
    import torch

    return torch.full(shape, PATTERN, dtype=torch.int64, device="cuda")


def branch_name(H, branch):
    return {H.BFV_DECRYPT_BEHZ: "BEHZ", H.BFV_DECRYPT_ONE_TOWER: "ONE_TOWER"}.get(branch) or BT.BRANCHES[branch]


def same(got, want, msg):
    bad = np.flatnonzero(got.reshape(-1) != want.reshape(-1))
    assert got.shape == want.shape and bad.size == 0, \
        (msg, bad.size, bad[:8], got.reshape(-1)[bad[:8]], want.reshape(-1)[bad[:8]])


def run_scale_round(H, ctx, k, technique, want, msg):
    T, n, batch = k["T"], k["n"], k["batch"]
    dec = H.BfvDecrypt(ctx, k["log_n"], T, technique)
    dx, out = dev(k["x"]), pattern(batch, n)
    dec.scale_round(dx.data_ptr(), out.data_ptr(), batch, stream())
    got, branch = host(out), dec.branch
    same(got, want, msg)
    same(host(dx), k["x"], msg + ": the input changed")
    dec.close()
    return got, branch_name(H, branch)


def run_decrypt(H, dec, plan, elems, s_eval, eval_form, want, msg):
    """the decrypt call on device copies of elems against want; every input is read back unchanged"""
    batch, n = want.shape
    ins, ds, out = [dev(e) for e in elems], dev(s_eval), pattern(batch, n)
    dec.decrypt(plan, [t.data_ptr() for t in ins], ds.data_ptr(), out.data_ptr(), eval_form, batch, stream())
    got = host(out)
    same(got, want, msg)
    for t, e in zip(ins + [ds], list(elems) + [s_eval]):
        same(host(t), e, msg + ": an input changed")
    return got


# --- the sweep ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(C.SEEDS * C.SCALE))
def test_fuzz_decrypt(hip, seed):
    H, ctx = hip
    c = C.case(seed)
    k = C.sweep_inputs(c)
    T, log_n, batch, is_behz, msg = k["T"], c["log_n"], c["batch"], C.behz(c), _msg(c)
    n = 1 << log_n
    plan = _plan(H, ctx, log_n, T.q, c["rq"], c["plan_q"])
    dec = H.BfvDecrypt(ctx, log_n, T, getattr(H, c["technique"]))
    assert branch_name(H, dec.branch) == C.branch_name(T, is_behz), msg
    # ScaleAndRound on the INTT of the reference's DecryptCore output
    dx, out = dev(k["x"]), pattern(batch, n)
    dec.scale_round(dx.data_ptr(), out.data_ptr(), batch, stream())
    same(host(out), D.scale_round_any(k["x"], T, is_behz), "scale_round: " + msg)
    same(host(dx), k["x"], "scale_round changed its input: " + msg)
    # the whole call in the drawn form and element count
    elems = k["elems"] if c["eval_form"] else [O.ntt_inv(e, k["tb"]) for e in k["elems"]]
    got = run_decrypt(H, dec, plan, elems, k["s_eval"], c["eval_form"], C.want_decrypt(c, k), "decrypt: " + msg)
    if C.reference_decrypts(T, is_behz):
        assert (got[0] % U64(T.t) == k["plain"].astype(U64)).all(), "entry 0 does not decrypt: " + msg
    # TimesQovert out of place, then in place
    want = D.times_q_over_t(k["tq"], T)
    dx, out = dev(k["tq"]), pattern(batch, len(T.q), n)
    dec.times_q_over_t(dx.data_ptr(), out.data_ptr(), batch, stream())
    same(host(out), want, "times_q_over_t: " + msg)
    same(host(dx), k["tq"], "times_q_over_t changed its input: " + msg)
    dec.times_q_over_t(dx.data_ptr(), dx.data_ptr(), batch, stream())
    same(host(dx), want, "times_q_over_t in place: " + msg)
    dec.close()
    plan.close()


# --- the decrypt call on fixed shapes -----------------------------------------------------------------
@lru_cache(maxsize=None)
def _call_case(log_n, towers, batch, t=T_PLAIN, q=None):
    """(T, roots, tb, s_eval [Q][n], three elements [batch][Q][n] in evaluation form) of one shape, edge-heavy
    uniform: a 60-bit chain unless q names the towers' sizes; built once"""
    m, r = O.moduli_chain(log_n, towers) if q is None else C.mixed_chain(log_n, list(q))
    n = 1 << log_n
    rng = np.random.default_rng([1900, log_n, towers, t % 1009])
    elems = [_edge_inputs(rng, batch, m, n) for _ in range(3)]
    s_eval = _edge_inputs(rng, 1, m, n)[0]
    return BT.DecryptTables(m, t), r, O.Tables(n, m, r), s_eval, elems


@lru_cache(maxsize=None)
def _call_ref(key, elements, eval_form, is_behz):
    """(the elements in the form asked for, the reference's output); one reference per shape and form"""
    T, _, tb, s_eval, elems = _call_case(*key)
    elems = elems[:elements] if eval_form else [O.ntt_inv(e, tb) for e in elems[:elements]]
    return elems, D.decrypt(O, elems, s_eval, T, tb, eval_form, is_behz)


def _run_call(H, ctx, key, elements, eval_form, is_behz, options=("SPLIT_AUTO", 0), want_branch=None):
    T, r, _, s_eval, _ = _call_case(*key)
    elems, want = _call_ref(key, elements, eval_form, is_behz)
    msg = f"{key} elements {elements} eval_form {eval_form} behz {is_behz} {options}"
    plan = _plan(H, ctx, key[0], T.q, r, options)
    dec = H.BfvDecrypt(ctx, key[0], T, H.BFV_BEHZ if is_behz else H.BFV_HPS)
    assert branch_name(H, dec.branch) == (want_branch or C.branch_name(T, is_behz)), msg
    run_decrypt(H, dec, plan, elems, s_eval, eval_form, want, msg)
    dec.close()
    plan.close()


@pytest.mark.parametrize("is_behz", [False, True], ids=["HPS", "BEHZ"])
@pytest.mark.parametrize("log_n,split,generic", FIXED_BFV)
def test_decrypt_plan_options(hip, log_n, split, generic, is_behz):
    """N = 2^13, 2^16 and 2^17 with every plan split of the ring size and with generic_moduli, 2 towers of 60
    bits, batch 2 at 2^13 and 1 above: 3 elements in coefficient form (three out-of-place forward
    plan_ntt_range, then the in-place inverse on scratch) and, at one split per ring, 2 in evaluation form"""
    H, ctx = hip
    key = (log_n, 2, 2 if log_n == 13 else 1)
    _run_call(H, ctx, key, 3, False, is_behz, (split, generic))
    if (split, generic) == ("SPLIT_COLS", 1):
        _run_call(H, ctx, key, 2, True, is_behz, (split, generic))


@pytest.mark.parametrize("is_behz", [False, True], ids=["HPS", "BEHZ"])
@pytest.mark.parametrize("eval_form", [False, True])
@pytest.mark.parametrize("towers", [9, 17])
def test_decrypt_many_towers(hip, towers, eval_form, is_behz):
    """9 and 17 towers at N = 2^8, 3 elements: past DEC_TILE and past 16 through the whole call (k_decrypt_core's
    row % size_q, the second and third tile of the scale-round kernels)"""
    H, ctx = hip
    _run_call(H, ctx, (8, towers, 2), 3, eval_form, is_behz)


# (t, the tower's bits): t < q / 2, and q <= 2 t (SwitchModulus by two subtractions) with an NTT-friendly q
ONE_TOWER_CALLS = [(T_PLAIN, 60), (1 << 29, 30)]


@pytest.mark.parametrize("is_behz", [False, True], ids=["HPS", "BEHZ"])
@pytest.mark.parametrize("eval_form", [False, True])
@pytest.mark.parametrize("t,bits", ONE_TOWER_CALLS)
@pytest.mark.parametrize("log_n", [4, 13])
def test_decrypt_one_tower(hip, log_n, t, bits, eval_form, is_behz):
    """one tower through the decrypt call (k_decrypt_core, the transforms, k_dec_one_tower) under either technique"""
    H, ctx = hip
    key = (log_n, 1, 2, t, (bits,))
    q = _call_case(*key)[0].q[0]
    assert (q <= 2 * t) == (bits == 30) and t <= q
    _run_call(H, ctx, key, 2 if eval_form else 3, eval_form, is_behz, want_branch="ONE_TOWER")


@pytest.mark.parametrize("log_n", [1, 2, 6])
def test_decrypt_small_ring_on_caller_stream(hip, delay, log_n):  # noqa: F811
    """N = 2, 4 and 64, 3 elements in coefficient form, 3 towers, batch 3: the whole call (scratch, three forward
    transforms, the inverse, three kernels on grids below one workgroup) ordered on the caller's stream alone"""
    H, ctx = hip
    key, batch = (log_n, 3, 3), 3
    T, r, _, s_eval, _ = _call_case(*key)
    elems, want = _call_ref(key, 3, False, False)
    plan = H.NTTPlan(ctx, log_n, T.q, r)
    dec = H.BfvDecrypt(ctx, log_n, T)
    run = OnStream(delay)
    ins = [run.input(e) for e in elems]
    ds = run.input(s_eval)
    out = run.output(batch, 1 << log_n)
    run.begin()
    dec.decrypt(plan, [t.data_ptr() for t in ins], ds.data_ptr(), out.data_ptr(), False, batch, run.h)
    run.fetch(out)
    same(run.wait()[0], want, f"log_n {log_n}")
    import torch

    torch.cuda.synchronize()
    dec.close()
    plan.close()


# --- scale-round on the fixed inputs ------------------------------------------------------------------
@pytest.mark.parametrize("name", list(C.LARGE_T))
def test_scale_round_large_t(hip, name):
    """t of 46-56 bits on up to 255 towers (F and H: intSum up to 64 bits, u2d(intSum) rounds, quot and
    td * double(quot) of 60 bits) and BEHZ at t = 2^32 - 1 and 2^32 - 5, on towers above and below t 2^26"""
    H, ctx = hip
    k = C.large_t_case(name)
    is_behz = k["technique"] == "BFV_BEHZ"
    want = D.scale_round_behz(k["x"], k["T"]) if is_behz else D.scale_round(k["x"], k["T"])
    _, branch = run_scale_round(H, ctx, k, getattr(H, k["technique"]), want, name)
    assert branch == ("BEHZ" if is_behz else name[0])


@pytest.mark.parametrize("c", C.EQUALS_T, ids=[D.case_id(c) for c in C.EQUALS_T])
def test_scale_round_equals_t(hip, c):
    """Q - e, e = 1 .. 32, and planted boundaries: the output is written as computed, so the device output holds
    a t wherever the reference's does (every one of the 32 under BEHZ)"""
    H, ctx = hip
    k = C.equals_t_case(c)
    T, is_behz = k["T"], c[0] == "BFV_BEHZ"
    want = D.scale_round_behz(k["x"], T) if is_behz else D.scale_round(k["x"], T)
    got, branch = run_scale_round(H, ctx, k, getattr(H, c[0]), want, D.case_id(c))
    assert branch == ("BEHZ" if is_behz else c[1])
    assert np.array_equal(got == U64(T.t), want == U64(T.t)) and (got <= U64(T.t)).all()
    if is_behz:
        assert (got[0, :C.EQUALS_E] == U64(T.t)).all()


@pytest.mark.parametrize("is_behz", [False, True], ids=["HPS", "BEHZ"])
@pytest.mark.parametrize("c", C.ONE_TOWER_WIDE, ids=[D.case_id(c) for c in C.ONE_TOWER_WIDE])
def test_scale_round_one_tower_wide(hip, c, is_behz):
    """the one-tower path at q <= 2 t (two csubs), t > q (no reduction), MR(v) >= q (umod64) and the wrapping
    q - MR(q - v), on every residue of the small q"""
    H, ctx = hip
    k = C.one_tower_wide_case(c)
    T = k["T"]
    want = D.one_tower(k["x"], T.q[0], T.t)
    _, branch = run_scale_round(H, ctx, k, H.BFV_BEHZ if is_behz else H.BFV_HPS, want, D.case_id(c))
    assert branch == "ONE_TOWER"


@pytest.mark.parametrize("name", list(C.TQT))
def test_times_q_over_t_wide(hip, name):
    """any 64-bit x_i (q_i, 2^63, 2^64 - 1, uniform words) at t = 2, 2^31, t > q_i, a 55-bit prime and 2^61 / 2^62;
    out of place, then in place.  ofhe_hip_bfv_decrypt_create admits 2 size_q t < 2^64 only: t = 2^62 on two
    towers is refused, and stands in decrypt_cases.TQT with its neighbours on either side of the limit"""
    H, ctx = hip
    k = C.tqt_case(name)
    T, x, batch = k["T"], k["x"], k["batch"]
    if name in C.TQT_REFUSED:
        with pytest.raises(H.MathError, match="below 2\\^64"):
            H.BfvDecrypt(ctx, k["log_n"], T)
        return
    want = D.times_q_over_t(x, T)
    dec = H.BfvDecrypt(ctx, k["log_n"], T)
    dx, out = dev(x), pattern(batch, len(T.q), k["n"])
    dec.times_q_over_t(dx.data_ptr(), out.data_ptr(), batch, stream())
    same(host(out), want, name)
    same(host(dx), x, name + ": the input changed")
    dec.times_q_over_t(dx.data_ptr(), dx.data_ptr(), batch, stream())
    same(host(dx), want, name + " in place")
    dec.close()
