"""Second test tier of the BSGS linear transform (ofhe_hip_ks_bsgs_transform and its stage calls):
what tests/test_gpu_linear_transform.py does not reach, bit for bit against
tests/linear_transform_ref.py.

The cases live in tests/linear_transform_cases.py (plain data, no GPU) and
tests/test_linear_transform_cases.py checks on the CPU what they reach:

* directed cases on the smallest rings: baby runs past KS_ROT_CAP, three term chunks of k_lt_inner
  with whole chunks absent, sum and term chunks in one call, more than 16 identity giants, three
  launches of k_lt_outer / k_lt_first, a runtime digit count with the 16-product reduction inside a
  digit set at the largest limb sums, indices not reduced mod 2N, one engine across levels and t,
  ragged chunks of the batched ModDown / ModUp, edge-heavy data, and the caller's stream;
* a seeded sweep: the key-switch draw of tests/tier2_cases.py (ring 2^4 .. 2^17, dnum, level, t,
  plan split, generic_moduli, separate_cols, separate_icol, chunk, single_stream) over towers of
  22-60 bits, with 1 .. 20 steps of either kind, identities anywhere, absent diagonals, padded
  diagonal strides and unreduced indices;
* a fixed grid at N = 2^13, 2^16 and 2^17 over every plan split x generic_moduli at two levels,
  one reference per (ring, level).

The reference takes the indices reduced mod 2N; the device gets them as they are.  Outputs start
as all-ones words, which no modulus admits."""
import numpy as np
import pytest

import keyswitch as K
import linear_transform_cases as C
import linear_transform_ref as LT
from leveled_cases import cached
from test_gpu_caller_stream import OnStream, delay  # noqa: F401  (delay is a fixture)
from test_gpu_fuzz_tier2 import _ks_options, _msg
from test_gpu_fuzz_tier3 import _top_column
from test_gpu_keyswitch import _ks_case, _uniform
from test_gpu_linear_transform import (EXTREME_CHAINS, Bsgs, _check, _mult_ext_sum, _rot_sum, _same, _stage_inputs,
                                       _top, nonid)
from test_gpu_parity import dev, host, stream

pytestmark = pytest.mark.gpu


def poison(*shape):
    import torch

    return torch.full(shape, -1, dtype=torch.int64, device="cuda")


def _engine(H, ctx, c, options=None):
    kp = C.params_of(c)
    return H.KeySwitch(ctx, c["log_n"], kp.q, kp.rq, kp.p, kp.rp, c["dnum"], options)


def _parity(bs, t, msg, want=None):
    """the call into poisoned outputs against the reference on reduced indices, the batch-1 call
    against its slice, inputs intact -> the reference"""
    want = C.reference(bs, t) if want is None else want
    out = poison(bs.B, bs.l, bs.n), poison(bs.B, bs.l, bs.n)
    assert _same(bs.run(t=t, out=out), want), msg
    if bs.B > 1:
        out = poison(1, bs.l, bs.n), poison(1, bs.l, bs.n)
        assert _same(bs.run(batch=1, t=t, out=out), [w[:1] for w in want]), "batch 1: " + msg
    assert bs.inputs_unchanged(), "inputs changed: " + msg
    return want


def _upload(bs):
    """after the host arrays were edited: the stored diagonals and every device copy again"""
    nd = len(bs.diag)
    bs.store[:, :bs.diag[0].size] = bs.diag.reshape(nd, -1)
    bs.d_c0, bs.d_c1, bs.d_diag = dev(bs.c0), dev(bs.c1), dev(bs.store)
    bs.d_bkeys = [None if k is None else (dev(k[0]), dev(k[1])) for k in bs.bkeys]
    bs.d_gkeys = [None if k is None else (dev(k[0]), dev(k[1])) for k in bs.gkeys]


# ---- A1, A3, A4: the launch chunking of the fused call ------------------------------------------------
@pytest.mark.parametrize("name", C.CHUNKED)
def test_bsgs_launch_chunking(hip, name):
    """a1_*: a baby run split at KS_ROT_CAP (the second k_ks_inner_rot call at r0 + i * per, i >= 16),
    runs around an identity, two and three term chunks of k_lt_inner (i0 = 32), whole chunks absent
    in the first and in a later launch.  a3_*: 17 identity giants (a second sum chunk of the identity
    rows, nadd > 16 in k_lt_outer, 2 + nid > 18 polynomials in the last ModDown), with no, 17 and 2
    rotated giants.  a4_*: three launches of k_lt_outer and k_lt_first (j0 = 32); g0 != 0 with acc = 1."""
    H, ctx = hip
    assert H.KS_ROT_CAP == C.KS_ROT_CAP
    i = C.CHUNKED.index(name)
    c = C.DIRECTED[i]
    ks = _engine(H, ctx, c)
    bs = C.build(c, Bsgs, ks, C.directed_seed(i))
    if all(k < 2 * bs.n for k in c["baby"] + c["giant"]):
        _check(bs, c["t"])
    _parity(bs, c["t"], name)
    ks.close()


# ---- A2: sum and term chunks together in the stage call -----------------------------------------------
@pytest.mark.parametrize("nterm,nsum", C.STAGE_SUMS)
def test_mult_ext_sum_sum_and_term_chunks(hip, nterm, nsum):
    """mult_ext_sum past LT_SUM_CAP and LT_TERM_CAP at once (g0 != 0 with acc = 1), with sums whose
    first chunk, a later chunk or every chunk is absent: into poisoned outputs, so that a first launch
    that contributes nothing must store zeros and an acc launch that contributes nothing must leave
    the stored sum alone."""
    H, ctx = hip
    c = C._directed("stage", 4, [1], [1])
    kp, ks = C.params_of(c), _engine(H, ctx, c)
    n, l, sp, B = 16, 4, 2, 2
    rng = np.random.default_rng(6000 + nterm + nsum)
    x0, x1, diag, _, _ = _stage_inputs(rng, kp, kp.q, kp.p, l, n, 2, B, nterm, nsum, 1)
    for present in (None, C.stage_present(nterm, nsum)):
        want = LT.mult_ext_sum_ref(kp, l, x0, x1, diag, present, nsum)
        assert _same(_mult_ext_sum(ks, l, sp, n, x0, x1, diag, present, nsum, B), want), (nterm, nsum, present)
        # batch 1 reads entry 0 of every term from the batch-2 stride
        assert _same(_mult_ext_sum(ks, l, sp, n, x0, x1, diag, present, nsum, 1), [w[:, :1] for w in want])
        d0, d1, dd = dev(x0), dev(x1), dev(diag)
        o0, o1 = poison(nsum, B, l + sp, n), poison(nsum, B, l + sp, n)
        ks.mult_ext_sum(l, nterm, d0.data_ptr(), d1.data_ptr(), B * (l + sp) * n, dd.data_ptr(), (l + sp) * n, present,
                        nsum, o0.data_ptr(), o1.data_ptr(), B, stream())
        assert _same((o0, o1), want), ("poisoned outputs", nterm, nsum, present)
    if present is not None:  # a sum without any diagonal is zero
        assert not want[0][3].any() and not want[1][nsum - 1].any()
    ks.close()


# ---- A5: a runtime digit count with the reduction inside a set ----------------------------------------
@pytest.mark.parametrize("chain", sorted(EXTREME_CHAINS))
def test_fast_rotation_ext_sum_runtime_beta_at_the_largest_limb_sums(hip, chain):
    """k_lt_outer<0> (beta = 5 and 6) with digits and keys all q_t - 1: 3 sets x 5 stay below the
    16-product reduction, 4 and 7 sets x 5 and 3 and 6 sets x 6 meet it inside a digit set; then the
    same sets on uniform words."""
    H, ctx = hip
    log_n, B = 4, 2
    n = 1 << log_n
    q6, rq6, p, rp = EXTREME_CHAINS[chain](log_n)
    for beta in sorted({b for b, _ in C.EXTREME_SETS}):
        q, rq = q6[:beta], rq6[:beta]
        kp = K.KeySwitchParams(n, q, rq, p, rp, beta)
        ks = H.KeySwitch(ctx, log_n, q, rq, p, rp, beta)
        l, sp, mods = beta, len(p), q + p
        assert ks.digits(l) == (1, beta) and kp.beta(l) == beta
        rng = np.random.default_rng(6100 + beta)
        for nset in [s for b, s in C.EXTREME_SETS if b == beta]:
            digits = _top((nset, B, beta, l + sp, n), mods)
            keys = [(_top((beta, l + sp, n), mods), _top((beta, l + sp, n), mods)) for _ in range(nset)]
            idx = [nonid(n, r) for r in range(nset)]
            want = LT.fast_rotation_ext_sum_ref(kp, digits, idx, keys)
            for e in range(2):
                for t, m in enumerate(mods):  # nset beta (m - 1)^2 = nset beta mod m
                    assert int(want[e][B - 1, t, n - 1]) == (nset * beta) % m
            assert _same(_rot_sum(ks, l, sp, n, digits, idx, keys, None, B), want), (beta, nset, "top")
            _, _, _, digits, keys = _stage_inputs(rng, kp, q, p, l, n, beta, B, 1, 1, nset)
            assert _same(_rot_sum(ks, l, sp, n, digits, idx, keys, None, B),
                         LT.fast_rotation_ext_sum_ref(kp, digits, idx, keys)), (beta, nset, "uniform")
        ks.close()


def test_fast_rotation_ext_sum_runtime_and_templated_beta_on_one_engine(hip):
    """Q 10, dnum 5: l = 10 and 9 take the runtime digit count (beta 5, 20 products: the reduction
    inside the fourth set), l = 8 the templated kernel (beta 4), one after the other on one engine."""
    H, ctx = hip
    log_n, sq, sp, dnum, B, nset = 4, 10, 2, 5, 2, 4
    n, q, rq, p, rp, kp, ks = _ks_case(H, ctx, log_n, sq, sp, dnum)
    rng = np.random.default_rng(6200)
    idx = [nonid(n, r) for r in range(nset)]
    for l in (10, 9, 8, 10):
        assert ks.digits(l)[1] == (4 if l == 8 else 5)
        _, _, _, digits, keys = _stage_inputs(rng, kp, q, p, l, n, dnum, B, 1, 1, nset)
        add = np.stack([_uniform(rng, B, q[:l] + p, n) for _ in range(2)])
        assert _same(_rot_sum(ks, l, sp, n, digits, idx, keys, None, B),
                     LT.fast_rotation_ext_sum_ref(kp, digits, idx, keys)), l
        assert _same(_rot_sum(ks, l, sp, n, digits, idx, keys, add, B),
                     LT.fast_rotation_ext_sum_ref(kp, digits, idx, keys, add)), (l, "addends")
    ks.close()


def test_bsgs_runtime_beta_with_four_rotated_giants(hip):
    H, ctx = hip
    c = C.FUSED_BETA5
    ks = _engine(H, ctx, c)
    assert ks.digits(c["level"])[1] == 5
    bs = C.build(c, Bsgs, ks, 6300)
    _check(bs, c["t"])
    _parity(bs, c["t"], c["name"])
    ks.close()


# ---- A6: indices that are not reduced mod 2N ----------------------------------------------------------
def test_bsgs_unreduced_indices(hip):
    """A rotated baby goes through inv_odd32 of the raw index and a rotated giant raw into rot_dest:
    k + 2N and k + 4N, the conjugation 2N - 1 as a baby and as a giant, 2^32 - 1 as a giant, and one
    index twice in a list under two keys.  Each equals the reference on the reduced indices."""
    H, ctx = hip
    n = 16
    k = [nonid(n, r) for r in range(4)]
    top = (1 << 32) - 1
    assert top % (2 * n) == 2 * n - 1
    lists = [([1, k[0] + 2 * n, 2 * n - 1], [k[1] + 4 * n, 2 * n - 1, 4 * n + 1]),
             ([k[0] + 4 * n, 1, k[0]], [k[2] + 2 * n, top, k[2]]),
             ([top, 2 * n + 1], [top - 2 * n, k[3] + (1 << 31)])]
    c0 = C._directed("indices", 4, [1], [1])
    ks = _engine(H, ctx, c0)
    for i, (baby, giant) in enumerate(lists):
        c = dict(c0, baby=baby, giant=giant, t=65537 * (i % 2))
        bs = C.build(c, Bsgs, ks, 6400 + i)
        want = _parity(bs, c["t"], str((baby, giant)))
        # the same data under the reduced indices: the device's words do not move either
        red = C.build(dict(c, baby=[b % (2 * n) for b in baby], giant=[g % (2 * n) for g in giant]), Bsgs, ks, 6400 + i)
        assert np.array_equal(red.c0, bs.c0) and np.array_equal(red.diag, bs.diag)
        assert _same(red.run(t=c["t"]), want)
    ks.close()


# ---- A7: one engine across levels and t ---------------------------------------------------------------
def test_bsgs_one_engine_across_levels_and_t(hip):
    """The KsLevel cache and the per-level t tables revisited: (l, t) = (Q, 0), (1, 65537), (Q, 3),
    (Q - 1, 0), (Q, 0), (1, 65537) on one KeySwitch; every call equals its own reference and every
    repeat the first call's words."""
    H, ctx = hip
    n, Q = 16, 4
    c0 = C._directed("levels", 4, [1, nonid(n, 0), nonid(n, 1)], [nonid(n, 2), 1, nonid(n, 3)],
                     present=[1, 1, 1, 1, 1, 1, 1, 0, 1])
    ks = _engine(H, ctx, c0)
    cases, first = {}, {}
    for l, t in [(Q, 0), (1, 65537), (Q, 3), (Q - 1, 0), (Q, 0), (1, 65537)]:
        if l not in cases:
            cases[l] = C.build(dict(c0, level=l), Bsgs, ks, 6500 + l)
        bs = cases[l]
        _parity(bs, t, f"level {l} t {t}")
        got = [host(o) for o in bs.run(t=t)]
        if (l, t) in first:
            assert all(np.array_equal(a, b) for a, b in zip(got, first[(l, t)])), ("repeat", l, t)
        first.setdefault((l, t), got)
    assert len(first) == 4
    ks.close()


# ---- A8: ragged chunks of the batched ModDown and ModUp ----------------------------------------------
RAGGED = C._directed("ragged_chunks", 6, [1, nonid(64, 0)], [nonid(64, 1), nonid(64, 2), 1, nonid(64, 3)],
                     present=[1, 1, 1, 1, 1, 1, 1, 0], sq=5, sp=3, batch=3, t=65537)


@pytest.mark.parametrize("chunk,single_stream", [(1, 0), (2, 0), (4, 0), (4, 1)])
def test_bsgs_ragged_chunks(hip, chunk, single_stream):
    """batch 3 x 3 rotated giants = 9 entries through the batched ModDown and ModUp in chunks of 1,
    of 2 (a ragged last chunk of 1), of 4 (4 + 4 + 1), and of 4 without side streams."""
    H, ctx = hip
    assert C.launch_plan(RAGGED["baby"], RAGGED["giant"], 64, 3)["nrot"] * RAGGED["batch"] == 9
    ks = _engine(H, ctx, RAGGED, H.KsOptions(chunk=chunk, single_stream=single_stream))
    bs = C.build(RAGGED, Bsgs, ks, 6600)
    want = cached(("ragged",), lambda: C.reference(bs, RAGGED["t"]))
    _parity(bs, RAGGED["t"], f"chunk {chunk} single_stream {single_stream}", want)
    ks.close()


# ---- A9: edge-heavy data -----------------------------------------------------------------------------
EDGES = ["zero_ciphertext", "zero_c1", "diagonal_columns", "key_column", "zero_diagonal"]


@pytest.mark.parametrize("edge", EDGES)
def test_bsgs_edge_heavy_data(hip, edge):
    """c0 = c1 = 0; c1 = 0; diagonals with a zero column and a q_t - 1 column; keys with a q_t - 1
    column; one diagonal identically zero but marked present -- on the mixed chain."""
    H, ctx = hip
    n = 16
    c = C._directed(edge, 4, [1, nonid(n, 0), nonid(n, 1)], [nonid(n, 2), 1, nonid(n, 3)], t=65537)
    ks = _engine(H, ctx, c)
    bs = C.build(c, Bsgs, ks, 6700 + EDGES.index(edge))
    mods = bs.kp.q + bs.kp.p
    if edge == "zero_ciphertext":
        bs.c0[:], bs.c1[:] = 0, 0
    elif edge == "zero_c1":
        bs.c1[:] = 0
    elif edge == "diagonal_columns":
        bs.diag[..., 2] = 0
        _top_column(bs.diag, mods, 5)
        _top_column(bs.c0, bs.kp.q, 5)
        _top_column(bs.c1, bs.kp.q, 5)
    elif edge == "key_column":
        for key in bs.bkeys + bs.gkeys:
            if key is not None:
                _top_column(key[0], mods, 7)
                _top_column(key[1], mods, 7)
    else:
        bs.diag[4] = 0
    _upload(bs)
    want = _parity(bs, c["t"], edge)
    if edge == "zero_ciphertext":
        assert not want[0].any() and not want[1].any()
    ks.close()


# ---- A10: the caller's stream ------------------------------------------------------------------------
def test_bsgs_three_launches_on_caller_stream(hip, delay):  # noqa: F811
    """33 rotated giants (three launches of k_lt_outer and k_lt_first, three sum chunks) and 18
    rotated babies (two k_ks_inner_rot calls, two term chunks) from a caller's stream, waited on
    through that stream alone."""
    H, ctx = hip
    n, B = 8, 2
    c = C._directed("caller_stream", 3, [nonid(n, r) for r in range(18)], [nonid(n, r) for r in range(33)],
                    present=[1] * (18 * 33 - 1) + [0], batch=B, t=65537)
    p = C.launch_plan(c["baby"], c["giant"], n, 2)
    assert len(p["outer"]) == 3 and len(p["baby_runs"]) == 2
    ks = _engine(H, ctx, c)
    bs = C.build(c, Bsgs, ks, 6800)
    st = OnStream(delay)
    bs.d_c0, bs.d_c1 = st.input(bs.c0), st.input(bs.c1)
    bs.d_diag = st.input(bs.store)
    bs.d_bkeys = [None if k is None else (st.input(k[0]), st.input(k[1])) for k in bs.bkeys]
    bs.d_gkeys = [None if k is None else (st.input(k[0]), st.input(k[1])) for k in bs.gkeys]
    o0, o1 = st.output(B, bs.l, n), st.output(B, bs.l, n)
    st.begin()
    bs.run(t=c["t"], s=st.h, out=(o0, o1))
    st.fetch(o0, o1)
    got = st.wait()
    assert all(np.array_equal(a, b) for a, b in zip(got, C.reference(bs, c["t"])))
    import torch

    torch.cuda.synchronize()
    assert bs.inputs_unchanged()
    ks.close()


# ---- B: the seeded sweep -----------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(C.SEEDS * C.SCALE))
def test_fuzz_linear_transform(hip, seed):
    H, ctx = hip
    c = C.case(seed)
    msg = _msg({k: v for k, v in c.items() if k != "present"})
    kp = K.KeySwitchParams(1 << c["log_n"], c["q"], c["rq"], c["p"], c["rp"], c["dnum"])
    ks = H.KeySwitch(ctx, c["log_n"], c["q"], c["rq"], c["p"], c["rp"], c["dnum"], _ks_options(H, c))
    assert ks.digits(c["level"]) == (kp.alpha, c["beta"])
    bs = C.build(c, Bsgs, ks, c["data_seed"])
    assert bs.diag_stride == (c["level"] + c["size_p"]) * bs.n + c["pad"]
    _parity(bs, c["t"], msg)
    ks.close()


# ---- C: the fixed grid on the large rings ------------------------------------------------------------
def _grid(log_n, level):
    """one set of inputs (host and device) and one reference per (ring, level)"""
    def make():
        bs = C.build(C.grid_case(log_n, level), Bsgs, None, 6900 + log_n + level)
        return bs, C.reference(bs, C.grid_case(log_n, level)["t"])
    return cached(("lt_grid", log_n, level), make)


@pytest.mark.parametrize("log_n,level,split,generic,option", C.GRID)
def test_bsgs_plan_splits_on_the_large_rings(hip, log_n, level, split, generic, option):
    """N = 2^13, 2^16, 2^17 with 4 + 2 towers of 60, 22 (2^17: 23), 45, 31 | 59, 36 bits, at level Q
    and Q - 1, under every plan split x generic_moduli and, at 2^17, separate_cols and
    separate_icol: the words cannot depend on the engine."""
    H, ctx = hip
    c = C.grid_case(log_n, level)
    opt = H.KsOptions()
    opt.plan = H.PlanOptions(getattr(H, split), generic)
    if option:
        setattr(opt, option, 1)
    bs, want = _grid(log_n, level)
    bs.ks = _engine(H, ctx, c, opt)
    _parity(bs, c["t"], f"log_n {log_n} level {level} {split} generic {generic} {option}", want)
    bs.ks.close()
