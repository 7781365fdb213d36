"""CPU tests of the BFV (HPS family) restatement in tests/bfv_ref.py and of the
tables of upmem--openfhe_amd/bfv_tables.py: the reference's known answer, the
mathematical definitions with exact integers, the sensitivity of alpha to the
order / fusing of the double sum (what lets the GPU parity test see a
contracted or reordered sum), both alpha branches of ScaleAndRound, and
encrypt -> EvalMult -> decrypt end to end."""
from fractions import Fraction

import numpy as np
import pytest
from conftest import load_golden

import bfv_ref as R
import bfv_tables as BT

REF = load_golden("reference_fixtures.json")
T_PLAIN = 65537


def chain(O, log_n, sq, sp, bits=60):
    m, r = O.moduli_chain(log_n, sq + sp, bits)
    return m[:sq], r[:sq], m[sq:], r[sq:]


def test_kat_switch_crt_basis(O):
    """UnitTestBFVrnsCRTOperations.cpp:290-376: towers 0-1 of FastExpandCRTBasisPloverQ's answer are
    SwitchCRTBasis(R -> Q) of its R towers; the whole restatement gives both halves."""
    k = REF["kat_fast_expand_crt_basis"]
    q, r = k["q"], k["r"]
    rl = np.array(k["expected_rl"], dtype=np.uint64).reshape(1, 2, 8)
    assert R.switch_crt_basis(rl, r, q)[0].tolist() == k["expected_ql"]
    T = BT.BfvTables(q, r, T_PLAIN, BT.HPSPOVERQ)
    full = R.fast_expand_p_over_q(O, np.array(k["x"], dtype=np.uint64).reshape(1, 2, 8), T)
    assert full[0, :2].tolist() == k["expected_ql"]
    assert full[0, 2:].tolist() == k["expected_rl"]
    # the scalar (Python float) and the vectorised (float64) sums are the same doubles
    ys = R.switch_ys(rl, r)
    nu = R.nu_switch(ys, r)
    for c in range(8):
        assert R.nu_switch_scalar([int(y[0, c]) for y in ys], r) == nu[0, c]


SWITCH_CASES = [(3, 1, 1, 60), (3, 2, 2, 60), (5, 3, 4, 60), (12, 16, 17, 60), (12, 17, 3, 60), (8, 4, 5, 40),
                (8, 3, 4, 30)]


@pytest.mark.parametrize("log_n,sq,sp,bits", SWITCH_CASES)
def test_switch_is_the_centred_representative(O, log_n, sq, sp, bits):
    """Away from the rounding boundary (|v/Q - 1/2| >= 2^-40, exact rationals) the exact switch gives
    the centred representative of x, in [-Q/2, Q/2), mod p_j.  No uniform input is that close to the
    boundary; the planted ones are, and are left to the parity tests."""
    q, _, p, _ = chain(O, log_n, sq, sp, bits)
    n = min(1 << log_n, 512)
    x, kinds = R.switch_inputs(q, n, 1, 7 + sq)
    out = R.switch_crt_basis(x, q, p)
    Q = BT.product(q)
    v = R.crt_lift(x, q)[0]
    near = np.array([abs(Fraction(int(a), Q) - Fraction(1, 2)) < Fraction(1, 1 << 40) for a in v])
    assert not near[kinds[0] == R.UNIFORM].any()
    check = ~near & (kinds[0] != R.PLANTED)
    assert check.sum() >= n // 2
    centred = np.where(v * 2 >= Q, v - Q, v)
    for j, pj in enumerate(p):
        assert (R.obj(out[0, j])[check] == (centred % pj)[check]).all()


@pytest.mark.parametrize("log_n,sq,sp", R.SWITCH_CASES)
def test_planted_inputs_tell_fused_from_separate_rounding(O, log_n, sq, sp):
    """On the very inputs of every GPU switch case (bfv_ref.switch_case: the same moduli, N, batch
    and seed, the one-tower and the mixed generic_moduli case included), a fused multiply-add chain
    gives a different alpha from the reference's separately rounded sum on at least one planted
    coefficient, and coefficient 0 is such a one -- so a kernel that contracts (or reorders) the sum
    cannot pass the parity tests, with batch 1 or 3.  Cases of at least 2048 coefficients plant 1024."""
    q, _, x, kinds = R.switch_case(O, log_n, sq, sp)
    flat = kinds.reshape(-1)
    sel = np.flatnonzero(flat == R.PLANTED)
    total = x.shape[0] * x.shape[2]
    assert len(sel) >= (1024 if total >= 2048 else 1)
    ys = R.switch_ys(x, q)
    ref = R.nu_switch(ys, q).astype(np.int64).reshape(-1)
    hot = []
    for c in sel:
        yc = [int(y.reshape(-1)[c]) for y in ys]
        assert int(R.nu_switch_scalar(yc, q)) == ref[c]
        if int(R.nu_switch_fused(yc, q)) != ref[c]:
            hot.append(c)
    print(f"({log_n}, {sq}, {sp}): fused alpha differs on {len(hot)} of {len(sel)} planted coefficients")
    assert len(hot) >= 1 and hot[0] == 0


def _hot_planted(x, kinds, q):
    """indices (flat, batch-major) of the planted coefficients on which a fused sum gives another alpha"""
    sel = np.flatnonzero(kinds.reshape(-1) == R.PLANTED)
    ys = R.switch_ys(x, q)
    ref = R.nu_switch(ys, q).astype(np.int64).reshape(-1)
    hot = []
    for c in sel:
        yc = [int(y.reshape(-1)[c]) for y in ys]
        assert int(R.nu_switch_scalar(yc, q)) == ref[c]
        if int(R.nu_switch_fused(yc, q)) != ref[c]:
            hot.append(c)
    return sel, hot


def _extremes_reach_the_last_alpha(x, kinds, q, p):
    """the three extreme columns of every batch entry: y_i = q_i - 1 gives alpha = size_q (the last row
    of alphaQModp, which alpha_of's clamp guards), and the digit columns hold the y_i they claim"""
    n = x.shape[2]
    assert (kinds[:, n - 3:] == R.EXTREME).all() and (kinds[:, :n - 3] != R.EXTREME).all()
    _, alpha = R.switch_crt_basis(x, q, p, want_alpha=True)
    assert (alpha[:, n - 3] == len(q)).all()
    if len(q) >= 12:  # with many sources nothing else gets there
        assert alpha[kinds != R.EXTREME].max() < len(q)
    ys = R.switch_ys(x, q)
    for i, m in enumerate(q):
        assert (ys[i][:, n - 3] == m - 1).all()
        assert (ys[i][:, n - 2] == min(m - 1, R.DIGITS_MAX)).all() and (ys[i][:, n - 1] == R.DIGITS_MIN % m).all()


@pytest.mark.parametrize("log_n,sq,sp", R.SWITCH_CASES_MMA)
def test_mma_cases_planted_and_extreme_inputs(O, log_n, sq, sp):
    """bfv_ref.SWITCH_CASES_MMA as test_planted_inputs_tell_fused_from_separate_rounding has it for
    SWITCH_CASES: at 12 .. 64 sources a fused chain still gives another alpha on planted coefficients
    (coefficient 0 among them), in batch entry 0 alone too; plus the extreme columns."""
    q, p, x, kinds = R.switch_case_mma(O, log_n, sq, sp)
    sel, hot = _hot_planted(x, kinds, q)
    print(f"({log_n}, {sq}, {sp}): fused alpha differs on {len(hot)} of {len(sel)} planted coefficients")
    assert len(sel) == x.shape[0] * x.shape[2] // 4
    assert len(hot) >= 1 and hot[0] == 0
    _extremes_reach_the_last_alpha(x, kinds, q, p)


def test_mma_case_table():
    """The K-step count, the target chunks and the reduction variant of every SWITCH_CASES_MMA entry,
    from the host's arithmetic restated in bfv_ref (bconv_mma_table / bconv_mma_lds: 1 KiB of
    fragments per tile and K-step, a 64-byte row per target, a 32-byte row per source, 64 KiB)."""
    assert [R.mma_ks(sq) for _, sq, _ in R.SWITCH_CASES_MMA] == [3, 6, 7, 8, 10, 12, 14, 16]
    reached = {R.mma_ks(sq) for _, sq, _ in R.SWITCH_CASES + R.SWITCH_CASES_MMA if sq <= 64}
    assert reached == set(range(1, 9)) | {10, 12, 14, 16}  # every instantiation of k_switch_mma
    chunks = {}
    for log_n, sq, sp in R.SWITCH_CASES_MMA:
        assert log_n >= 5  # the matrix-core kernel needs a wave of 32 coefficients
        tiles, tpc = R.mma_tpc(sq, sp)
        chunks[(log_n, sq, sp)] = -(-tiles // tpc)
    assert R.mma_tpc(32, 28) == (7, 7) and R.mma_tpc(32, 29) == (8, 7)  # KS 8: a second chunk from 29 targets
    assert R.mma_tpc(64, 12) == (3, 3) and R.mma_tpc(64, 13) == (4, 3)  # KS 16: from 13 targets
    assert [c for c, v in chunks.items() if v >= 2] == [(6, 32, 29), (6, 64, 13)]
    assert all(R.mma_ks(sq) == ks for (_, sq, _), ks in R.SWITCH_MMA_MIXED.items())
    assert sorted(R.SWITCH_MMA_MIXED.values()) == [6, 12]  # no special-prime reduction below and above KS 8


@pytest.mark.parametrize("log_n,sq,sp", R.SWITCH_CASES_MMA)
def test_mma_case_reduction_variant(O, log_n, sq, sp):
    """mm_spq of each chain: the 60-bit chain's targets are 2^60 - d (special-prime reduction), the
    mixed generic chain's are not; the mixed chain holds a tower below 32 bits and one of 60"""
    q, p, _, _ = R.switch_case_mma(O, log_n, sq, sp)
    mixed = (log_n, sq, sp) in R.SWITCH_MMA_MIXED
    assert R.mma_spq(p) == (not mixed)
    if mixed:
        bits = {m.bit_length() for m in q + p}
        assert min(bits) < 32 and max(bits) == 60
    assert len(set(q + p)) == sq + sp


def test_switch_cap_case(O):
    """SWITCH_CAP_CASE has more blocks than the matrix-core kernel's grid cap, a partial second trip
    of the group loop whose coefficients (batch entry 3) carry sensitive planted values too."""
    blocks_per_cu, cus = 3, 256  # BCONV_MMA_BLOCKS_PER_CU (csrc/bconv_mma.hpp) and the grid cap's CU count
    log_n, sq, sp = R.SWITCH_CAP_CASE
    q, p, x, kinds = R.switch_case_cap(O)
    tiles, tpc = R.mma_tpc(sq, sp)
    chunks = -(-tiles // tpc)
    cap = cus * blocks_per_cu // chunks
    blocks = R.SWITCH_CAP_BATCH * (1 << log_n) // 256  # 8 waves of 32 coefficients each
    assert cap < blocks < 2 * cap and (cap, blocks) == (768, 1024)
    assert R.mma_ks(sq) == 1 and R.mma_spq(p)
    sel, hot = _hot_planted(x, kinds, q)
    first_of_second_trip = cap * 256
    assert hot[0] == 0 and any(c >= first_of_second_trip for c in hot)
    _extremes_reach_the_last_alpha(x, kinds, q, p)


@pytest.mark.parametrize("log_n,sq,sp", R.SWITCH_CASES + R.SWITCH_CASES_MMA)
def test_fast_switch_is_the_exact_one(O, log_n, sq, sp):
    """bfv_ref's 64-bit-word path (fast = True) gives the residues of the Python-integer path on the
    planted, special and extreme inputs of every GPU switch case, 22-bit to 60-bit towers"""
    mma = (log_n, sq, sp) in R.SWITCH_CASES_MMA
    q, p, x, _ = (R.switch_case_mma if mma else R.switch_case)(O, log_n, sq, sp)
    x = x[:, :, :256]
    assert np.array_equal(R.switch_crt_basis(x, q, p, fast=True), R.switch_crt_basis(x, q, p))


def test_fast_word_products():
    """mulmod_const against Python integers on boundary words and moduli of 22 to 62 bits"""
    rng = np.random.default_rng(5)
    for m in (4194301, (1 << 31) - 1, (1 << 32) + 15, (1 << 60) - 93, (1 << 62) + 135, (1 << 63) - 25):
        a = np.concatenate([np.array([0, 1, m - 1, m, 2 * m - 1, (1 << 64) - 1, 1 << 63, (1 << 32) - 1, 1 << 32],
                                     dtype=np.uint64), rng.integers(0, 1 << 64, size=500, dtype=np.uint64)])
        for c in (0, 1, m - 1, m // 2, int(rng.integers(0, m))):
            assert R.mulmod_const(a, c, m).tolist() == [int(v) * c % m for v in a]


@pytest.mark.parametrize("tech,sq,sr", [(BT.HPS, 2, 3), (BT.HPSPOVERQ, 2, 2), (BT.HPS, 5, 5)])
def test_fast_eval_mult_is_the_exact_one(O, tech, sq, sr):
    """EvalMult and ExpandCRTBasis (ScaleAndRound and both switches inside) by the two paths, on a
    60-bit and on a mixed 22-60-bit chain"""
    from test_mixed_moduli_oracle import mixed_chain

    log_n, n = 6, 64
    for m, rt in (O.moduli_chain(log_n, sq + sr), mixed_chain(log_n, R.MIXED_BITS[:sq + sr], generic=True)):
        q, rq, r, rr = m[:sq], rt[:sq], m[sq:], rt[sq:]
        T = BT.BfvTables(q, r, T_PLAIN, tech)
        ring = R.Ring(O, log_n, q, rq, r, rr)
        cts = [O.uniform_dcrt(2, sq, n, q, 60 + k) for k in range(4)]
        for c in cts:
            c[:, :, :3] = np.array([[0, 1, v - 1] for v in q], dtype=np.uint64)
        for a, b in zip(R.eval_mult(O, T, ring, *cts, fast=True), R.eval_mult(O, T, ring, *cts)):
            assert np.array_equal(a, b)
        for ev in (False, True):
            assert np.array_equal(R.expand_crt_basis(O, cts[0], q, r, ring.tb_q, ring.tb_r, ev, fast=True),
                                  R.expand_crt_basis(O, cts[0], q, r, ring.tb_q, ring.tb_r, ev))


SR_CASES = [(2, 60), (4, 60), (16, 60), (4, 40), (3, 30)]


@pytest.mark.parametrize("out_is_q", [False, True])
@pytest.mark.parametrize("towers,bits", SR_CASES)
def test_scale_and_round_definition(O, towers, bits, out_is_q):
    """ScaleAndRound's output is round(t x / Q) mod r_j (HPS; round(t x / R) mod q_i for HPSPOVERQ)
    up to the rounding error of the double sum: size_i (size_i + 5) max(s) 2^-53 + 1 (each of the
    size_i terms carries the error of frac, of double(x_i), of the product and of up to size_i
    partial sums, relative 2^-53 each, on values below max(s)); towers of at most 40 bits convert
    and multiply almost exactly, so the error is at most 1."""
    sq = towers
    sp = towers if out_is_q else towers + 1
    q, _, r, _ = chain(O, 8, sq, sp, bits)
    T = BT.BfvTables(q, r, T_PLAIN, BT.HPSPOVERQ if out_is_q else BT.HPS)
    rng = np.random.default_rng(towers * 100 + bits)
    n = 256
    QR = T.Q * T.R
    v = np.array([int.from_bytes(rng.bytes(300), "little") % QR for _ in range(n)], dtype=object).reshape(1, n)
    x = R.residues(v, q + r)
    out = R.scale_and_round(x, q, r, out_is_q, T.sr_table, T.sr_frac)
    outs, den = (q, T.R) if out_is_q else (r, T.Q)
    M = BT.product(outs)
    want = np.array([(2 * T_PLAIN * int(a) + den) // (2 * den) for a in v[0]], dtype=object)
    diff = (R.crt_lift(out, outs)[0] - want) % M
    diff = np.where(diff * 2 >= M, diff - M, diff)
    worst = max(abs(int(d)) for d in diff)
    si = sp if out_is_q else sq
    bound = 1 if bits <= 40 else int(si * (si + 5) * max(r if out_is_q else q) * 2.0 ** -53) + 1
    print(f"{towers} x {bits}-bit, out_is_q = {out_is_q}: worst centred error {worst}, bound {bound}")
    assert worst <= bound


@pytest.mark.parametrize("out_is_q", [False, True])
def test_scale_and_round_both_alpha_branches(O, out_is_q):
    """17 summed 60-bit towers with frac = 1 - 2^-53: nu > 2^64 where x_i = q_i - 1 (the reference's
    128-bit branch) and nu < 2^64 elsewhere (its native branch); both are floor(nu) mod o_j, checked
    here against a per-coefficient restatement with Python floats."""
    q, p, table, frac, x = R.two_branch_case(O, 5, 11, out_is_q)
    out, nu = R.scale_and_round(x, q, p, out_is_q, table, frac, want_nu=True)
    even = np.arange(32) % 2 == 0
    assert (nu[0][even] > 2.0 ** 64).all() and (nu[0][~even] < 2.0 ** 64).all()
    xin, xown, outs = (x[0, 17:], x[0, :17], q) if out_is_q else (x[0, :17], x[0, 17:], p)
    for c in range(32):
        f = 0.5
        for i in range(17):
            f = f + (frac[i] * float(int(xin[i, c])))
        assert f == nu[0, c]
        for j, oj in enumerate(outs):
            cur = sum(int(xin[i, c]) * table[j][i] for i in range(17)) + int(xown[j, c]) * table[j][17]
            assert int(out[0, j, c]) == (cur % oj + int(f) % oj) % oj


@pytest.mark.parametrize("log_n", [4, 8])
@pytest.mark.parametrize("tech,sq,sr", [(BT.HPS, 2, 3), (BT.HPSPOVERQ, 2, 2)])
def test_eval_mult_decrypts_to_the_product(O, log_n, tech, sq, sr):
    """Encrypt two random plaintexts under a ternary secret (error bound 3), multiply with the
    restated EvalMult, decrypt the 3-element result with exact integers: the negacyclic product mod t."""
    q, rq, r, rr = chain(O, log_n, sq, sr)
    T = BT.BfvTables(q, r, T_PLAIN, tech)
    ring = R.Ring(O, log_n, q, rq, r, rr)
    rng = np.random.default_rng(log_n * 10 + tech)
    n = 1 << log_n
    s = np.array([int(v) for v in rng.integers(-1, 2, size=n)], dtype=object)
    m1 = np.array([int(v) for v in rng.integers(0, T_PLAIN, size=n)], dtype=object)
    m2 = np.array([int(v) for v in rng.integers(0, T_PLAIN, size=n)], dtype=object)
    c0, c1 = R.encrypt(O, rng, m1, s, q, ring.tb_q, T_PLAIN)
    d0, d1 = R.encrypt(O, rng, m2, s, q, ring.tb_q, T_PLAIN)
    outs = R.eval_mult(O, T, ring, c0, c1, d0, d1)
    got = R.decrypt3(outs, s, q, T_PLAIN)
    assert (got == R.negacyclic(m1, m2) % T_PLAIN).all()
