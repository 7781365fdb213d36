"""behz_ref (the CPU restatement of the BEHZ functions) against the reference's
known answer and against the exact-integer definitions of the three functions,
and the coverage conditions of the GPU cases on the very draws the GPU tests
use.  CPU only; integers only, every comparison is exact."""
import numpy as np
import pytest

import behz_ref as Z
import bfv_ref as BR
import bfv_tables as BT

KAT = Z.load_vectors()


def test_known_answer_through_behz_expand(O):
    """UnitTestBFVrnsCRTOperations.cpp:197-287: evaluation-form input, N = 8, two towers; B and msk
    are the ones behz_bases chooses"""
    b, msk, _ = Z.behz_bases(O, KAT["log_n"], KAT["q"], KAT["t"])
    assert b + [msk] == KAT["bsk"]
    T = BT.BehzTables(KAT["q"], b, msk, KAT["t"])
    ring = Z.Ring(O, KAT["log_n"], T)
    x = np.array([KAT["x"]], dtype=np.uint64)
    got = Z.behz_expand(O, x, T, ring, True)
    assert np.array_equal(got[0], np.array(KAT["expected"], dtype=np.uint64))
    # the same polynomial handed over in coefficient form
    assert np.array_equal(Z.behz_expand(O, O.ntt_inv(x, ring.tb_q), T, ring, False), got)


def definition_chains(O):
    """chains of 1-4 towers, 22-60 bits: (log_n, q, b, msk)"""
    from test_mixed_moduli_oracle import mixed_chain

    out = []
    for log_n, bits in [(3, [60]), (4, [60, 60]), (4, [22, 45, 31, 60]), (5, [40, 36, 54]), (4, [27, 58])]:
        q = mixed_chain(log_n, bits, generic=True)[0]
        b, msk, _ = Z.behz_bases(O, log_n, q, Z.T_PLAIN)
        out.append((log_n, q, b, msk))
    m = O.moduli_chain(4, 7)[0]
    out.append((4, m[:2], m[2:6], m[6]))  # size_b != size_q
    return out


def test_q_to_bsk_definition(O):
    """v = sum_i y_i Q / q_i, r_c the centred r: out_j = ((v + r_c Q) / 2^16) mod b_j; the division is
    exact and the quotient is = x (mod Q)"""
    rng = np.random.default_rng(1)
    for log_n, q, b, msk in definition_chains(O):
        T = BT.BehzTables(q, b, msk, Z.T_PLAIN)
        n = 1 << log_n
        x = np.stack([np.stack([rng.integers(0, m, size=n, dtype=np.uint64) for m in q]) for _ in range(2)])
        out, r = Z.q_to_bsk(x, T, want_r=True)
        X = BR.crt_lift(x, q)
        ys = [BR.obj(x[:, i, :]) * T.mtildeQHatInvModq[i] % q[i] for i in range(len(q))]
        v = sum(y * (T.Q // qi) for y, qi in zip(ys, q))
        rc = np.where(r >= 0x8000, r - 0x10000, r).astype(object)
        num = v + rc * T.Q
        assert not (num % BT.MTILDE).any()
        quo = num // BT.MTILDE
        assert not ((quo - X) % T.Q).any()
        for j, bj in enumerate(T.bsk):
            assert np.array_equal(out[:, j, :], BR.u64(quo % bj))


def test_floor_definition(O):
    """for any integer X given by its residues: out_j = ((t X - v') / Q) mod b_j, v' = sum_i y_i Q / q_i"""
    rng = np.random.default_rng(2)
    for log_n, q, b, msk in definition_chains(O):
        T = BT.BehzTables(q, b, msk, Z.T_PLAIN)
        n = 1 << log_n
        M = T.Q * T.B * msk
        X = np.array([int.from_bytes(rng.bytes(64), "little") % M for _ in range(2 * n)], dtype=object).reshape(2, n)
        x = BR.residues(X, T.q + T.bsk)
        keep = x.copy()
        out = Z.floor_q(x, T)
        assert np.array_equal(x, keep)  # the input is not modified
        ys = [BR.obj(x[:, i, :]) * T.tQHatInvModq[i] % q[i] for i in range(len(q))]
        v = sum(y * (T.Q // qi) for y, qi in zip(ys, q))
        num = Z.T_PLAIN * X - v
        assert not (num % T.Q).any()
        for j, bj in enumerate(T.bsk):
            assert np.array_equal(out[:, j, :], BR.u64(num // T.Q % bj))


def test_sk_definition_and_the_wrapping_case(O):
    """for every integer |Y| < B (msk / 2 - size_b): out_j = Y mod q_j, also on a chain with a tower
    below msk / 2, where the reference's unsigned ModSubFast gives another word"""
    rng = np.random.default_rng(3)
    told_apart = 0
    for log_n, q, b, msk in definition_chains(O):
        T = BT.BehzTables(q, b, msk, Z.T_PLAIN)
        n = 1 << log_n
        bound = T.B * (msk // 2 - len(b))
        Y = np.array([int.from_bytes(rng.bytes(64), "little") % (2 * bound - 1) - (bound - 1) for _ in range(2 * n)],
                     dtype=object).reshape(2, n)
        Y[0, :4] = [0, bound - 1, 1 - bound, -1]
        x = BR.residues(Y, T.bsk)
        out, alpha = Z.conv_sk(x, T, want_alpha=True)
        assert np.array_equal(out, BR.residues(Y, q))
        assert (alpha < msk).all()
        wrapped = Z.conv_sk(x, T, wrapping=True)
        if min(q) * 2 > msk:
            assert np.array_equal(wrapped, out)  # msk < 2 min q: the reference does not wrap
        elif not np.array_equal(wrapped, out):
            told_apart += 1
            small = [j for j, qj in enumerate(q) if qj < msk // 2]
            assert small and all((wrapped[:, j, :] == out[:, j, :]).all() for j in range(len(q)) if j not in small)
    assert told_apart >= 1, "no chain with a tower below msk / 2 told the centred definition from the wrapping one"


def test_fast_path_equals_exact_integers(O):
    c = Z.case(O, "tile1")
    T = c["T"]
    assert np.array_equal(Z.q_to_bsk(c["xq"], T, fast=True), Z.q_to_bsk(c["xq"], T))
    assert np.array_equal(Z.floor_q(c["xqb"], T, fast=True), Z.floor_q(c["xqb"], T))
    assert np.array_equal(Z.conv_sk(c["xb"], T, fast=True), Z.conv_sk(c["xb"], T))
    m = Z.case(O, "mixed")
    assert np.array_equal(Z.conv_sk(m["xb"], m["T"], fast=True), Z.conv_sk(m["xb"], m["T"]))
    assert np.array_equal(Z.q_to_bsk(m["xq"], m["T"], fast=True), Z.q_to_bsk(m["xq"], m["T"]))


def test_encrypt_multiply_decrypt(O):
    """encrypt -> eval_mult_behz -> decrypt3 gives the product plaintext (t = 65537)"""
    log_n, sq = 4, 2
    n = 1 << log_n
    q, rq = O.moduli_chain(log_n, sq)
    b, msk, _ = Z.behz_bases(O, log_n, q, Z.T_PLAIN)
    T = BT.BehzTables(q, b, msk, Z.T_PLAIN)
    ring = Z.Ring(O, log_n, T, rq)
    rng = np.random.default_rng(9)
    s = np.array([int(v) for v in rng.integers(-1, 2, size=n)], dtype=object)
    ms = [np.array([int(v) for v in rng.integers(0, Z.T_PLAIN, size=n)], dtype=object) for _ in range(2)]
    cts = list(BR.encrypt(O, rng, ms[0], s, q, ring.tb_q, Z.T_PLAIN)) + \
        list(BR.encrypt(O, rng, ms[1], s, q, ring.tb_q, Z.T_PLAIN))
    outs = Z.eval_mult_behz(O, T, ring, *cts)
    assert (BR.decrypt3(outs, s, q, Z.T_PLAIN) == BR.negacyclic(ms[0], ms[1]) % Z.T_PLAIN).all()


@pytest.mark.parametrize("name", [c[0] for c in Z.CASES])
def test_gpu_cases_cover_every_branch(O, name):
    """On the inputs the GPU parity tests use: the q -> Bsk case holds r = 0, 0x7fff, 0x8000 and 0xffff
    (planted) and both sides of r >= 0x8000 among the others; the SK case holds alpha = 0, msk / 2,
    msk / 2 + 1 and msk - 1 (planted) and both signs among the others; the mixed chain has a tower
    below msk / 2 on which the centred correction differs from the wrapping one."""
    c = Z.case(O, name)
    T, n = c["T"], c["n"]
    _, r = Z.q_to_bsk(c["xq"], T, want_r=True, fast=c["fast"])
    r = r.reshape(-1)
    assert list(r[:4]) == Z.R_TARGETS
    assert (r[4:] >= 0x8000).any() and (r[4:] < 0x8000).any()
    out, a = Z.conv_sk(c["xb"], T, want_alpha=True, fast=c["fast"])
    a = a.reshape(-1)
    assert [int(v) for v in a[:4]] == Z.alpha_targets(T.msk)
    rest = np.array([int(v) > T.msk // 2 for v in a[4:]])
    assert rest.any() and not rest.all()
    assert (c["xq"] < np.array(T.q, dtype=np.uint64)[None, :, None]).all()
    assert (c["xb"] < np.array(T.bsk, dtype=np.uint64)[None, :, None]).all()
    assert c["xq"].shape == (Z.BATCH, len(T.q), n) and c["xqb"].shape == (Z.BATCH, len(T.q) + len(T.bsk), n)
    if name == "mixed":
        assert min(T.q) < T.msk // 2 and T.q[-1] == max(T.q)
        assert not np.array_equal(Z.conv_sk(c["xb"], T, wrapping=True), out)
    if name == "uneven":
        assert len(T.b) != len(T.q)
