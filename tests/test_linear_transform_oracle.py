"""CPU checks of the BSGS linear transform's reference composition
(tests/linear_transform_ref.py), the yardstick of tests/test_gpu_linear_transform.py.

1. The stage definitions against exact integers.
2. Semantics with real keys: the composition decrypts to the linear transform.
3. The EvalLinearTransform mapping reproduces the reference's loop bounds.
4. The place of ModDown (before the automorphism) is observable in the output words.
"""
import math
from fractions import Fraction

import numpy as np
import pytest

import keyswitch as K
import linear_transform_ref as LT
import oracle as O
import rotation_ref as R
from test_keyswitch_oracle import _bases, _uniform
from test_rotation_oracle import coeff_automorphism_signed


def test_ext_ref_is_c_times_p_mod_q():
    log_n, sq, sp = 3, 4, 2
    n = 1 << log_n
    q, rq, p, rp = _bases(log_n, sq, sp)
    kp = K.KeySwitchParams(n, q, rq, p, rp, 2)
    rng = np.random.default_rng(1)
    Pint = math.prod(p)
    for l in (sq, 2):
        c = _uniform(rng, 2, q[:l], n)
        c[0, 0, 0], c[0, 0, 1] = 0, q[0] - 1
        got = LT.ext_ref(kp, c)
        assert got.shape == (2, l + sp, n)
        for b in range(2):
            for t in range(l):
                assert [int(v) for v in got[b, t]] == [int(v) * Pint % q[t] for v in c[b, t]]
        assert not got[:, l:].any()


def test_mult_ext_sum_ref_against_integers():
    log_n, sq, sp, l = 3, 4, 2, 3
    n = 1 << log_n
    q, rq, p, rp = _bases(log_n, sq, sp)
    kp = K.KeySwitchParams(n, q, rq, p, rp, 2)
    mods = q[:l] + p
    rng = np.random.default_rng(2)
    nterm, nsum, B = 3, 2, 2
    x0 = np.stack([_uniform(rng, B, mods, n) for _ in range(nterm)])
    x1 = np.stack([_uniform(rng, B, mods, n) for _ in range(nterm)])
    diag = _uniform(rng, nsum * nterm, mods, n)
    x0[0, 0, 0, :2] = mods[0] - 1
    diag[0, 0, :2] = mods[0] - 1   # the largest product
    present = [1, 0, 1, 1, 1, 1]
    for pres in (None, present):
        o = LT.mult_ext_sum_ref(kp, l, x0, x1, diag, pres, nsum)
        for e, x in enumerate((x0, x1)):
            for j in range(nsum):
                for b in range(B):
                    for t, m in enumerate(mods):
                        want = [sum(int(x[i, b, t, c]) * int(diag[j * nterm + i, t, c]) for i in range(nterm)
                                    if pres is None or pres[j * nterm + i]) % m for c in range(n)]
                        assert [int(v) for v in o[e][j, b, t]] == want


def _real_key_case(seed=11):
    """N = 2^6, 5 + 3 towers, dnum 2; nbaby = ngiant = 3 with an identity at position 0 of both lists and
    the last diagonal absent; real rotation keys; one ternary polynomial per diagonal, taken mod
    every Ql|P tower."""
    log_n, sq, sp, dnum = 6, 5, 3, 2
    n = 1 << log_n
    q, rq, p, rp = _bases(log_n, sq, sp)
    kp = K.KeySwitchParams(n, q, rq, p, rp, dnum)
    rng = np.random.default_rng(seed)
    s = K.ternary(n, rng)
    c0 = K.set_format(_uniform(rng, 1, q, n), q, rq, True)
    c1 = K.set_format(_uniform(rng, 1, q, n), q, rq, True)
    baby, giant = [1, 5, 25], [1, pow(5, 3, 2 * n), pow(5, 6, 2 * n)]

    def key(k):
        if k == 1:
            return None
        return K.keyswitch_gen(kp, s, coeff_automorphism_signed(s, R.inverse_index(k, n)), rng)

    bkeys, gkeys = [key(k) for k in baby], [key(k) for k in giant]
    diag = np.concatenate([K.small_poly_eval(K.ternary(n, rng), q + p, rq + rp) for _ in range(9)])
    present = [1] * 8 + [0]
    return dict(log_n=log_n, sq=sq, sp=sp, dnum=dnum, n=n, q=q, rq=rq, p=p, rp=rp, kp=kp, s=s, c0=c0, c1=c1,
                baby=baby, giant=giant, bkeys=bkeys, gkeys=gkeys, diag=diag, present=present)


def residual_bound(kp, l, n, nbaby, ngiant, diag_norm=1, key_err=3):
    """Bound on the centred residual of the BSGS transform's decryption (see
    test_reference_composition_decrypts_to_the_linear_transform)."""
    sp = len(kp.p)
    beta, alpha = kp.beta(l), kp.alpha
    qd = max(math.prod(kp.q[kp.digit(l, j)[0]:sum(kp.digit(l, j))]) for j in range(beta))
    e_ks = Fraction(key_err * beta * alpha * n * qd, math.prod(kp.p))   # one key switch's noise / P
    md = sp * (1 + n)                                                    # one ciphertext ModDown's rounding
    return math.ceil(ngiant * (nbaby * n * diag_norm * e_ks + md) + ngiant * e_ks + md)


def check_decrypts(case, out0, out1):
    """out0 + out1 s - sum_j sigma_gj(sum_i d_ji sigma_bi(c0 + c1 s)), centred, against the bound."""
    q, rq, n, sq = case["q"], case["rq"], case["n"], case["sq"]
    s_eval = K.small_poly_eval(case["s"], q, rq)
    msg = O.eltwise("add", case["c0"], O.eltwise("mul", case["c1"], s_eval, q), q)
    nb = len(case["baby"])
    want = np.zeros_like(msg)
    for j, g in enumerate(case["giant"]):
        inner = np.zeros_like(msg)
        for i, b in enumerate(case["baby"]):
            if case["present"][j * nb + i]:
                d = np.ascontiguousarray(case["diag"][j * nb + i][None, :sq])
                inner = O.eltwise("add", inner, O.eltwise("mul", d, R.sigma(msg, b), q), q)
        want = O.eltwise("add", want, R.sigma(inner, g), q)
    lhs = O.eltwise("add", out0, O.eltwise("mul", out1, s_eval, q), q)
    d = K.set_format(O.eltwise("sub", lhs, want, q), q, rq, False)
    err = max(abs(e) for e in K.crt_centered(d[0], q))
    bound = residual_bound(case["kp"], sq, n, nb, len(case["giant"]))
    print(f"residual {err.bit_length()} bits, bound {bound.bit_length()} bits, Q_l {math.prod(q).bit_length()} bits")
    assert bound << 60 < math.prod(q)   # a wrong term, uniform mod Q_l, cannot pass
    assert err <= bound, (err, bound)
    # the transform's value itself is Q-sized: the bound is not met trivially
    assert max(abs(e) for e in K.crt_centered(K.set_format(want, q, rq, False)[0], q)) > bound << 60


def test_reference_composition_decrypts_to_the_linear_transform():
    """With keys KeySwitchGen(s, sigma_{k^-1}(s)) (error coefficients |e| <= 3) and ternary
    diagonals (norm 1), out0 + out1 s = sum_j sigma_gj(sum_i d_ji sigma_bi(c0 + c1 s)) + residual.

    Bound on the residual.  A key switch leaves, at scale P, the noise sum_d digit_d e_d with digit_d
    in [0, alpha Q_d) (ApproxSwitchCRTBasis without its correction) and beta digits, so
    |E| <= 3 beta alpha N Q_d; after the division by P this is e_ks = 3 beta alpha N max(Q_d) / P.
    KeySwitchExt is exact.  A product by a diagonal multiplies a norm by at most N ||d|| = N.  One
    ApproxModDown of a ciphertext subtracts (x~0 + x~1 s) / P with x~ in [0, sp P): at most
    md = sp (1 + N).  Automorphisms keep norms.  Hence per giant step nbaby N e_ks + md, for the
    giant key switches ngiant e_ks, and md for the last ModDown:
        residual <= ngiant (nbaby N e_ks + md) + ngiant e_ks + md
    which is about 2^20 here against Q_l of about 2^300."""
    case = _real_key_case()
    out0, out1 = LT.bsgs_ref(case["kp"], case["c0"], case["c1"], case["baby"], case["giant"], case["bkeys"],
                             case["gkeys"], case["diag"], case["present"])
    check_decrypts(case, out0, out1)


def test_a_wrong_term_fails_the_semantic_check():
    case = _real_key_case()
    present = list(case["present"])
    present[4] = 0  # one diagonal dropped from the computation only
    out0, out1 = LT.bsgs_ref(case["kp"], case["c0"], case["c1"], case["baby"], case["giant"], case["bkeys"],
                             case["gkeys"], case["diag"], present)
    with pytest.raises(AssertionError):
        check_decrypts(case, out0, out1)


@pytest.mark.parametrize("slots", [5, 8, 9])
def test_eval_linear_transform_mapping(slots):
    """The plan's indices and presence against the reference's loops restated (ckksrns-fhe.cpp:1499-1547)."""
    n = 32
    M = 2 * n
    b, g, baby, giant, present = LT.linear_transform_plan(slots, n)
    bstep = math.ceil(math.sqrt(slots))
    gstep = math.ceil(slots / bstep)
    assert (b, g) == (bstep, gstep) and len(baby) == bstep and len(giant) == gstep
    assert baby[0] == 1 and giant[0] == 1
    used = set()
    for j in range(gstep):
        used.add((j, 0))                        # EvalMultExt(KeySwitchExt(ct), A[bStep * j]), 1521
        assert bstep * j < slots                # ... which the reference reads unconditionally
        for i in range(1, bstep):
            if bstep * j + i < slots:           # 1523
                used.add((j, i))
    assert {(j, i) for j in range(g) for i in range(b) if present[j * b + i]} == used
    assert len(used) == slots
    for i in range(1, bstep):                   # EvalFastRotationExt(ct, i, ...), 1514
        assert baby[i] == pow(5, i, M) and not LT.is_identity(baby[i], n)
    for j in range(1, gstep):                   # FindAutomorphismIndex2nComplex(bStep * j, M), 1538
        assert giant[j] == pow(5, bstep * j, M)


def test_moddown_before_the_automorphism_is_observable():
    """Planted case: N = 8, 4 + 2 towers, dnum 2, uniform inputs and keys (seed 5), babies (1, 5),
    giants (1, 25), all diagonals present.  Taking giant step 1's ModDown after its automorphism
    instead of before changes output words: ApproxModDown works on coefficients and the
    evaluation-form permutation is not one of them, so bit parity with the composition pins the order."""
    log_n, sq, sp, dnum = 3, 4, 2, 2
    n = 1 << log_n
    q, rq, p, rp = _bases(log_n, sq, sp)
    kp = K.KeySwitchParams(n, q, rq, p, rp, dnum)
    rng = np.random.default_rng(5)
    c0, c1 = _uniform(rng, 1, q, n), _uniform(rng, 1, q, n)
    baby, giant = [1, 5], [1, 25 % (2 * n)]
    keys = lambda: (_uniform(rng, dnum, q + p, n), _uniform(rng, dnum, q + p, n))  # noqa: E731
    bkeys, gkeys = [None, keys()], [None, keys()]
    diag = _uniform(rng, 4, q + p, n)
    a = LT.bsgs_ref(kp, c0, c1, baby, giant, bkeys, gkeys, diag)
    b = LT.bsgs_ref(kp, c0, c1, baby, giant, bkeys, gkeys, diag, moddown_after_automorphism=(1,))
    assert np.array_equal(a[1], b[1])          # only the first element takes that path
    assert np.count_nonzero(a[0] != b[0]) > 0
