"""CPU tests of the restatement the BGV decryption parity tests compare against (tests/bgv_decrypt_ref.py):
the chain against exact integers, real encryptions through both of the reference's branches, the difference
between the branches, NativeVectorT::Mod(t) on its boundaries, and the scaling-factor helper of the binding
against its definition."""
import numpy as np
import pytest

import bgv_decrypt_ref as G
import oracle as O

T_VALUES = [2, 65537, 1 << 20, G.mixed_chain(1)[0] + 2]  # the last is above q_0


def crt(x, q):
    """[L][n] residues -> list of integers in [0, Q)"""
    Q = 1
    for m in q:
        Q *= int(m)
    out = []
    for c in range(x.shape[1]):
        v = 0
        for i, m in enumerate(q):
            Mi = Q // int(m)
            v += int(x[i, c]) * Mi * pow(Mi % int(m), -1, int(m))
        out.append(v % Q)
    return out


@pytest.mark.parametrize("t", T_VALUES)
def test_chain_agrees_with_exact_integers(t):
    """after step j the lifted value X + t [delta], [delta] the centred x_j negtInvModq[j] mod q_j, is
    divisible by q_j and = X mod t, and the towers left hold (X + t [delta]) / q_j"""
    q, n, batch = G.mixed_chain(5), 8, 2
    assert any(q[i] > q[j] for j in range(5) for i in range(j)) and any(q[i] < q[j] for j in range(5) for i in range(j))
    x = G.planted(batch, q, n, 7)
    steps = []
    out = G.chain(x, q, t, False, steps)
    assert [j for j, _, _ in steps] == [4, 3, 2, 1]
    nti = G.neg_t_inv_modq(q, t)
    for j, before, after in steps:
        qj = int(q[j])
        for b in range(batch):
            X = crt(before[b], q[:j + 1])
            for c in range(n):
                d = int(before[b, j, c]) * nti[j] % qj
                d = d - qj if d > qj >> 1 else d
                Y = X[c] + t * d
                assert Y % qj == 0 and (Y - X[c]) % t == 0
                assert [int(after[b, i, c]) for i in range(j)] == [Y // qj % int(q[i]) for i in range(j)]
    assert np.array_equal(out, steps[-1][2][:, 0])
    assert np.array_equal(G.chain(x, q, t, True), G.mod_t(out, q[0], t))
    # one tower: the loop is skipped
    assert np.array_equal(G.chain(x[:, :1], q, t, False), x[:, 0])


@pytest.mark.parametrize("elements", [2, 3])
@pytest.mark.parametrize("size_ql", [1, 2, 3, 4])
def test_real_encryptions_decrypt_in_both_branches(size_ql, elements):
    """N = 16, t = 65537, a chain of 40-, 50-, 30- and 45-bit NTT primes, a ternary secret, v = m + t e with
    0 <= m < t and |e| <= E, the extremes +-E planted.  Every ModReduce step multiplies the plaintext by
    q_j^-1 mod t, so both branches return m (q_1 .. q_l)^-1 mod t (the reference tracks that in
    scalingFactorInt).

    The bound E, derived, not tuned.  Write L = size_ql, P = q_1 .. q_{L-1}.  A step maps an integer X to
    (X + t [delta]) / q_j with |[delta]| < q_j / 2, so after the chain X_0 = X / P + t eta with
    |eta| < c_L = sum_{j=1}^{L-1} 1 / (2 q_1 .. q_{j-1}).
      evaluation-form branch: the chain runs on b = v (its own centred lift as |v| < Q_L / 2), and the word
        left is v / P + t eta, read centred mod q_0: right when |v| / P + t c_L < q_0 / 2;
      coefficient-form branch: the chain runs on each c_k (uniform mod Q_L), c_k' = c_k / P + t eta_k, and
        DecryptCore on tower 0 forms sum c_k' s^k = v / P + t sum eta_k s^k (mod q_0).  With s ternary,
        |eta_k s^k| <= N^k |eta_k|, so the word is right when |v| / P + t c_L (1 + N + N^2) < q_0 / 2, and
        P times it is v + t (an integer polynomial), i.e. it is v P^-1 mod t.
    The second condition implies the first (and |v| < Q_L / 2); with |v| < t (E + 1) it holds for
    E = floor((q_0 / 2 - t c_L (1 + N + N^2)) P / t) - 1, which is G.noise_bound."""
    log_n, t = 4, 65537
    n = 1 << log_n
    q = [O.first_prime(b, 2 * n) for b in (40, 50, 30, 45)]
    rq = [O.root_of_unity(2 * n, m) for m in q]
    ql, rql = q[:size_ql], rq[:size_ql]
    E = G.noise_bound(n, t, ql)
    assert E >= 1
    rng = np.random.default_rng(100 * size_ql + elements)
    s = np.array([int(v) for v in rng.integers(-1, 2, size=n)], dtype=object)
    m = np.array([int(v) for v in rng.integers(0, t, size=n)], dtype=object)
    m[0], m[1] = t - 1, 0
    e = G.uniform_mod(rng, n, 2 * E + 1) - E
    e[0], e[1] = E, -E
    elems = G.encrypt(rng, m + t * e, s, ql, rql, elements)
    s_eval = np.stack([(s % int(x)).astype(np.uint64) for x in q])[None]
    s_eval = G.K.set_format(s_eval, q, rq, True)[0]
    scale = 1
    for x in ql[1:]:
        scale = scale * pow(int(x), -1, t) % t
    want = (m * scale % t).astype(np.uint64)
    got_eval = G.decrypt(elems, s_eval, q, rq, t, True)
    coef = [G.K.set_format(c, ql, rql, False) for c in elems]
    got_coef = G.decrypt(coef, s_eval, q, rq, t, False)
    assert np.array_equal(got_eval[0], want) and np.array_equal(got_coef[0], want)


def test_the_two_branches_differ_before_mod_t():
    """on a real encryption over 3 towers the two branches reach the same plaintext through different tower-0
    words, so a parity test against one restatement does not pass with the other branch's arithmetic"""
    log_n, t = 4, 65537
    n = 1 << log_n
    q = [O.first_prime(b, 2 * n) for b in (40, 50, 30)]
    rq = [O.root_of_unity(2 * n, m) for m in q]
    rng = np.random.default_rng(5)
    s = np.array([int(v) for v in rng.integers(-1, 2, size=n)], dtype=object)
    m = np.array([int(v) for v in rng.integers(0, t, size=n)], dtype=object)
    elems = G.encrypt(rng, m + t * np.array([int(v) for v in rng.integers(-3, 4, size=n)], dtype=object), s, q, rq, 3)
    s_eval = G.K.set_format(np.stack([(s % int(x)).astype(np.uint64) for x in q])[None], q, rq, True)[0]
    w_eval, w_coef = [], []
    a = G.decrypt(elems, s_eval, q, rq, t, True, w_eval)
    b = G.decrypt([G.K.set_format(c, q, rq, False) for c in elems], s_eval, q, rq, t, False, w_coef)
    assert np.array_equal(a, b)
    assert (w_eval[0] != w_coef[0]).sum() > n // 2


def test_mod_t_cases_on_the_boundaries():
    """t == 2, t > q_0 and t <= q_0 at 0, q_0 >> 1, (q_0 >> 1) + 1, q_0 - 1, against the centred residue"""
    for q0 in (1073741827, 4194319, (1 << 59) + 55):
        x = np.array([0, q0 >> 1, (q0 >> 1) + 1, q0 - 1, 1, 2], dtype=np.uint64)
        for t in (2, 3, 65537, 1 << 20, q0 - 2, q0 + 2, (1 << 60) + 1):
            got = G.mod_t(x, q0, t)
            for v, g in zip(x, got):
                v = int(v)
                c = v - q0 if v > q0 >> 1 else v
                if t == 2:
                    # ModByTwoEq: the parity of the centred value (q_0 odd: v - q_0 flips the parity of v)
                    assert int(g) == (c % 2)
                elif t > q0:
                    assert int(g) == (v + t - q0 if v > q0 >> 1 else v) and int(g) % t == c % t
                else:
                    assert int(g) == c % t
    # the three cases written out on one word each
    assert G.mod_t([6], 11, 2)[0] == 1 and G.mod_t([5], 11, 2)[0] == 1 and G.mod_t([10], 11, 2)[0] == 1
    assert G.mod_t([6], 11, 13)[0] == 8 and G.mod_t([5], 11, 13)[0] == 5
    assert G.mod_t([6], 11, 3)[0] == (6 - 11) % 3 and G.mod_t([5], 11, 3)[0] == 2


def test_scaling_factor_helper_against_its_definition():
    import ofhe_hip as H

    t = 65537
    rng = np.random.default_rng(3)
    factors = [int(v) for v in rng.integers(1, t, size=6)]
    for size_ql in range(1, 7):
        for sf in (1, 12345, t - 1):
            want = sf
            for i in range(size_ql - 1):
                inv = next(k for k in range(1, t) if k * factors[size_ql - 1 - i] % t == 1) if size_ql <= 2 else \
                    pow(factors[size_ql - 1 - i], t - 2, t)
                want = want * inv % t
            assert H.bgv_scaling_factor(sf, factors, size_ql, t) == want == G.scaling_factor(sf, factors, size_ql, t)
    assert H.bgv_scaling_factor(7, [], 1, t) == 7  # one tower: nothing to undo
    with pytest.raises(H.MathError, match="not invertible"):
        H.bgv_scaling_factor(1, [1, 6], 2, 9)
    with pytest.raises(H.MathError, match="one factor per level"):
        H.bgv_scaling_factor(1, [1, 5], 3, 7)
