"""CPU: the oracle on modulus chains of mixed size and form.

tests/test_gpu_mixed_moduli.py, test_gpu_fuzz_tier2.py and
test_gpu_caller_stream.py use oracle/keyswitch.py as the reference for chains
whose towers differ by up to 30 bits, where NativeVectorT::SwitchModulus
(mubintvecnat.cpp:111-136) takes every one of its branches.  The oracle's
other CPU tests only see O.moduli_chain (strictly decreasing primes just below
2^60), so the identities of test_rescale_oracle.py, test_bv_oracle.py and
test_keyswitch_oracle.py are repeated here on such chains, against exact
integers:
  * SwitchModulus is "the centred value modulo the new modulus" whether the new
    modulus is larger, smaller by less than a factor of two, smaller by more,
    or equal;
  * DropLastElementAndScale is rounding division by q_l, ModReduce exact
    division, and both give the same result from either input form;
  * the BV identity ct0 + ct1 s_new = c s_old - sum_i d_i e_i holds exactly;
  * a HYBRID key switch with 40-60-bit Q towers decrypts with a small error.
Ring sizes stay at N <= 2^10: the big-integer CRT lifts are slow in Python.
"""
import numpy as np
import pytest

import keyswitch as K
import oracle as O


def mixed_chain(log_n, bits, generic=False):
    """Distinct primes = 1 mod 2N, one per entry of `bits`, with their minimal
    roots of unity: (moduli, roots).  An integer entry b asks for a b-bit prime:
    of the form 2^b - d (the first primes below 2^b, O.previous_prime), or with
    generic = True one found by O.next_prime from 1.375 * 2^(b-1), whose top
    word is far from all-ones.  Entries of equal size get strictly decreasing
    primes in the order they are listed.  ("next", x) / ("prev", x) ask for the
    nearest such prime above / below the integer x, whatever its form."""
    m = 2 << log_n
    qs = [None] * len(bits)
    for b in sorted({e for e in bits if isinstance(e, int)}, reverse=True):
        idx = [i for i, e in enumerate(bits) if e == b and isinstance(e, int)]
        found = []
        if generic:
            start = 11 << (b - 4)
            q = start - start % m + 1
            for _ in idx:
                q = O.next_prime(q, m)
                found.append(q)
            found.reverse()
        else:
            q = ((1 << b) // m) * m + 1
            for _ in idx:
                q = O.previous_prime(q, m)
                found.append(q)
        for i, q in zip(idx, found):
            assert q.bit_length() == b, f"no {b}-bit prime = 1 mod {m} from this start"
            qs[i] = q
    for i, e in enumerate(bits):
        if not isinstance(e, int):
            kind, x = e
            base = x - x % m + 1
            if kind == "next":  # O.next_prime / O.previous_prime start one step away from their argument
                q = O.next_prime(base if base <= x else base - m, m)
                while q in qs:
                    q = O.next_prime(q, m)
            else:
                q = O.previous_prime(base + m if base < x else base, m)
                while q in qs:
                    q = O.previous_prime(q, m)
            qs[i] = q
    assert len(set(qs)) == len(qs) and all(3 <= q < (1 << 60) and q % m == 1 for q in qs)
    return qs, [O.root_of_unity(m, q) for q in qs]


# One chain, all regimes: the last tower L (about 50 bits) is switched into a
# 60-bit tower (up, large difference), a prime just above it (up, small
# difference), a prime just below it (down, two conditional subtractions) and a
# small tower (down by more than a factor of two: the general remainder).
def rescale_chain(log_n, generic=False, small_bits=30):
    q, r = mixed_chain(log_n, [60, 50, 50, 50, small_bits], generic)
    order = [0, 1, 4, 3, 2]  # 60-bit, just above L, small, just below L, L
    return [q[i] for i in order], [r[i] for i in order]


# Four towers whose digit -> tower pairs take every branch.  Special form: a
# 60-bit tower, two consecutive primes below 2^59 (down by less than a factor of
# two one way, up the other; the 60-bit tower against them sits within a few
# 2N of the factor-of-two boundary) and a small tower.  Generic form: the second
# tower is the first prime above half of the first (the old modulus just below
# twice the new one), then a 59-bit and a small tower.
def bv_chain(log_n, generic=False, small_bits=30, extra=()):
    if not generic:
        return mixed_chain(log_n, [60, 59, 59, small_bits, *extra])
    (q0,), _ = mixed_chain(log_n, [60], True)
    return mixed_chain(log_n, [60, ("next", q0 // 2), 59, small_bits, *extra], True)


def is_special_prime(q):
    """The plan's test for the special-prime kernels (ofhe_hip_plan_create_ex):
    q = 2^L - d with L >= 33, d < 2^32 (the top word all ones, the low word not
    zero) and 16 d < q.  A plan takes those kernels only if every tower passes."""
    L = q.bit_length()
    d = (1 << L) - q
    return L >= 33 and (q >> 32) == (1 << (L - 32)) - 1 and (q & 0xFFFFFFFF) != 0 and 16 * d < q


def regime(om, nm):
    """Which branch SwitchModulus(om -> nm) takes."""
    if nm > om:
        return "up"
    if nm == om:
        return "equal"
    return "down_small" if om <= 2 * nm else "down_big"


def boundary_words(q):
    return [0, 1, q // 2, q // 2 + 1, q - 1]


def with_boundaries(rng, rows, q, n):
    """[rows][n] uniform residues mod q, every other word one of q's boundary words."""
    x = rng.integers(0, q, size=(rows, n), dtype=np.uint64)
    w = np.array(boundary_words(q), np.uint64)
    x[:, ::2] = w[rng.integers(0, len(w), size=(rows, (n + 1) // 2))]
    return x


def uniform(rng, batch, moduli, n):
    return np.stack([np.stack([rng.integers(0, m, size=n, dtype=np.uint64) for m in moduli]) for _ in range(batch)])


def rescale_input(rng, batch, q, n):
    """Coefficient-form [batch][T][n] with boundary words in the last tower."""
    x = uniform(rng, batch, q, n)
    x[:, -1] = with_boundaries(rng, batch, q[-1], n)
    return x


def _switch_pairs():
    (q60, q30, q50), _ = mixed_chain(10, [60, 30, 50])
    (g60, g45), _ = mixed_chain(10, [60, 45], generic=True)
    (above, below, hi, lo), _ = mixed_chain(10, [("next", 1 << 59), ("prev", 1 << 59), ("next", q60 // 2),
                                                 ("prev", q60 // 2)])
    assert above > (1 << 59) > below and hi > q60 // 2 > lo
    return [(q30, q60), (q50, g60), (g45, q50),                      # up
            (above, below), (q60, hi), (q60, g60),                    # down by less than a factor of two
            (q60, lo), (q60, q30), (g60, g45), (q50, q30),            # down by more than a factor of two
            (q60, q60), (q30, q30)]                                   # equal


SWITCH_PAIRS = _switch_pairs()


def test_switch_pairs_cover_every_regime():
    got = [regime(om, nm) for om, nm in SWITCH_PAIRS]
    for name in ("up", "down_small", "down_big", "equal"):
        assert got.count(name) >= 2, name
    om, nm = SWITCH_PAIRS[3]
    assert nm < om < 2 * nm and om - nm < om >> 20  # 2^59 + eps against 2^59 - eps


@pytest.mark.parametrize("om,nm", SWITCH_PAIRS)
def test_switch_modulus_is_centred_value(om, nm):
    rng = np.random.default_rng(om % 9973 + nm % 97)
    v = rng.integers(0, om, size=512, dtype=np.uint64)
    edge = boundary_words(om) + [om // 2 - 1, om - 2, min(nm, om) - 1, nm % om, (om - nm) % om]
    v[:len(edge)] = edge
    got = K.switch_modulus(v, om, nm)
    want = [((int(x) if int(x) <= om // 2 else int(x) - om) % nm) for x in v]
    assert got.dtype == np.uint64 and [int(x) for x in got] == want


def test_rescale_chain_covers_every_regime():
    for generic in (False, True):
        for log_n in (5, 10, 17):
            q, _ = rescale_chain(log_n, generic)
            assert [regime(q[-1], qi) for qi in q[:-1]] == ["up", "up", "down_big", "down_small"]
            assert q[0].bit_length() == 60 and q[2].bit_length() <= 30 and q[-1].bit_length() == 50
            assert q[1] - q[-1] < q[-1] >> 12 and q[-1] - q[3] < q[-1] >> 12
            # one level lower the last tower is the prime just below L: up, up, down_big
            assert [regime(q[3], qi) for qi in q[:3]] == ["up", "up", "down_big"]
            for small_bits in (30, 34):
                b, _ = bv_chain(log_n, generic, small_bits, extra=(45,))
                pairs = {regime(b[i], b[k]) for i in range(4) for k in range(4) if i != k}
                assert pairs == {"up", "down_small", "down_big"}
                if generic:
                    assert b[1] > b[0] // 2 and b[1] - b[0] // 2 < b[0] >> 12
                else:
                    assert b[2] < b[1] < 1 << 59 and b[1] - b[2] < b[1] >> 12


def test_special_chains_pass_the_plans_special_prime_test():
    """What the GPU tests call a special-form chain takes the special-prime
    kernels only if EVERY tower passes the plan's test; a tower below 33 bits
    never does, and the generic chains have no tower that does."""
    assert is_special_prime((1 << 60) - 93) and is_special_prime((1 << 33) - 9)
    assert not is_special_prime((1 << 32) - 5) and not is_special_prime((1 << 59) + 1)
    assert not is_special_prime(11 << 56) and not is_special_prime((1 << 60) - (1 << 32) - 1)
    for log_n in (4, 5, 12, 13, 15, 16, 17):
        for chain in (rescale_chain(log_n, False, 34)[0], bv_chain(log_n, False, 34, extra=(45,))[0]):
            assert all(is_special_prime(q) for q in chain), (log_n, chain)
        for chain in (rescale_chain(log_n, False, 30)[0], bv_chain(log_n, False, 30, extra=(45,))[0]):
            assert [is_special_prime(q) for q in chain].count(False) == 1  # the 30-bit tower alone
        for chain in (rescale_chain(log_n, True, 30)[0], bv_chain(log_n, True, 30, extra=(45,))[0]):
            assert not any(is_special_prime(q) for q in chain), (log_n, chain)


@pytest.mark.parametrize("log_n", [6, 10])
@pytest.mark.parametrize("generic", [False, True])
def test_rescale_is_rounding_division_mixed(log_n, generic):
    n = 1 << log_n
    q, r = rescale_chain(log_n, generic)
    x = rescale_input(np.random.default_rng(11 + log_n), 2, q, n)
    c, a = K.rescale_tables(q)
    out = K.drop_last_and_scale(x, q, r, False, c, a)
    y = K.set_format(out, q[:-1], r[:-1], False)
    ql = q[-1]
    for b in range(x.shape[0]):
        X, Y = K.crt_centered(x[b], q), K.crt_centered(y[b], q[:-1])
        assert all(2 * abs(Y[i] * ql - X[i]) <= ql for i in range(n))
    xe = K.set_format(x, q, r, True)
    assert np.array_equal(K.drop_last_and_scale(xe, q, r, True, c, a), out)


@pytest.mark.parametrize("t", [2, 65537])
@pytest.mark.parametrize("generic", [False, True])
def test_mod_reduce_is_exact_division_mixed(t, generic):
    log_n = 9
    n = 1 << log_n
    q, r = rescale_chain(log_n, generic)
    x = rescale_input(np.random.default_rng(7 + t), 2, q, n)
    ql = q[-1]
    _, a = K.rescale_tables(q)
    negtinv = (-pow(t, -1, ql)) % ql
    out = K.mod_reduce(x, q, r, False, t, negtinv, a)
    for b in range(x.shape[0]):
        X, Y = K.crt_centered(x[b], q), K.crt_centered(out[b], q[:-1])
        assert all((Y[i] * ql - X[i]) % t == 0 and 2 * abs(Y[i] * ql - X[i]) <= t * ql for i in range(n))
    xe = K.set_format(x, q, r, True)
    oe = K.mod_reduce(xe, q, r, True, t, negtinv, a)
    assert np.array_equal(K.set_format(oe, q[:-1], r[:-1], False), out)


@pytest.mark.parametrize("log_n", [6, 10])
@pytest.mark.parametrize("generic", [False, True])
def test_bv_identity_mixed(log_n, generic):
    n = 1 << log_n
    q, rq = bv_chain(log_n, generic)
    T = len(q)
    rng = np.random.default_rng(3 + log_n)
    coef = np.stack([with_boundaries(rng, 1, qi, n)[0] for qi in q])[None]
    c = K.set_format(coef, q, rq, True)
    d = K.crt_decompose0(c, q, rq)
    for i in range(T):
        assert np.array_equal(d[0, i, i], c[0, i])
        coef_di = K.set_format(d[:, i], q, rq, False)
        for k in range(T):
            want = [((int(v) if int(v) <= q[i] // 2 else int(v) - q[i]) % q[k]) for v in coef[0, i]]
            assert [int(v) for v in coef_di[0, k]] == want, (i, k)
    s_old = K.small_poly_eval(rng.integers(-1, 2, size=n), q, rq)[0]
    s_new = K.small_poly_eval(rng.integers(-1, 2, size=n), q, rq)[0]
    kb, ka, es = K.bv_keygen(q, rq, s_old, s_new, rng)
    o0, o1 = K.bv_fast_core(d, kb, ka, q)
    lhs = O.eltwise("add", o0, O.eltwise("mul", o1, s_new[None], q), q)
    noise = O.eltwise("mul", d[:, 0], es[0:1], q)
    for i in range(1, T):
        noise = O.eltwise("add", noise, O.eltwise("mul", d[:, i], es[i:i + 1], q), q)
    rhs = O.eltwise("sub", O.eltwise("mul", c, s_old[None], q), noise, q)
    assert np.array_equal(lhs, rhs)


def centred_same_small(d, q, bound):
    """[T][N] residues: every tower holds the same integer e with |e| < bound
    (so the CRT value is e itself and no big-integer lift is needed)."""
    qa = np.array(q, np.uint64)[:, None]
    v = np.where(d > qa // np.uint64(2), d.astype(np.int64) - qa.astype(np.int64), d.astype(np.int64))
    return bool(np.all(np.abs(v) < bound) and np.all(v == v[0:1]))


@pytest.mark.parametrize("dnum", [2, 4])
@pytest.mark.parametrize("generic", [False, True])
def test_hybrid_keyswitch_mixed_sizes(dnum, generic):
    """Q towers of 60 / 45 / 50 / 40 bits, P of 58 and 60 bits (P exceeds every
    digit's modulus at both splits): ct0 + ct1 s_new - c s_old is one small
    integer in every tower."""
    log_n = 8
    n = 1 << log_n
    m, r = mixed_chain(log_n, [60, 45, 50, 40, 58, 60], generic)
    q, rq, p, rp = m[:4], r[:4], m[4:], r[4:]
    kp = K.KeySwitchParams(n, q, rq, p, rp, dnum)
    rng = np.random.default_rng(70 + dnum)
    s_old, s_new = K.ternary(n, rng), K.ternary(n, rng)
    kb, ka = K.keyswitch_gen(kp, s_old, s_new, rng)
    c = K.set_format(uniform(rng, 2, q, n), q, rq, True)
    c0, c1 = K.ks_core(kp, c, kb, ka)
    sn = np.repeat(K.small_poly_eval(s_new, q, rq), 2, 0)
    so = np.repeat(K.small_poly_eval(s_old, q, rq), 2, 0)
    lhs = O.eltwise("add", c0, O.eltwise("mul", c1, sn, q), q)
    d = K.set_format(O.eltwise("sub", lhs, O.eltwise("mul", c, so, q), q), q, rq, False)
    for b in range(2):
        assert centred_same_small(d[b], q, 1 << 20)
