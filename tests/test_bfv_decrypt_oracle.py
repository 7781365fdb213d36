"""CPU: the restatement of BFV decryption (tests/decrypt_ref.py) against the
definitions, on the very inputs tests/test_gpu_bfv_decrypt.py runs.

* every table of bfv_tables.DecryptTables against its definition, exact integers;
* the cases reach all eight loops A-H of DCRTPolyImpl::ScaleAndRound -> NativePoly
  (dcrtpoly-impl.h:1547-1803; tests/test_gpu_bfv_decrypt.py asserts that the library runs the same one);
* real encryptions decrypt to the plaintext in every loop, under BEHZ and on the
  one-tower path; on uniform towers the reference legitimately differs from
  round(t x / Q) mod t (its error bounds assume |x_i| <= q_i / 2), so those are
  compared with the restatement only and the difference is just reported;
* on every input the final cast of the loops E-H is of a non-negative double
  (decrypt_ref.scale_round asserts it);
* sensitivity: a fused multiply-add chain gives another output than the
  separately rounded one on planted coefficients (see test_fused_chain_differs).

These are the cases the feature shipped with: towers of one size, small
plaintext moduli, t < q / 2 on one tower.  The sweep beyond them (mixed chains,
t up to 2^62, outputs equal to t, q <= 2 t and t > q, any 64-bit word into
TimesQovert, every plan option of the decrypt call) is tests/decrypt_cases.py,
with its coverage conditions in tests/test_decrypt_cases.py and its GPU parity
in tests/test_gpu_fuzz_decrypt.py.
"""
from fractions import Fraction

import numpy as np
import pytest

import bfv_ref as BR
import bfv_tables as BT
import decrypt_ref as D
import oracle as O

HPS_IDS = [D.case_id(c) for c in D.HPS_CASES]

# Cases that must hold planted coefficients which tell a fused chain from the reference's, whatever
# the seeds and moduli: the ones in which a search over 1320 planted candidates found such
# coefficients before these tests were written.  Every other case that holds any (with these moduli B
# with 2 towers and the 17- and 33-tower F, H and C cases, the ones that reach the kernel's second and
# later tower tiles) must carry one into its input too: test_fused_chain_differs asserts that from
# the search itself.  Only a case in which the bounded search finds none reports and does not assert:
# A with 2 towers, E, G (12 towers too) and H at t = 3221225473 with 60-bit towers.  In E and G the
# exact integer sum (up to 2^52) is added to floatSum before the quotient is taken and swamps the
# chain's low bits.
SENSITIVE = {(b, t, bits, towers) for b, t, bits, towers in
             [("A", 1 << 15, 30, 5), ("B", 1 << 31, 35, 5), ("C", 1 << 15, 60, 2), ("C", 1 << 15, 60, 5),
              ("D", 1 << 31, 60, 2), ("D", 1 << 31, 60, 5), ("F", 5308417, 30, 2), ("F", 5308417, 30, 5),
              ("F", 65537, 45, 2), ("F", 65537, 45, 5), ("H", 5308417, 55, 2), ("H", 5308417, 55, 5)]}


def test_tables_match_their_definitions():
    rng = np.random.default_rng(1)
    for _, t, bits in D.BRANCH_TABLE:
        for towers in (1, 2, 5):
            q = D.towers_below(O, 8, bits, towers)
            T = BT.DecryptTables(q, t)
            Q, hf = T.Q, q[0].bit_length() >> 1
            assert T.q_msb_hf == hf and T.tgamma == t << 26
            for i, m in enumerate(q):
                X = t * pow(Q // m % m, -1, m)
                for shift, ints, fracs in ((0, T.tQHatInvModqDivqModt, T.tQHatInvModqDivqFrac),
                                           (hf, T.tQHatInvModqBDivqModt, T.tQHatInvModqBDivqFrac)):
                    Xs = X << shift
                    assert (Xs - ints[i] * m - Xs % m) % (t * m) == 0 and 0 <= ints[i] < t
                    assert fracs[i] == float(Xs % m) / float(m)  # the reference's static_cast<double> division
                    assert abs(Fraction(fracs[i]) - Fraction(Xs % m, m)) <= Fraction(1, 1 << 52)
                assert (T.negInvqModtgamma[i] * m + 1) % T.tgamma == 0 and 0 <= T.negInvqModtgamma[i] < T.tgamma
                assert (T.tgammaQHatInvModq[i] * (Q // m) - T.tgamma) % m == 0 and 0 <= T.tgammaQHatInvModq[i] < m
                assert T.tInvModq[i] * t % m == 1
            assert (T.negQModt + Q) % t == 0 and 0 < T.negQModt <= t
            # the tables together: sum_i x_i X_i / q_i = t v / Q modulo t, exactly
            v = int(rng.integers(0, 1 << 62)) % Q
            total = sum(Fraction(v % m * (T.tQHatInvModqDivqModt[i] * m + t * pow(Q // m % m, -1, m) % m), m)
                        for i, m in enumerate(q))
            assert (total - Fraction(t * v, Q)) % t == 0


def test_cases_cover_all_eight_loops():
    seen = set()
    for c in D.HPS_CASES:
        letter, t, bits, towers, log_n, _ = c
        q = D.towers_below(O, log_n, bits, towers)
        assert all(m % (2 << log_n) == 1 and m.bit_length() == bits for m in q) and len(set(q)) == towers
        T = BT.DecryptTables(q, t)
        assert BT.BRANCHES[T.branch] == letter, c
        assert T.split == (letter in "CDGH")
        seen.add(letter)
    assert seen == set("ABCDEFGH")
    assert {c[3] for c in D.HPS_CASES} >= {2, 5, 12, 17, 33}


@pytest.mark.parametrize("c", D.HPS_CASES, ids=HPS_IDS)
def test_scale_round_restatement(c):
    """the vectorised and the scalar restatement agree; the real encryption decrypts; the final cast is
    defined on every input (scale_round asserts it); the difference from round(t x / Q) mod t on uniform
    towers is reported"""
    k = D.hps_case(O, c)
    T, x, kinds = k["T"], k["x"], k["kinds"]
    want = D.scale_round(x, T)
    assert D.defined(x, T).all()
    assert (want[0] == k["plain"].astype(np.uint64)).all(), "the real encryption does not decrypt"
    flat, wflat = x.transpose(0, 2, 1).reshape(-1, len(T.q)), want.reshape(-1)
    picks = np.concatenate([np.flatnonzero(kinds.reshape(-1) == kind)[:48] for kind in (D.REAL, D.PLANTED, D.UNIFORM)])
    for p in picks:
        assert D.scale_round_scalar([int(v) for v in flat[p]], T) == int(wflat[p]), (c, p)
    uni = np.flatnonzero(kinds.reshape(-1) == D.UNIFORM)[:64]
    lift = BR.crt_lift(x, T.q).reshape(-1)
    off = sum(D.definition(lift[p], T.Q, T.t) != int(wflat[p]) for p in uni)
    print(f"{D.case_id(c)}: {off} of {len(uni)} uniform coefficients differ from round(t x / Q) mod t, "
          f"{int((wflat == T.t).sum())} outputs equal t")
    assert (wflat <= T.t).all()


@pytest.mark.parametrize("c", D.HPS_CASES, ids=HPS_IDS)
def test_fused_chain_differs(c):
    """Sensitivity, as tests/test_bfv_oracle.py does for the exact switch: on the planted coefficients
    v = floor((2k + 1) Q / (2t)) + delta of the case's own input a fused multiply-add chain (each
    a * b + c exact, rounded once) gives another output than the separately rounded chain -- so the GPU
    parity test on this input can tell the two.  The cases of SENSITIVE (and their copies at N = 2 and
    N = 2^12) must hold such coefficients; every case whose search over the POOL candidates finds any
    must have one among its planted inputs.  The cases in which the bounded search finds none (A with 2
    towers, E, G, H at t = 3221225473 / 60 bits: see SENSITIVE's comment) report the count and do not
    assert.  Uniform input alone is not enough: it holds 0-3 sensitive coefficients in 1500."""
    k = D.hps_case(O, c)
    T, x, kinds = k["T"], k["x"], k["kinds"]
    flat = x.transpose(0, 2, 1).reshape(-1, len(T.q))
    planted = np.flatnonzero(kinds.reshape(-1) == D.PLANTED)
    hits = sum(D.fused_differs([int(v) for v in flat[p]], T) for p in planted[:256])
    print(f"{D.case_id(c)}: fused differs on {k['pool_hot']} of {k['pool']} candidates, "
          f"{hits} of the first {min(256, len(planted))} planted coefficients of the input")
    if tuple(c[:4]) in SENSITIVE:
        assert k["pool_hot"] >= 1, c
    if k["pool_hot"] >= 1:
        assert hits >= 1, c


@pytest.mark.parametrize("c", D.BEHZ_CASES, ids=[D.case_id(c) for c in D.BEHZ_CASES])
def test_behz_restatement(c):
    k = D.behz_case(O, c)
    T, x = k["T"], k["x"]
    want = D.scale_round_behz(x, T)
    # written as computed: t stands for 0 when t v / Q rounds up to t (a small negative error on m = 0)
    assert (want <= T.t).all() and (want[0] % np.uint64(T.t) == k["plain"].astype(np.uint64)).all()
    # the loop with Python integers on a few uniform coefficients
    for ri in range(8):
        s = 0
        for i, m in enumerate(T.q):
            y = int(x[1, i, ri]) * T.tgammaQHatInvModq[i] % m
            s = (s + y * T.negInvqModtgamma[i] % T.tgamma) % T.tgamma
        assert (s + (s & ((1 << 26) - 1))) >> 26 == int(want[1, ri])


@pytest.mark.parametrize("c", D.ONE_TOWER_CASES, ids=[D.case_id(c) for c in D.ONE_TOWER_CASES])
def test_one_tower_restatement(c):
    k = D.one_tower_case(O, c)
    T, x = k["T"], k["x"]
    q, t = T.q[0], T.t
    want = D.one_tower(x, q, t)
    assert (want[0] == k["plain"].astype(np.uint64)).all()
    assert [int(v) for v in x[1, 0, :4]] == [q >> 1, (q >> 1) + 1, 0, q - 1]

    def scalar(v):  # mubintvecnat.cpp:420-435, ubintnat.h:536-540, mubintvecnat.cpp:111-136 with Python floats
        mr = lambda y: int(float(t) * (float(y) / float(q)) + 0.5)  # noqa: E731
        r = q - mr(q - v) if v > q >> 1 else mr(v) % q
        if r > q >> 1:
            r += t - q % t
        return r % t if r >= t else r

    for ri in range(16):
        assert scalar(int(x[1, 0, ri])) == int(want[1, ri])
    # the two sides of q / 2 are the two sides of t / 2 (0 when t is even: -t/2 = t/2 mod t)
    assert int(want[1, 0]) in (t // 2, (t + 1) // 2) and int(want[1, 1]) in (t // 2, (t + 1) // 2, 0)
    assert int(want[1, 2]) == 0 and int(want[1, 3]) == 0


def test_times_q_over_t_is_the_exact_scaling():
    """CRT lift of TimesQovert(m) is (Q m + r) / t with r = -Q m mod t: the integer next to Q m / t"""
    rng = np.random.default_rng(3)
    for t, bits, towers in ((65537, 60, 5), (1 << 15, 30, 2), (3221225473, 60, 1)):
        q = D.towers_below(O, 8, bits, towers)
        T = BT.DecryptTables(q, t)
        m = np.array([int(v) for v in rng.integers(0, t, size=16)], dtype=object)
        out = D.times_q_over_t(BR.residues(m.reshape(1, 16), q), T)
        lift = BR.crt_lift(out, q)[0]
        for mi, v in zip(m, lift):
            r = -T.Q * int(mi) % t
            assert (T.Q * int(mi) + r) % t == 0 and int(v) == (T.Q * int(mi) + r) // t % T.Q


def test_decrypt_composition_decrypts():
    """DecryptCore + INTT + ScaleAndRound on a bfv_ref.encrypt ciphertext (2 elements, evaluation form)"""
    log_n, t = 6, 65537
    n = 1 << log_n
    q = D.towers_below(O, log_n, 60, 2)
    rq = [O.root_of_unity(2 << log_n, m) for m in q]
    tb = O.Tables(n, q, rq)
    rng = np.random.default_rng(5)
    s = np.array([int(v) for v in rng.integers(-1, 2, size=n)], dtype=object)
    m = np.array([int(v) for v in rng.integers(0, t, size=n)], dtype=object)
    c0, c1 = BR.encrypt(O, rng, m, s, q, tb, t)
    s_eval = O.ntt_fwd(BR.residues(s.reshape(1, n), q), tb)[0]
    T = BT.DecryptTables(q, t)
    for behz in (False, True):
        assert (D.decrypt(O, [c0, c1], s_eval, T, tb, True, behz)[0] == m.astype(np.uint64)).all()
    coef = [O.ntt_inv(c, tb) for c in (c0, c1)]
    assert (D.decrypt(O, coef, s_eval, T, tb, False)[0] == m.astype(np.uint64)).all()
