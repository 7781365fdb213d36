"""CPU checks of the hoisted-rotation reference composition (tests/rotation_ref.py)
and of the two C-ABI entry points' argument handling.

1. Semantics with real keys: for a secret s and rotation keys generated as
   KeySwitchGen(s, sigma_{k^-1}(s)), both fast_rotation_ref and
   ModDown(fast_rotation_ext_ref(addFirst)) decrypt under s to
   sigma_k(c0 + c1 s) up to a small error.
2. The evaluation-form automorphism maps every aligned block of 2^m storage
   words onto one aligned block of 2^m storage words (what lets the kernel
   permute on its store without a strided pass).
3. A NULL engine is OFHE_ERR_STATE for both calls, without a device.
"""
import ctypes

import numpy as np
import pytest

import keyswitch as K
import oracle as O
import rotation_ref as R
from test_keyswitch_oracle import _bases, _uniform

OFHE_ERR_STATE = 4


def coeff_automorphism_signed(s, k):
    """X -> X^k on signed coefficients (poly-impl.h:350-361 without a modulus)."""
    n = len(s)
    out = np.zeros(n, dtype=np.int64)
    for j in range(n):
        jk = j * k
        out[jk % n] = -s[j] if (jk // n) & 1 else s[j]
    return out


@pytest.mark.parametrize("log_n,sq,sp,dnum", [(4, 4, 2, 2), (6, 5, 3, 2), (10, 6, 2, 3)])
def test_reference_composition_semantics(log_n, sq, sp, dnum):
    n = 1 << log_n
    q, rq, p, rp = _bases(log_n, sq, sp)
    kp = K.KeySwitchParams(n, q, rq, p, rp, dnum)
    rng = np.random.default_rng(7)
    s = K.ternary(n, rng)
    s_eval = K.small_poly_eval(s, q, rq)
    c0 = K.set_format(_uniform(rng, 1, q, n), q, rq, True)
    c1 = K.set_format(_uniform(rng, 1, q, n), q, rq, True)
    digits = K.ks_precompute(kp, c1)
    indices = [5, 2 * n - 1, pow(5, 3, 2 * n)]
    keys = [K.keyswitch_gen(kp, s, coeff_automorphism_signed(s, R.inverse_index(k, n)), rng) for k in indices]
    msg = O.eltwise("add", c0, O.eltwise("mul", c1, s_eval, q), q)

    def max_err(o0, o1, k):
        lhs = O.eltwise("add", o0, O.eltwise("mul", o1, s_eval, q), q)
        d = K.set_format(O.eltwise("sub", lhs, R.sigma(msg, k), q), q, rq, False)
        return max(abs(e) for e in K.crt_centered(d[0], q))

    o0, o1 = R.fast_rotation_ref(kp, digits, c0, indices, keys)
    e0, e1 = R.fast_rotation_ext_ref(kp, digits, c0, indices, keys)
    for r, k in enumerate(indices):
        err = max_err(o0[r], o1[r], k)
        err_ext = max_err(K.ks_mod_down(kp, e0[r]), K.ks_mod_down(kp, e1[r]), k)
        print(f"log_n {log_n} k {k}: error bits {err.bit_length()} (non-Ext), {err_ext.bit_length()} (Ext + ModDown)")
        assert err < 1 << 20 and err_ext < 1 << 20
    # the message itself is Q-sized: the bound is not met trivially
    assert max(abs(e) for e in K.crt_centered(K.set_format(msg, q, rq, False)[0], q)) > 1 << 200


@pytest.mark.parametrize("log_n", [4, 9, 12])
def test_evaluation_automorphism_is_block_local(log_n):
    n = 1 << log_n
    for k in (3, 5, 25, 2 * n - 1, pow(5, 7, 2 * n)):
        src = R.perm(n, k)
        assert sorted(src.tolist()) == list(range(n))
        for m in sorted({1, 3, min(8, log_n)}):
            blocks = src.reshape(-1, 1 << m)
            assert np.all(blocks >> m == blocks[:, :1] >> m), (n, k, m)  # one source block per output block


def test_index_is_taken_mod_2n():
    n = 16
    assert np.array_equal(R.perm(n, 5), R.perm(n, 5 + 2 * n)) and np.array_equal(R.perm(n, 1), np.arange(n))


def test_null_engine_is_a_state_error_without_device():
    import ofhe_hip as H

    L = H.lib()
    null = ctypes.c_void_p()
    assert L.ofhe_hip_ks_fast_rotation_ext(null, 1, null, null, 1, None, None, None, null, null, 1,
                                           null) == OFHE_ERR_STATE
    assert L.ofhe_hip_last_error()
    assert L.ofhe_hip_ks_fast_rotation(null, 1, null, null, 1, None, None, None, null, null, 0, 1,
                                       null) == OFHE_ERR_STATE
    assert set(H.EXPORTED_SYMBOLS) >= {"ofhe_hip_ks_fast_rotation_ext", "ofhe_hip_ks_fast_rotation"}
