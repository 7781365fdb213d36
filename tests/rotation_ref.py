"""Reference composition of the hoisted rotations (helper, not a test).

LeveledSHECKKSRNS::EvalFastRotationExt (ckksrns-leveledshe.cpp:402-457) and
LeveledSHEBase::EvalFastRotation (base-leveledshe.cpp:471-513) restated from
oracle functions that exist without the feature: K.ks_fast_core_ext,
K.ks_mod_down, K.automorphism, O.eltwise and O.mul_scalar.  The evaluation-form
automorphism of a (N, k) pair is derived once, by applying K.automorphism to
arange(N), and then applied as an index.
"""
from functools import lru_cache

import numpy as np

import keyswitch as K
import oracle as O


@lru_cache(maxsize=None)
def perm(n: int, k: int) -> np.ndarray:
    """AutomorphismTransform(k) in evaluation form as a gather: out[..., p] = x[..., perm[p]]."""
    return K.automorphism(np.arange(n, dtype=np.uint64), k, True, 0).astype(np.int64)


def sigma(x: np.ndarray, k: int) -> np.ndarray:
    return np.ascontiguousarray(x[..., perm(x.shape[-1], k)])


def p_mod_q(kp, l):
    """m_PModq (rns-cryptoparameters.h:340) for the first l towers."""
    P = K._prod(kp.p)
    return [P % q for q in kp.q[:l]]


def inner_products(kp, digits, keys):
    """EvalFastKeySwitchCoreExt per key: [(ct0, ct1)], shared by the callers below."""
    return [K.ks_fast_core_ext(kp, digits, kb, ka) for kb, ka in keys]


def fast_rotation_ext_ref(kp, digits, c0, indices, keys, cts=None):
    """digits [B][beta][l+P][N], c0 [B][l][N] or None (addFirst = false),
    keys[r] = (kb, ka); cts: inner_products(kp, digits, keys) if already at
    hand.  Returns out0, out1: [R][B][l+P][N]."""
    l = digits.shape[2] - len(kp.p)
    ql = kp.q[:l]
    out0, out1 = [], []
    for k, (ct0, ct1) in zip(indices, cts or inner_products(kp, digits, keys)):
        ct0 = ct0.copy()
        if c0 is not None:
            c_mult = O.mul_scalar(c0, p_mod_q(kp, l), ql)              # TimesNoCheck(GetPModq())
            ct0[:, :l] = O.eltwise("add", ct0[:, :l], c_mult, ql)      # (*cTilda)[0] += psiC0
        out0.append(sigma(ct0, k))
        out1.append(sigma(ct1, k))
    return np.stack(out0), np.stack(out1)


def fast_rotation_ref(kp, digits, c0, indices, keys, t=0, cts=None):
    """The reference's order: ModDown, += c0, automorphism.  Returns out0, out1: [R][B][l][N]."""
    l = digits.shape[2] - len(kp.p)
    ql = kp.q[:l]
    out0, out1 = [], []
    for k, (ct0, ct1) in zip(indices, cts or inner_products(kp, digits, keys)):
        b = O.eltwise("add", K.ks_mod_down(kp, ct0, t), c0, ql)        # (*ba)[0] += cv[0]
        out0.append(sigma(b, k))
        out1.append(sigma(K.ks_mod_down(kp, ct1, t), k))
    return np.stack(out0), np.stack(out1)


def inverse_index(k: int, n: int) -> int:
    return pow(k, -1, 2 * n)
