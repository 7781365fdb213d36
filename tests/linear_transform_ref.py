"""Reference composition of the BSGS linear transform (helper, not a test).

One level of FHECKKSRNS::EvalLinearTransform (ckksrns-fhe.cpp:1484-1555) -- the
"double hoisting" loop shared by EvalCoeffsToSlots / EvalSlotsToCoeffs --
restated from functions that exist without the feature:
rotation_ref.fast_rotation_ext_ref, rotation_ref.sigma, rotation_ref.p_mod_q,
K.ks_precompute, K.ks_mod_down, O.eltwise and O.mul_scalar.

    R_i  = identity ? KeySwitchExt(ct, true) : EvalFastRotationExt(ct, baby_index[i], digits(c1), true)
    I_j  = sum_{i present} R_i * diag[j * nbaby + i]          (both elements, over Ql|P)
    identity giant j:  first += ModDown(I_j[0]);  outer[1] += I_j[1]
    other giant j:     (m0, m1) = ModDown(I_j);   first += sigma_kj(m0)
                       outer += EvalFastRotationExt((., m1), giant_index[j], digits(m1), false)
    out0 = ModDown(outer[0]) + first,   out1 = ModDown(outer[1])
"""
import math

import numpy as np

import keyswitch as K
import oracle as O
import rotation_ref as R


def is_identity(k: int, n: int) -> bool:
    return k % (2 * n) == 1


def ext_ref(kp, c):
    """KeySwitchExt on one element (keyswitch-hybrid.cpp:231-256): [B][l][N] -> [B][l+P][N]."""
    B, l, n = c.shape
    out = np.zeros((B, l + len(kp.p), n), np.uint64)
    out[:, :l] = O.mul_scalar(c, R.p_mod_q(kp, l), kp.q[:l])
    return out


def mult_ext_sum_ref(kp, l, x0, x1, diag, present, nsum):
    """x_e [nterm][B][l+P][N], diag [nsum * nterm][l+P][N], present: truth values
    [nsum * nterm] or None -> out_e [nsum][B][l+P][N] (EvalMultExt / EvalAddExtInPlace)."""
    mods = kp.q[:l] + kp.p
    nterm, B = x0.shape[0], x0.shape[1]
    out = [np.zeros((nsum,) + x0.shape[1:], np.uint64) for _ in range(2)]
    for j in range(nsum):
        for i in range(nterm):
            if present is not None and not present[j * nterm + i]:
                continue
            d = np.ascontiguousarray(np.broadcast_to(diag[j * nterm + i], x0.shape[1:]))
            for e, x in enumerate((x0, x1)):
                out[e][j] = O.eltwise("add", out[e][j], O.eltwise("mul", x[i], d, mods), mods)
    return out[0], out[1]


def fast_rotation_ext_sum_ref(kp, digit_sets, indices, keys, addend1=None):
    """digit_sets [nset][B][beta][l+P][N], keys[j] = (kb, ka), addend1 [nadd][B][l+P][N] or None
    -> out0, out1 [B][l+P][N]."""
    l = digit_sets.shape[3] - len(kp.p)
    mods = kp.q[:l] + kp.p
    o0 = np.zeros(digit_sets.shape[1:2] + digit_sets.shape[3:], np.uint64)
    o1 = o0.copy()
    for dg, k, key in zip(digit_sets, indices, keys):
        e0, e1 = R.fast_rotation_ext_ref(kp, np.ascontiguousarray(dg), None, [k], [key])
        o0 = O.eltwise("add", o0, e0[0], mods)
        o1 = O.eltwise("add", o1, e1[0], mods)
    for a in ([] if addend1 is None else addend1):
        o1 = O.eltwise("add", o1, a, mods)
    return o0, o1


def baby_steps_ref(kp, c0, c1, baby_index, baby_keys):
    """R_i, both elements: [nbaby][B][l+P][N] each."""
    n = c0.shape[2]
    rot = [i for i, k in enumerate(baby_index) if not is_identity(k, n)]
    r0, r1 = [None] * len(baby_index), [None] * len(baby_index)
    if rot:
        digits = K.ks_precompute(kp, c1)
        e0, e1 = R.fast_rotation_ext_ref(kp, digits, c0, [baby_index[i] for i in rot], [baby_keys[i] for i in rot])
        for pos, i in enumerate(rot):
            r0[i], r1[i] = e0[pos], e1[pos]
    for i, k in enumerate(baby_index):
        if is_identity(k, n):
            r0[i], r1[i] = ext_ref(kp, c0), ext_ref(kp, c1)
    return np.stack(r0), np.stack(r1)


def bsgs_ref(kp, c0, c1, baby_index, giant_index, baby_keys, giant_keys, diag, present=None, t=0,
             moddown_after_automorphism=()):
    """c0, c1 [B][l][N]; diag [ngiant * nbaby][l+P][N]; keys[i] = (kb, ka) or None at an identity
    step -> out0, out1 [B][l][N].  moddown_after_automorphism: giant steps whose first element is
    rotated before its ModDown instead of after (the order the reference does NOT use; for the
    sensitivity test only)."""
    B, l, n = c0.shape
    ql, mods = kp.q[:l], kp.q[:l] + kp.p
    nb, ng = len(baby_index), len(giant_index)
    r0, r1 = baby_steps_ref(kp, c0, c1, baby_index, baby_keys)
    i0, i1 = mult_ext_sum_ref(kp, l, r0, r1, diag, present, ng)
    first = np.zeros((B, l, n), np.uint64)
    outer0 = np.zeros((B, l + len(kp.p), n), np.uint64)
    outer1 = outer0.copy()
    for j, k in enumerate(giant_index):
        if is_identity(k, n):
            first = O.eltwise("add", first, K.ks_mod_down(kp, i0[j], t), ql)     # KeySwitchDownFirstElement
            outer1 = O.eltwise("add", outer1, i1[j], mods)
            continue
        m0, m1 = K.ks_mod_down(kp, i0[j], t), K.ks_mod_down(kp, i1[j], t)       # KeySwitchDown
        if j in moddown_after_automorphism:
            m0 = K.ks_mod_down(kp, R.sigma(i0[j], k), t)
            first = O.eltwise("add", first, m0, ql)
        else:
            first = O.eltwise("add", first, R.sigma(m0, k), ql)
        e0, e1 = R.fast_rotation_ext_ref(kp, K.ks_precompute(kp, m1), None, [k], [giant_keys[j]])
        outer0 = O.eltwise("add", outer0, e0[0], mods)
        outer1 = O.eltwise("add", outer1, e1[0], mods)
    out0 = O.eltwise("add", K.ks_mod_down(kp, outer0, t), first, ql)
    return out0, K.ks_mod_down(kp, outer1, t)


# ---- the EvalLinearTransform mapping ------------------------------------------
def auto_index_2n_complex(i: int, m: int) -> int:
    """FindAutomorphismIndex2nComplex (the CKKS rotation by i slots): 5^i mod m, m = 2N."""
    return pow(5, i % (m // 4), m) if i >= 0 else pow(pow(5, -1, m), (-i) % (m // 4), m)


def linear_transform_plan(slots: int, n: int, dim1: int = 0):
    """Index arrays and presence of EvalLinearTransform (ckksrns-fhe.cpp:1499-1547):
    bStep = ceil(sqrt(slots)) (or dim1), gStep = ceil(slots / bStep); baby i rotates by i, giant
    j by bStep * j; diagonal bStep * j + i exists while it is < slots."""
    b = dim1 or math.ceil(math.sqrt(slots))
    g = math.ceil(slots / b)
    baby = [auto_index_2n_complex(i, 2 * n) for i in range(b)]
    giant = [auto_index_2n_complex(b * j, 2 * n) for j in range(g)]
    present = [1 if b * j + i < slots else 0 for j in range(g) for i in range(b)]
    return b, g, baby, giant, present
