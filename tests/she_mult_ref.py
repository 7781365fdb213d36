"""CKKS / BGV EvalMult, EvalSquare, Relinearize and ModReduceInternalInPlace restated from the CPU oracle's
pieces, in the reference's order of operations: the yardstick of tests/test_gpu_she_mult.py and
tests/test_cpp_she_mult.py.  Built only from oracle.eltwise, keyswitch.ks_core, drop_last_and_scale,
mod_reduce and rescale_tables; never from the device's own composition.

All polynomials are uint64 [batch][towers][N] in evaluation form over kp.q[:l], l = the towers given."""
import numpy as np

import keyswitch as K
import oracle as O

CKKS, BGV = 0, 1


def _mul(a, b, q):
    return O.eltwise("mul", np.ascontiguousarray(a), np.ascontiguousarray(b), list(q))


def _add(a, b, q):
    return O.eltwise("add", np.ascontiguousarray(a), np.ascontiguousarray(b), list(q))


def eval_mult_core(c0, c1, d0, d1, q):
    """LeveledSHEBase::EvalMultCore, base-leveledshe.cpp:667-672."""
    o2 = _mul(c1, d1, q)
    o1 = _mul(c1, d0, q)
    o0 = _mul(d0, c0, q)
    o1 = _add(o1, _mul(c0, d1, q), q)
    return o0, o1, o2


def eval_square_core(c0, c1, q):
    """LeveledSHEBase::EvalSquareCore, base-leveledshe.cpp:707-713."""
    o0 = _mul(c0, c0, q)
    o2 = _mul(c1, c1, q)
    tmp = _mul(c0, c1, q)
    return o0, _add(tmp, tmp, q), o2


def bgv_neg_t_inv(t, ql):
    """negtInvModq of the dropped tower (bgvrns-cryptoparameters.cpp:91-107)."""
    return (int(ql) - pow(int(t) % int(ql), -1, int(ql))) % int(ql)


def rescale_once(x, q, rq, scheme, t):
    """One ModReduceInternalInPlace level on one element over the towers q: DropLastElementAndScale
    (ckksrns-leveledshe.cpp:107-132) or ModReduce (bgvrns-leveledshe.cpp:45-77), with the tables of
    rescale_tables (Python integers)."""
    c, a = K.rescale_tables(q)
    if scheme == CKKS:
        return K.drop_last_and_scale(x, q, rq, True, c, a)
    return K.mod_reduce(x, q, rq, True, int(t), bgv_neg_t_inv(t, q[-1]), a)


def rescale(kp, elements, scheme, t, levels):
    """`levels` rescalings of every element, one level after another."""
    out = []
    for x in elements:
        l = x.shape[1]
        for lv in range(levels):
            x = rescale_once(x, kp.q[:l - lv], kp.rq[:l - lv], scheme, t)
        out.append(x)
    return out


def relinearize(kp, elements, keys, t=0):
    """LeveledSHEBase::RelinearizeInPlace, base-leveledshe.cpp:357-372: keys[j - 2] = (key_b, key_a) for
    element j."""
    l = elements[0].shape[1]
    q = kp.q[:l]
    o0, o1 = elements[0], elements[1]
    for j in range(2, len(elements)):
        kb, ka = keys[j - 2]
        a0, a1 = K.ks_core(kp, elements[j], kb, ka, t)
        o0, o1 = _add(o0, a0, q), _add(o1, a1, q)
    return o0, o1


def eval_mult(kp, c0, c1, d0, d1, kb, ka, scheme=CKKS, t=0, levels=0):
    """LeveledSHEBase::EvalMult(ct1, ct2, evalKey), base-leveledshe.cpp:199-218, then `levels` rescalings;
    d0 is None: EvalSquare(ct, evalKey), 262-280."""
    q = kp.q[:c0.shape[1]]
    cv = eval_square_core(c0, c1, q) if d0 is None else eval_mult_core(c0, c1, d0, d1, q)
    o0, o1 = relinearize(kp, list(cv), [(kb, ka)], t)
    if levels:
        o0, o1 = rescale(kp, [o0, o1], scheme, t, levels)
    return o0, o1
