"""CPU tests of the entry points of BV key switching with a digit size: the symbols exist with the documented
signatures, the binding agrees with the header, and every argument rule that needs no plan refuses with
OFHE_ERR_ARG before the plan (NULL here: there is no device) is looked at.

The rules that need the plan -- towers outside [1, plan towers], n_digits above the towers' digit count,
partial overlaps -- run after the plan check and are covered on the device by tests/test_gpu_bv_digits.py."""
import ctypes

import pytest

from test_abi_linear_transform import header_params

U32, CP, MP = "uint32_t", "const uint64_t*", "uint64_t*"
DOCUMENTED = {
    "ofhe_hip_bv_digit_count": ["ofhe_plan_t", U32, U32, "uint32_t*"],
    "ofhe_hip_bv_precompute_digits": ["ofhe_plan_t", U32, U32, CP, MP, U32, "void*"],
    "ofhe_hip_bv_core_digits": ["ofhe_plan_t", U32, U32, CP, CP, CP, U32, MP, MP, U32, "void*"],
    "ofhe_hip_bv_key_switch": ["ofhe_plan_t", U32, U32, CP, CP, CP, U32, CP, CP, MP, MP, U32, U32, "void*"],
}
ERR_ARG, ERR_STATE = 1, 4


def test_header_and_binding_agree_on_the_signatures():
    import ofhe_hip as H

    L = H.lib()
    vp = ctypes.c_void_p
    for name, params in DOCUMENTED.items():
        assert header_params(name) == params, name
        assert hasattr(L, name), name
        assert name in H.EXPORTED_SYMBOLS
        res, args = H._SIGS[name]
        assert res is ctypes.c_int and len(args) == len(params), name
        for a, p in zip(args, params):
            assert a is (ctypes.c_uint32 if p == U32 else vp), (name, p, a)
    for method in ("bv_digit_count", "bv_precompute_digits", "bv_core_digits", "bv_key_switch"):
        assert callable(getattr(H.NTTPlan, method))


def test_argument_rules_come_before_the_plan():
    import ofhe_hip as H

    L = H.lib()
    null = ctypes.c_void_p()
    P = [ctypes.c_void_p(16 * k) for k in range(1, 12)]   # distinct, 16-byte aligned, never dereferenced
    odd = ctypes.c_void_p(24)                             # 8-byte aligned only
    cnt = ctypes.c_uint32(0)

    def refused(fn, good, overs):
        for over in overs:
            bad = list(good)
            for k, v in over.items():
                bad[k] = v
            rc = fn(*bad)
            assert rc == ERR_ARG, (fn.__name__, over, rc, L.ofhe_hip_last_error())
        assert fn(*good) == ERR_STATE, fn.__name__       # with every plan-free rule in order: the NULL plan
        assert b"NULL" in L.ofhe_hip_last_error()

    # bv_digit_count(plan, towers, digit_size, count)
    refused(L.ofhe_hip_bv_digit_count, [null, 3, 20, ctypes.addressof(cnt)], [{2: 31}, {2: 64}, {3: null}])
    # bv_precompute_digits(plan, towers, digit_size, c, digits, batch, stream)
    refused(L.ofhe_hip_bv_precompute_digits, [null, 3, 20, P[0], P[1], 1, null],
            [{3: null}, {4: null}, {5: 0}, {3: odd}, {4: odd}, {2: 31}, {2: 1 << 31}])
    # bv_core_digits(plan, towers, n_digits, digits, key_b, key_a, key_towers, out0, out1, batch, stream)
    refused(L.ofhe_hip_bv_core_digits, [null, 3, 9, P[0], P[1], P[2], 3, P[3], P[4], 1, null],
            [{k: null} for k in (3, 4, 5, 7, 8)] + [{k: odd} for k in (3, 4, 5, 7, 8)] +
            [{9: 0}, {2: 0}, {6: 2}, {7: P[0]}, {8: P[0]}, {8: P[3]}])
    # bv_key_switch(plan, towers, digit_size, c, key_b, key_a, key_towers, add0, add1, out0, out1, chunk, batch, stream)
    good = [null, 3, 20, P[0], P[1], P[2], 3, P[3], P[4], P[5], P[6], 0, 1, null]
    refused(L.ofhe_hip_bv_key_switch, good,
            [{k: null} for k in (3, 4, 5, 9, 10)] + [{k: odd} for k in (3, 4, 5, 7, 8, 9, 10)] +
            [{12: 0}, {2: 31}, {6: 2}, {10: P[5]}])
    # either addend may be NULL, each may be its own output, and c may be an output: the plan is what is refused
    for over in ({7: null}, {8: null}, {7: null, 8: null}, {7: P[5], 8: P[6]}, {10: P[0]}, {2: 0}, {2: 30}):
        ok = list(good)
        for k, v in over.items():
            ok[k] = v
        assert L.ofhe_hip_bv_key_switch(*ok) == ERR_STATE, over


def test_device_free_digit_count():
    import ofhe_hip as H

    q = [(1 << 60) - 93, (1 << 59) - 55, (1 << 30) - 35, (1 << 22) - 3]
    assert [x.bit_length() for x in q] == [60, 59, 30, 22]
    assert H.bv_digit_count(q, 0) == 4
    assert H.bv_digit_count(q, 1) == 60 + 59 + 30 + 22
    assert H.bv_digit_count(q, 7) == 9 + 9 + 5 + 4
    assert H.bv_digit_count(q, 29) == 3 + 3 + 2 + 1
    assert H.bv_digit_count(q, 30) == 2 + 2 + 1 + 1
    assert H.bv_digit_count(q[:2], 20) == 6
    for r in (31, 64, -1):
        with pytest.raises(H.MathError):
            H.bv_digit_count(q, r)
