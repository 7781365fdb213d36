"""CPU tests of the CKKS / BGV multiplication's entry points of the C ABI: the symbols exist with the
documented signatures, the binding agrees with the header, and every argument rule that needs no engine
refuses with OFHE_ERR_ARG before the engine (NULL here: there is no device) is looked at.

The rules that need the engine's dimensions -- size_ql outside the engine, t not invertible modulo a
tower, overlapping buffers -- run after the engine check and are covered on the device by
tests/test_gpu_she_mult.py."""
import ctypes

from test_abi_linear_transform import header_params, _header

DOCUMENTED = {
    "ofhe_hip_ks_rescale": ["ofhe_ks_t", "uint32_t", "int", "uint64_t", "uint32_t", "uint32_t",
                            "const uint64_t* const*", "uint64_t* const*", "uint32_t", "void*"],
    "ofhe_hip_ks_relinearize": ["ofhe_ks_t", "uint32_t", "uint32_t", "const uint64_t* const*",
                                "const uint64_t* const*", "const uint64_t* const*", "uint64_t*", "uint64_t*",
                                "uint64_t", "uint32_t", "void*"],
    "ofhe_hip_ks_eval_mult": ["ofhe_ks_t", "uint32_t", "const uint64_t*", "const uint64_t*", "const uint64_t*",
                              "const uint64_t*", "const uint64_t*", "const uint64_t*", "int", "uint64_t", "uint32_t",
                              "uint64_t*", "uint64_t*", "uint32_t", "void*"],
}
ERR_ARG, ERR_STATE = 1, 4
CKKS, BGV = 0, 1


def test_header_and_binding_agree_on_the_signatures():
    import ofhe_hip as H

    L = H.lib()
    vp = ctypes.c_void_p
    exact = {"uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "int": ctypes.c_int,
             "const uint64_t* const*": ctypes.POINTER(vp), "uint64_t* const*": ctypes.POINTER(vp)}
    for name, params in DOCUMENTED.items():
        assert header_params(name) == params, name
        assert hasattr(L, name), name
        assert name in H.EXPORTED_SYMBOLS
        res, args = H._SIGS[name]
        assert res is ctypes.c_int and len(args) == len(params), name
        for a, p in zip(args, params):
            assert a is exact.get(p, vp), (name, p, a)  # handles, device pointers, the stream: void*


def test_scheme_constants_match_the_header():
    import re

    import ofhe_hip as H

    h = _header()
    assert int(re.search(r"#define\s+OFHE_SHE_CKKS\s+(\d+)", h).group(1)) == H.SHE_CKKS == CKKS
    assert int(re.search(r"#define\s+OFHE_SHE_BGV\s+(\d+)", h).group(1)) == H.SHE_BGV == BGV


def test_argument_checks_come_before_the_engine():
    import ofhe_hip as H

    L = H.lib()
    null = ctypes.c_void_p()
    P = [ctypes.c_void_p(16 * k) for k in range(1, 12)]   # distinct, 16-byte aligned, never dereferenced
    odd = ctypes.c_void_p(24)                             # 8-byte aligned only

    def arg(rc):
        assert rc == ERR_ARG, (rc, L.ofhe_hip_last_error())

    def arr(*v):
        return (ctypes.c_void_p * len(v))(*[getattr(x, "value", x) for x in v])

    # ks_eval_mult(ks, size_ql, c0, c1, d0, d1, key_b, key_a, scheme, t, levels, out0, out1, batch, stream)
    good = [null, 3, P[0], P[1], P[2], P[3], P[4], P[5], CKKS, 0, 1, P[6], P[7], 1, null]
    for k in (2, 3, 6, 7, 11, 12):                       # NULL operand, key, output
        bad = list(good)
        bad[k] = null
        arg(L.ofhe_hip_ks_eval_mult(*bad))
    for k in (4, 5):                                      # exactly one of d0, d1 NULL
        bad = list(good)
        bad[k] = null
        arg(L.ofhe_hip_ks_eval_mult(*bad))
    for k in (2, 5, 11):                                  # misaligned
        bad = list(good)
        bad[k] = odd
        arg(L.ofhe_hip_ks_eval_mult(*bad))
    for over in ({13: 0}, {8: 2}, {8: -1}, {9: 65537}, {8: BGV, 9: 0}, {8: BGV, 9: 1}, {10: 3}, {10: 4},
                 {12: P[6]}):                             # batch, scheme, t against scheme, levels >= size_ql, out0 == out1
        bad = list(good)
        for k, v in over.items():
            bad[k] = v
        arg(L.ofhe_hip_ks_eval_mult(*bad))
    # ks_rescale(ks, size_ql, scheme, t, levels, nelem, x, out, batch, stream)
    x, o = arr(P[0], P[1]), arr(P[2], P[3])
    good = [null, 3, BGV, 65537, 1, 2, x, o, 1, null]
    for over in ({6: None}, {7: None}, {5: 0}, {8: 0}, {6: arr(P[0], None)}, {7: arr(None, P[3])},
                 {6: arr(P[0], odd)}, {2: 7}, {3: 0}, {3: 1}, {2: CKKS}, {4: 0}, {4: 3}, {4: 9}):
        bad = list(good)
        for k, v in over.items():
            bad[k] = v
        arg(L.ofhe_hip_ks_rescale(*bad))
    # ks_relinearize(ks, size_ql, nelem, c, key_b, key_a, out0, out1, t, batch, stream)
    c, kb, ka = arr(P[0], P[1], P[2]), arr(P[3]), arr(P[4])
    good = [null, 3, 3, c, kb, ka, P[5], P[6], 0, 1, null]
    for over in ({3: None}, {4: None}, {5: None}, {6: null}, {7: null}, {2: 2}, {2: 0}, {9: 0},
                 {3: arr(P[0], None, P[2])}, {4: arr(None)}, {5: arr(None)}, {3: arr(P[0], P[1], odd)}, {6: odd},
                 {7: P[5]}):
        bad = list(good)
        for k, v in over.items():
            bad[k] = v
        arg(L.ofhe_hip_ks_relinearize(*bad))
    # with every engine-free argument in order the NULL engine is what is refused
    assert L.ofhe_hip_ks_eval_mult(null, 3, P[0], P[1], P[2], P[3], P[4], P[5], CKKS, 0, 1, P[6], P[7], 1,
                                   null) == ERR_STATE
    assert L.ofhe_hip_ks_eval_mult(null, 3, P[0], P[1], null, null, P[4], P[5], BGV, 2, 0, P[0], P[1], 1,
                                   null) == ERR_STATE   # the square, in place
    assert L.ofhe_hip_ks_rescale(null, 3, BGV, 65537, 2, 2, x, o, 1, null) == ERR_STATE
    assert L.ofhe_hip_ks_relinearize(null, 3, 3, c, kb, ka, P[5], P[6], 0, 1, null) == ERR_STATE
    assert b"NULL" in L.ofhe_hip_last_error()
