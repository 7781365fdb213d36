"""CPU tests of the BGV decryption entry points of the C ABI: the symbols exist with the documented
signatures, ofhe_hip_bgv_decrypt_create refuses each bad argument before it looks at the context (so without a
device), and the calls refuse a NULL handle."""
import ctypes
import re

import pytest

import bgv_decrypt_ref as G
from test_abi_behz import CTYPES, HEADER, header_params

# name -> parameter types as the header spells them, in order
DOCUMENTED = {
    "ofhe_hip_bgv_decrypt_create": ["ofhe_ctx_t", "uint32_t", "uint32_t", "const uint64_t*", "uint64_t",
                                    "ofhe_bgv_decrypt_t*"],
    "ofhe_hip_bgv_decrypt_destroy": ["ofhe_bgv_decrypt_t"],
    "ofhe_hip_bgv_mod_reduce_chain": ["ofhe_bgv_decrypt_t", "uint32_t", "int", "const uint64_t*", "uint64_t*",
                                      "uint32_t", "void*"],
    "ofhe_hip_bgv_decrypt": ["ofhe_bgv_decrypt_t", "ofhe_plan_t", "uint32_t", "uint32_t", "int"] +
                            ["const uint64_t*"] * 4 + ["uint64_t*", "uint32_t", "void*"],
    "ofhe_hip_decrypt_core": ["ofhe_plan_t", "uint32_t", "uint32_t", "int", "int"] + ["const uint64_t*"] * 4 +
                             ["uint64_t*", "uint32_t", "void*"],
}


def test_header_and_binding_agree_on_the_signatures():
    import ofhe_hip as H

    L = H.lib()
    for name, params in DOCUMENTED.items():
        assert header_params(name) == params, name
        assert hasattr(L, name), name
        assert name in H.EXPORTED_SYMBOLS
        res, args = H._SIGS[name]
        assert res is ctypes.c_int and len(args) == len(params), name
        for a, p in zip(args, params):
            if p in ("uint32_t", "uint64_t", "int"):
                exp = CTYPES[p]
            elif p == "ofhe_bgv_decrypt_t*":
                exp = ctypes.POINTER(ctypes.c_void_p)
            elif name == "ofhe_hip_bgv_decrypt_create" and p == "const uint64_t*":
                exp = CTYPES[p]  # the host array of moduli
            else:
                exp = ctypes.c_void_p  # handles, device pointers, the stream
            assert a is exp, (name, p, a)
    limit = re.search(r"#define OFHE_BGV_DECRYPT_MAX_TOWERS (\d+)", open(HEADER).read())
    assert int(limit.group(1)) == H.BGV_DECRYPT_MAX_TOWERS


def _create(H, q, t, log_n=8):
    """the message of the refusal of a create without a context"""
    try:
        H.BgvDecrypt(None, log_n, q, t)
    except H.MathError as e:
        assert str(e).startswith("ofhe_hip error 1:"), e  # OFHE_ERR_ARG
        return str(e)
    raise AssertionError("create succeeded without a context")


def test_create_rejects_bad_arguments_without_a_device():
    import ofhe_hip as H

    q = G.mixed_chain(5)
    t = 65537
    # every argument good: the only complaint left is the missing context, so each check below fires before
    # the context (and with it the device) is touched
    for good_t in (2, t, 1 << 20, q[0] + 2, q[1] + 2):
        assert "context is NULL" in _create(H, q, good_t)
    assert "context is NULL" in _create(H, q[:1], t)
    assert "context is NULL" in _create(H, G.mixed_chain(H.BGV_DECRYPT_MAX_TOWERS), t)
    # t need not be invertible modulo q_0, which is never divided out
    assert "context is NULL" in _create(H, q, 3 * q[0])
    cases = [
        ("t must be at least 2", (q, 1)),
        ("t must be at least 2", (q, 0)),
        ("size_q", ([], t)),
        ("size_q", (G.mixed_chain(H.BGV_DECRYPT_MAX_TOWERS + 1), t)),
        ("odd", ([q[0] - 1] + q[1:], t)),
        ("odd", (q[:4] + [q[4] + 1], t)),
        ("below 2^60", ([(1 << 60) + 33] + q[1:], t)),
        ("below 2^60", (q[:4] + [(1 << 60) + 33], t)),
        ("repeats", (q[:4] + [q[1]], t)),
        ("repeats", ([q[0], q[0]], t)),
        ("t is not invertible modulo modulus 2", (q, q[2])),
        ("t is not invertible modulo modulus 4", (q, 5 * q[4])),
        ("t is not invertible modulo modulus 1", (q, 2 * q[1])),
        ("is not invertible modulo modulus", ([15, 7, 21], 2)),  # distinct, odd, but 21 and 15 share 3
    ]
    for match, (moduli, tt) in cases:
        assert match in _create(H, moduli, tt), (match, moduli, tt)
    assert "log_n" in _create(H, q, t, log_n=18) and "log_n" in _create(H, q, t, log_n=0)
    L = H.lib()
    h = ctypes.c_void_p()
    assert L.ofhe_hip_bgv_decrypt_create(None, 8, 5, None, 65537, ctypes.byref(h)) == 1 and h.value is None
    assert L.ofhe_hip_bgv_decrypt_create(None, 8, 5, H._arr(q), 65537, None) == 1


def test_calls_reject_a_null_handle_without_a_device():
    import ofhe_hip as H

    L = H.lib()
    null = ctypes.c_void_p()
    rcs = [L.ofhe_hip_bgv_decrypt_destroy(null), L.ofhe_hip_bgv_mod_reduce_chain(null, 1, 1, null, null, 1, null),
           L.ofhe_hip_bgv_decrypt(null, null, 1, 2, 1, null, null, null, null, null, 1, null),
           L.ofhe_hip_decrypt_core(null, 1, 2, 1, 0, null, null, null, null, null, 1, null)]
    assert all(rc != 0 for rc in rcs), rcs
    assert L.ofhe_hip_last_error()


def test_binding_names_the_kernel_cap():
    """BGV_CHAIN_K is the kernel header's cap: the GPU tests choose their tower counts around it"""
    import os

    import ofhe_hip as H

    src = open(os.path.join(os.path.dirname(H.__file__), "csrc", "bgv_decrypt_kernels.hpp")).read()
    assert int(re.search(r"constexpr int BGV_CHAIN_K = (\d+);", src).group(1)) == H.BGV_CHAIN_K


@pytest.mark.parametrize("n", [1, 3, 4])
def test_element_layout_is_refused_by_the_library_not_the_binding(n):
    """_c012 passes any count through: 2 or 3 is the library's rule"""
    import ofhe_hip as H

    c = H._c012([16] * n)
    assert len(c) == 3 and [bool(p.value) for p in c] == [True] * min(n, 3) + [False] * (3 - min(n, 3))
