"""CPU tests of the HPSPOVERQLEVELED entry points of the C ABI: the symbols exist with the
documented signatures, the binding agrees with the header, and every entry point refuses bad
arguments before it touches a device."""
import ctypes
import os
import re

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "ofhe_hip.h")

# name -> parameter types as the header spells them, in order
DOCUMENTED = {
    "ofhe_hip_bfv_level_create": ["ofhe_ctx_t", "uint32_t"] + ["ofhe_plan_t"] * 4 + ["ofhe_bconv_t"] * 3 +
                                 ["ofhe_scale_round_t"] * 2 + ["const uint64_t*", "ofhe_bfv_level_t*"],
    "ofhe_hip_bfv_level_destroy": ["ofhe_bfv_level_t"],
    "ofhe_hip_expand_ql_hat": ["ofhe_bfv_level_t", "const uint64_t*", "const uint64_t*", "uint64_t*", "uint32_t",
                               "void*"],
    "ofhe_hip_scale_round_expand_ql_hat": ["ofhe_bfv_level_t", "const uint64_t*", "uint64_t*", "uint32_t", "void*"],
    "ofhe_hip_bfv_eval_mult_leveled": ["ofhe_bfv_level_t"] + ["const uint64_t*"] * 4 + ["uint64_t*"] * 3 +
                                      ["uint32_t", "void*"],
    "ofhe_hip_bfv_relinearize_leveled": ["ofhe_bfv_level_t", "ofhe_ks_t", "uint32_t", "int"] +
                                        ["const uint64_t*"] * 5 + ["uint64_t*"] * 2 + ["uint32_t", "void*"],
}
CTYPES = {"uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "int": ctypes.c_int}
ERR_ARG, ERR_STATE = 1, 4


def header_params(name):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", src)
    assert m, name
    out = []
    for p in m.group(1).split(","):
        words = p.replace("*", "* ").split()
        out.append(" ".join(words[:-1]).replace(" *", "*"))  # drop the parameter's name
    return out


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
            if p in CTYPES:
                exp = CTYPES[p]
            elif p == "ofhe_bfv_level_t*":
                exp = ctypes.POINTER(ctypes.c_void_p)
            elif name == "ofhe_hip_bfv_level_create" and p == "const uint64_t*":
                exp = ctypes.POINTER(ctypes.c_uint64)  # the host array ql_hat_modq
            else:
                exp = ctypes.c_void_p  # handles, device pointers, the stream
            assert a is exp, (name, p, a)
    err = re.search(r"OFHE_ERR_ARG\s*=\s*(\d+)", open(HEADER).read())
    assert err is None or int(err.group(1)) == ERR_ARG


def test_create_rejects_null_arguments_without_a_device():
    import ofhe_hip as H

    L = H.lib()
    h = ctypes.c_void_p()
    one = H._arr([1])
    fake = ctypes.c_void_p(8)  # never dereferenced: the NULL checks come first
    # no context, no output slot, no table
    assert L.ofhe_hip_bfv_level_create(None, 0, fake, fake, fake, fake, fake, fake, fake, None, fake, one,
                                       ctypes.byref(h)) == ERR_ARG
    assert b"NULL argument" in L.ofhe_hip_last_error()
    assert L.ofhe_hip_bfv_level_create(fake, 0, fake, fake, fake, fake, fake, fake, fake, None, fake, one,
                                       None) == ERR_ARG
    assert L.ofhe_hip_bfv_level_create(fake, 0, fake, fake, fake, fake, fake, fake, fake, None, fake, None,
                                       ctypes.byref(h)) == ERR_ARG
    # each composed handle missing in turn (drop alone may be NULL)
    for k in (2, 3, 4, 5, 6, 7, 8, 10):
        args = [fake, 0, fake, fake, fake, fake, fake, fake, fake, None, fake, one, ctypes.byref(h)]
        args[k] = None
        assert L.ofhe_hip_bfv_level_create(*args) == ERR_STATE, k
        assert b"NULL object" in L.ofhe_hip_last_error()
    assert h.value is None


def test_calls_reject_bad_arguments_without_a_device():
    import ofhe_hip as H

    L = H.lib()
    null = ctypes.c_void_p()
    rcs = [L.ofhe_hip_bfv_level_destroy(null),
           L.ofhe_hip_expand_ql_hat(null, null, null, null, 1, null),
           L.ofhe_hip_scale_round_expand_ql_hat(null, null, null, 1, null),
           L.ofhe_hip_bfv_eval_mult_leveled(null, null, null, null, null, null, null, null, 1, null),
           L.ofhe_hip_bfv_relinearize_leveled(null, null, 3, 1, null, null, null, null, null, null, null, 1, null)]
    assert all(rc != 0 for rc in rcs), rcs
    assert b"NULL" in L.ofhe_hip_last_error()
