"""CPU tests of the BEHZ entry points of the C ABI: the symbols exist with the
documented signatures, and ofhe_hip_behz_create refuses each bad argument
before it looks at the context (so without a device)."""
import ctypes
import os
import re

import behz_ref as Z
import bfv_tables as BT
from conftest import ROOT

KAT = Z.load_vectors()
HEADER = os.path.join(ROOT, "include", "ofhe_hip.h")

# name -> parameter types as the header spells them, in order
DOCUMENTED = {
    "ofhe_hip_behz_create": ["ofhe_ctx_t", "uint32_t", "uint32_t", "const uint64_t*", "uint32_t", "const uint64_t*",
                             "uint64_t", "const ofhe_behz_tables*", "ofhe_behz_t*"],
    "ofhe_hip_behz_destroy": ["ofhe_behz_t"],
    "ofhe_hip_behz_q_to_bsk": ["ofhe_behz_t", "const uint64_t*", "uint64_t*", "uint32_t", "void*"],
    "ofhe_hip_behz_expand": ["ofhe_behz_t", "ofhe_plan_t", "ofhe_plan_t", "int", "const uint64_t*", "uint64_t*",
                             "uint32_t", "void*"],
    "ofhe_hip_behz_floor": ["ofhe_behz_t", "const uint64_t*", "uint64_t*", "uint32_t", "void*"],
    "ofhe_hip_behz_conv_sk": ["ofhe_behz_t", "const uint64_t*", "uint64_t*", "uint32_t", "void*"],
    "ofhe_hip_behz_floor_sk": ["ofhe_behz_t", "int", "const uint64_t*", "uint64_t*", "uint32_t", "void*"],
    "ofhe_hip_bfv_eval_mult_behz": ["ofhe_behz_t", "ofhe_plan_t", "ofhe_plan_t", "ofhe_plan_t"] +
                                   ["const uint64_t*"] * 4 + ["uint64_t*"] * 3 + ["uint32_t", "void*"],
}
CTYPES = {"uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "int": ctypes.c_int,
          "const uint64_t*": ctypes.POINTER(ctypes.c_uint64)}


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
        res, args = H._SIGS[name]
        assert res is ctypes.c_int and len(args) == len(params), name
        for a, p in zip(args, params):
            if p in ("uint32_t", "uint64_t", "int"):
                exp = CTYPES[p]
            elif p == "ofhe_behz_t*":
                exp = ctypes.POINTER(ctypes.c_void_p)
            elif name == "ofhe_hip_behz_create" and p == "const uint64_t*":
                exp = CTYPES[p]  # host arrays of moduli
            else:
                exp = ctypes.c_void_p  # handles, device pointers, the stream
            assert a is exp, (name, p, a)
    fields = re.search(r"typedef struct ofhe_behz_tables \{(.*?)\} ofhe_behz_tables;", open(HEADER).read(), re.S)
    names = re.findall(r"const uint64_t\* (\w+);", fields.group(1))
    assert tuple(names) == BT.BehzTables.TABLES == tuple(f[0] for f in H.BehzTablesStruct._fields_)


def _create(L, H, T, size_q=None, size_b=None, drop=None, log_n=3):
    keep = {name: H._arr(T.flat(name)) for name in T.TABLES}
    ts = H.BehzTablesStruct(**{k: ctypes.cast(a, ctypes.POINTER(ctypes.c_uint64)) for k, a in keep.items()
                               if k != drop})
    h = ctypes.c_void_p()
    rc = L.ofhe_hip_behz_create(None, log_n, len(T.q) if size_q is None else size_q, H._arr(T.q),
                                len(T.b) if size_b is None else size_b, H._arr(T.bsk), T.t,
                                ctypes.cast(ctypes.byref(ts), ctypes.c_void_p), ctypes.byref(h))
    assert h.value is None
    return rc, L.ofhe_hip_last_error().decode()


def test_create_rejects_bad_arguments_without_a_device():
    import copy

    import ofhe_hip as H

    L = H.lib()
    T = BT.BehzTables(KAT["q"], KAT["bsk"][:-1], KAT["bsk"][-1], KAT["t"])

    def with_moduli(q=T.q, b=T.b, msk=T.msk):
        bad = copy.copy(T)
        bad.q, bad.b, bad.bsk = list(q), list(b), list(b) + [msk]
        return bad

    ERR_ARG = 1
    # every argument good: the only complaint left is the missing context, so each check below
    # fires before the context (and with it the device) is touched
    assert _create(L, H, T) == (ERR_ARG, "context is NULL")
    cases = [
        ("odd", dict(T=with_moduli(q=[T.q[0], T.q[1] + 1]))),
        ("odd", dict(T=with_moduli(b=[T.b[0] - 1, T.b[1]]))),
        ("below 2^60", dict(T=with_moduli(q=[(1 << 60) + 33, T.q[1]]))),
        ("below 2^60", dict(T=with_moduli(msk=(1 << 61) + 1))),
        ("exceed 2^16", dict(T=with_moduli(b=[T.b[0], (1 << 16) - 15]))),
        ("exceed 2^16", dict(T=with_moduli(msk=(1 << 16) - 15))),
        ("repeated", dict(T=with_moduli(q=[T.q[0], T.q[0]]))),
        ("repeated", dict(T=with_moduli(b=[T.b[0], T.q[1]]))),
        ("repeated", dict(T=with_moduli(msk=T.b[0]))),
        ("size_q", dict(T=T, size_q=0)),
        ("size_q", dict(T=T, size_q=256)),
        ("size_b", dict(T=T, size_b=0)),
        ("size_b", dict(T=T, size_b=256)),
        ("log_n", dict(T=T, log_n=18)),
    ] + [("NULL table", dict(T=T, drop=name)) for name in T.TABLES]
    for match, kw in cases:
        rc, msg = _create(L, H, **kw)
        assert rc == ERR_ARG and match in msg, (match, kw, rc, msg)
    h = ctypes.c_void_p()
    assert L.ofhe_hip_behz_create(None, 3, 2, None, 2, H._arr(T.bsk), T.t, None, ctypes.byref(h)) == ERR_ARG


def test_calls_reject_a_null_handle_without_a_device():
    import ofhe_hip as H

    L = H.lib()
    null = ctypes.c_void_p()
    rcs = [L.ofhe_hip_behz_destroy(null), L.ofhe_hip_behz_q_to_bsk(null, null, null, 1, null),
           L.ofhe_hip_behz_expand(null, null, null, 1, null, null, 1, null),
           L.ofhe_hip_behz_floor(null, null, null, 1, null), L.ofhe_hip_behz_conv_sk(null, null, null, 1, null),
           L.ofhe_hip_behz_floor_sk(null, 2, null, null, 1, null),
           L.ofhe_hip_bfv_eval_mult_behz(null, null, null, null, null, null, null, null, null, null, null, 1, null)]
    assert all(rc != 0 for rc in rcs), rcs
    assert L.ofhe_hip_last_error()
