"""CPU tests of the BSGS linear transform's entry points of the C ABI: the symbols exist with the
documented signatures, the binding agrees with the header, and every argument check that needs no
engine refuses with OFHE_ERR_ARG before the engine (NULL here: there is no device) is looked at.

The three checks that need the engine's dimensions -- diag_stride < (l + P) N, a NULL key at a
non-identity step (identity is "index = 1 mod 2N") and outputs aliasing inputs -- run after the
engine check and are covered on the device by tests/test_gpu_linear_transform.py."""
import ctypes
import os
import re

from conftest import ROOT

HEADER = os.path.join(ROOT, "include", "ofhe_hip.h")

DOCUMENTED = {
    "ofhe_hip_ks_ext": ["ofhe_ks_t", "uint32_t", "const uint64_t*", "uint64_t*", "uint32_t", "void*"],
    "ofhe_hip_ks_mult_ext_sum": ["ofhe_ks_t", "uint32_t", "uint32_t", "const uint64_t*", "const uint64_t*",
                                 "uint64_t", "const uint64_t*", "uint64_t", "const uint8_t*", "uint32_t",
                                 "uint64_t*", "uint64_t*", "uint32_t", "void*"],
    "ofhe_hip_ks_fast_rotation_ext_sum": ["ofhe_ks_t", "uint32_t", "uint32_t", "const uint64_t*", "const uint32_t*",
                                          "const uint64_t* const*", "const uint64_t* const*", "const uint64_t*",
                                          "uint32_t", "uint64_t*", "uint64_t*", "uint32_t", "void*"],
    "ofhe_hip_ks_bsgs_transform": ["ofhe_ks_t", "uint32_t", "const ofhe_bsgs*", "const uint64_t*", "const uint64_t*",
                                   "uint64_t*", "uint64_t*", "uint64_t", "uint32_t", "void*"],
}
BSGS_FIELDS = ["nbaby", "ngiant", "baby_index", "giant_index", "baby_key_b", "baby_key_a", "giant_key_b",
               "giant_key_a", "diag", "diag_stride", "present"]
ERR_ARG, ERR_STATE = 1, 4


def _header():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def header_params(name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", _header())
    assert m, name
    out = []
    for p in m.group(1).split(","):
        words = p.replace("*", "* ").split()
        out.append(" ".join(words[:-1]).replace(" *", "*"))  # drop the parameter's name
    return out


def test_header_and_binding_agree_on_the_signatures():
    import ofhe_hip as H

    L = H.lib()
    vp = ctypes.c_void_p
    exact = {"uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64,
             "const uint8_t*": ctypes.POINTER(ctypes.c_uint8), "const uint32_t*": ctypes.POINTER(ctypes.c_uint32),
             "const uint64_t* const*": ctypes.POINTER(vp), "const ofhe_bsgs*": ctypes.POINTER(H.Bsgs)}
    for name, params in DOCUMENTED.items():
        assert header_params(name) == params, name
        assert hasattr(L, name), name
        assert name in H.EXPORTED_SYMBOLS
        res, args = H._SIGS[name]
        assert res is ctypes.c_int and len(args) == len(params), name
        for a, p in zip(args, params):
            assert a is exact.get(p, vp), (name, p, a)  # handles, device pointers, the stream: void*


def test_bsgs_struct_matches_the_header():
    import ofhe_hip as H

    m = re.search(r"typedef\s+struct\s+ofhe_bsgs\s*\{(.*?)\}\s*ofhe_bsgs\s*;", _header(), flags=re.S)
    assert m
    names = [re.sub(r"\W", "", w) for decl in m.group(1).split(";") if decl.strip()
             for w in decl.split(",") for w in [w.split()[-1]]]
    assert names == BSGS_FIELDS == [f[0] for f in H.Bsgs._fields_]
    # natural alignment of a C struct with these members
    assert ctypes.sizeof(H.Bsgs) == 8 + 6 * 8 + 8 + 8 + 8
    assert H.Bsgs.baby_index.offset == 8 and H.Bsgs.diag_stride.offset == 64


def _bsgs(H, **over):
    """A well-formed descriptor over fake pointers (never dereferenced on the paths tested here)."""
    idx = (ctypes.c_uint32 * 2)(1, 5)
    keys = (ctypes.c_void_p * 2)(8, 8)
    f = dict(nbaby=2, ngiant=2, baby_index=idx, giant_index=idx, baby_key_b=keys, baby_key_a=keys,
             giant_key_b=keys, giant_key_a=keys, diag=ctypes.c_void_p(8), diag_stride=1 << 20, present=None)
    f.update(over)
    tr = H.Bsgs(**f)
    tr._keep = (idx, keys, f)
    return tr


def test_argument_checks_come_before_the_engine():
    import ofhe_hip as H

    L = H.lib()
    null, a, b, c, d = ctypes.c_void_p(), ctypes.c_void_p(8), ctypes.c_void_p(16), ctypes.c_void_p(24), \
        ctypes.c_void_p(32)
    idx = (ctypes.c_uint32 * 2)(1, 5)
    even = (ctypes.c_uint32 * 2)(1, 6)
    keys = (ctypes.c_void_p * 2)(8, 8)
    nokey = (ctypes.c_void_p * 2)(8, None)

    def arg(rc):
        assert rc == ERR_ARG, (rc, L.ofhe_hip_last_error())

    # KeySwitchExt: NULL data, batch 0
    arg(L.ofhe_hip_ks_ext(null, 1, null, b, 1, null))
    arg(L.ofhe_hip_ks_ext(null, 1, a, null, 1, null))
    arg(L.ofhe_hip_ks_ext(null, 1, a, b, 0, null))
    # mult_ext_sum: NULL data, zero counts, out0 == out1
    good = [null, 1, 2, a, b, 1 << 20, c, 1 << 20, None, 2, d, ctypes.c_void_p(40), 1, null]
    for k in (3, 4, 6, 10, 11):
        bad = list(good)
        bad[k] = null
        arg(L.ofhe_hip_ks_mult_ext_sum(*bad))
    for k in (2, 9, 12):
        bad = list(good)
        bad[k] = 0
        arg(L.ofhe_hip_ks_mult_ext_sum(*bad))
    bad = list(good)
    bad[11] = bad[10]
    arg(L.ofhe_hip_ks_mult_ext_sum(*bad))
    # fast_rotation_ext_sum: NULL data and arrays, zero counts, NULL key, even index, out0 == out1,
    # an addend without its count
    good = [null, 1, 2, a, idx, keys, keys, null, 0, b, c, 1, null]
    for k, v in ((3, null), (4, None), (5, None), (6, None), (9, null), (10, null), (2, 0), (11, 0), (4, even),
                 (5, nokey), (6, nokey), (10, b), (7, d), (8, 1)):
        bad = list(good)
        bad[k] = v
        arg(L.ofhe_hip_ks_fast_rotation_ext_sum(*bad))
    # bsgs_transform: NULL descriptor, data, arrays; zero counts; even indices; out0 == out1
    call = lambda tr, c0=a, c1=b, o0=c, o1=d, batch=1: L.ofhe_hip_ks_bsgs_transform(  # noqa: E731
        null, 1, ctypes.byref(tr) if tr is not None else None, c0, c1, o0, o1, 0, batch, null)
    arg(call(None))
    for kw in (dict(c0=null), dict(c1=null), dict(o0=null), dict(o1=null), dict(batch=0), dict(o1=c)):
        arg(call(_bsgs(H), **kw))
    for over in (dict(diag=None), dict(baby_index=None), dict(giant_index=None), dict(baby_key_b=None),
                 dict(baby_key_a=None), dict(giant_key_b=None), dict(giant_key_a=None), dict(nbaby=0),
                 dict(ngiant=0), dict(baby_index=even), dict(giant_index=even)):
        arg(call(_bsgs(H, **over)))
    # with every engine-free argument in order the NULL engine is what is refused
    assert call(_bsgs(H)) == ERR_STATE
    assert L.ofhe_hip_ks_ext(null, 1, a, b, 1, null) == ERR_STATE
    assert b"NULL" in L.ofhe_hip_last_error()
