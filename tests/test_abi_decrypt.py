"""CPU tests of the BFV decryption entry points of the C ABI: the symbols exist
with the documented signatures, ofhe_hip_bfv_decrypt_create refuses each bad
argument before it looks at the context (so without a device), and the calls
refuse a NULL handle."""
import ctypes
import re

import bfv_tables as BT
import decrypt_ref as D
import oracle as O
from test_abi_behz import CTYPES, HEADER, header_params

# name -> parameter types as the header spells them, in order
DOCUMENTED = {
    "ofhe_hip_bfv_decrypt_create": ["ofhe_ctx_t", "uint32_t", "uint32_t", "const uint64_t*", "uint64_t", "int",
                                    "const ofhe_bfv_decrypt_tables*", "ofhe_bfv_decrypt_t*"],
    "ofhe_hip_bfv_decrypt_destroy": ["ofhe_bfv_decrypt_t"],
    "ofhe_hip_bfv_decrypt_branch": ["ofhe_bfv_decrypt_t", "int*"],
    "ofhe_hip_bfv_decrypt_scale_round": ["ofhe_bfv_decrypt_t", "const uint64_t*", "uint64_t*", "uint32_t", "void*"],
    "ofhe_hip_bfv_decrypt": ["ofhe_bfv_decrypt_t", "ofhe_plan_t", "uint32_t", "int"] + ["const uint64_t*"] * 4 +
                            ["uint64_t*", "uint32_t", "void*"],
    "ofhe_hip_times_q_over_t": ["ofhe_bfv_decrypt_t", "const uint64_t*", "uint64_t*", "uint32_t", "void*"],
}


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
            elif p == "int*":
                exp = ctypes.POINTER(ctypes.c_int)
            elif p == "ofhe_bfv_decrypt_t*":
                exp = ctypes.POINTER(ctypes.c_void_p)
            elif name == "ofhe_hip_bfv_decrypt_create" and p == "const uint64_t*":
                exp = CTYPES[p]  # the host array of moduli
            else:
                exp = ctypes.c_void_p  # handles, device pointers, the tables, the stream
            assert a is exp, (name, p, a)
    fields = re.search(r"typedef struct ofhe_bfv_decrypt_tables \{(.*?)\} ofhe_bfv_decrypt_tables;",
                       open(HEADER).read(), re.S)
    names = re.findall(r"const (?:uint64_t|double)\* (\w+);", fields.group(1))
    assert tuple(names) == BT.DecryptTables.TABLES == tuple(f[0] for f in H.BfvDecryptTablesStruct._fields_)
    enums = dict(re.findall(r"(OFHE_BFV_\w+) = (\d+)", open(HEADER).read()))
    assert (int(enums["OFHE_BFV_BEHZ"]), int(enums["OFHE_BFV_DECRYPT_BEHZ"]), int(enums["OFHE_BFV_DECRYPT_ONE_TOWER"])) \
        == (H.BFV_BEHZ, H.BFV_DECRYPT_BEHZ, H.BFV_DECRYPT_ONE_TOWER) == (BT.BEHZ, 8, 9)


def _create(H, T, technique=0, log_n=8, drop=()):
    """(message of the refusal) of a create without a context; drop: tables to leave NULL"""
    import copy

    T = copy.copy(T)
    for name in drop:
        setattr(T, name, None)
    try:
        H.BfvDecrypt(None, log_n, T, technique)
    except H.MathError as e:
        assert str(e).startswith("ofhe_hip error 1:"), e  # OFHE_ERR_ARG
        return str(e)
    raise AssertionError("create succeeded without a context")


def test_create_rejects_bad_arguments_without_a_device():
    import copy

    import ofhe_hip as H

    def tables(bits, towers, t):
        return BT.DecryptTables(D.towers_below(O, 8, bits, towers), t)

    def changed(T, **kw):
        bad = copy.copy(T)
        for k, v in kw.items():
            setattr(bad, k, v)
        return bad

    split, plain = tables(60, 5, 65537), tables(30, 5, 65537)
    assert split.split and not plain.split
    # every argument good: the only complaint left is the missing context, so each check below fires
    # before the context (and with it the device) is touched
    for T, technique in ((split, H.BFV_HPS), (plain, H.BFV_HPSPOVERQ), (split, H.BFV_BEHZ), (tables(60, 1, 65537), 0)):
        assert "context is NULL" in _create(H, T, technique)
    # the B tables are needed only when the split applies; one tower needs none
    assert "context is NULL" in _create(H, plain, drop=("tQHatInvModqBDivqModt", "tQHatInvModqBDivqFrac"))
    assert "context is NULL" in _create(H, tables(60, 1, 65537), drop=("tInvModq", "negQModt"))
    cases = [
        ("t must be at least 2", dict(T=changed(split, t=1))),
        ("t must be at least 2", dict(T=changed(split, t=0))),
        ("size_q", dict(T=changed(split, q=[]))),
        ("size_q", dict(T=changed(split, q=split.q * 52))),  # 260 towers
        ("below 2^64", dict(T=changed(split, t=(1 << 64) // 10 + 1))),  # 2 * 5 * t >= 2^64
        ("below 2^64", dict(T=changed(split, t=(1 << 63)))),
        ("odd", dict(T=changed(split, q=[split.q[0] - 1] + split.q[1:]))),
        ("below 2^60", dict(T=changed(split, q=[(1 << 60) + 33] + split.q[1:]))),
        ("technique", dict(T=split, technique=3)),
        ("log_n", dict(T=split, log_n=18)),
        ("NULL table", dict(T=split, drop=("tQHatInvModqDivqModt",))),
        ("NULL table", dict(T=split, drop=("tQHatInvModqDivqFrac",))),
        ("NULL B table", dict(T=split, drop=("tQHatInvModqBDivqModt",))),
        ("NULL B table", dict(T=split, drop=("tQHatInvModqBDivqFrac",))),
        ("NULL BEHZ table", dict(T=split, technique=H.BFV_BEHZ, drop=("negInvqModtgamma",))),
        ("NULL BEHZ table", dict(T=split, technique=H.BFV_BEHZ, drop=("tgammaQHatInvModq",))),
        ("2^58", dict(T=changed(split, t=1 << 32), technique=H.BFV_BEHZ)),
        ("come together", dict(T=split, drop=("negQModt",))),
    ]
    for match, kw in cases:
        assert match in _create(H, **kw), (match, kw)
    # the bound 2 size_q t < 2^64 is exact
    five = (1 << 64) // 10
    assert 2 * 5 * five < 1 << 64 <= 2 * 5 * (five + 1)
    assert "context is NULL" in _create(H, changed(split, t=five, split=True))
    assert "below 2^64" in _create(H, changed(split, t=five + 1, split=True))
    L = H.lib()
    h = ctypes.c_void_p()
    assert L.ofhe_hip_bfv_decrypt_create(None, 8, 5, None, 65537, 0, None, ctypes.byref(h)) == 1 and h.value is None


def test_calls_reject_a_null_handle_without_a_device():
    import ofhe_hip as H

    L = H.lib()
    null = ctypes.c_void_p()
    b = ctypes.c_int(-1)
    rcs = [L.ofhe_hip_bfv_decrypt_destroy(null), L.ofhe_hip_bfv_decrypt_branch(null, ctypes.byref(b)),
           L.ofhe_hip_bfv_decrypt_scale_round(null, null, null, 1, null),
           L.ofhe_hip_bfv_decrypt(null, null, 2, 1, null, null, null, null, null, 1, null),
           L.ofhe_hip_times_q_over_t(null, null, null, 1, null)]
    assert all(rc != 0 for rc in rcs), rcs
    assert L.ofhe_hip_last_error() and b.value == -1
