"""Every kernel of the shipped library allocates at least 64 VGPRs.

The round-2 EvalMultCore kernel (grid-stride k_tensor2) returned wrong words
whenever its 56-VGPR waves shared a CU with other workgroups; its unchanged
machine code with the allocation raised to 64 or 72 VGPRs is exact
(tools/diag/tensor2_asm_diag.hip, DESIGN.md "The round-2 EvalMultCore
failure").  csrc/arith.hpp's OFHE_VGPR_FLOOR() holds every kernel at >= 64.
This test reads the allocation each kernel's descriptor asks the hardware for
(COMPUTE_PGM_RSRC1.GRANULATED_WORKITEM_VGPR_COUNT, granule 8 on gfx950) from
every gfx950 code object inside the built library (one offload bundle per
translation unit) -- no GPU needed.
"""
import os
import struct

import pytest

LIB = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "upmem--openfhe_amd", "lib", "libofhe_hip.so")


def _sections(elf):
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", elf, 0x3A)
    secs = []
    for i in range(shnum):
        name, typ, flags, addr, off, size, link, info, align, entsize = struct.unpack_from(
            "<IIQQQQIIQQ", elf, shoff + i * shentsize)
        secs.append(dict(name=name, type=typ, addr=addr, off=off, size=size, link=link, entsize=entsize))
    strtab = secs[shstrndx]
    for s in secs:
        end = elf.index(b"\0", strtab["off"] + s["name"])
        s["name"] = elf[strtab["off"] + s["name"]:end].decode()
    return secs


def _section_bytes(elf, name):
    s = next(s for s in _sections(elf) if s["name"] == name)
    return elf[s["off"]:s["off"] + s["size"]]


_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def _gfx950_code_objects(lib):
    """every gfx950 code object of every offload bundle (one bundle per translation unit)"""
    fb = _section_bytes(lib, ".hip_fatbin")
    assert fb[:24] == _MAGIC
    cos = []
    base = fb.find(_MAGIC)
    while base >= 0:
        n, = struct.unpack_from("<Q", fb, base + 24)
        p = end = base + 32
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", fb, p)
            p += 24
            triple = fb[p:p + tl].decode()
            p += tl
            end = max(end, p, base + off + size)
            if triple.endswith("gfx950") and size:
                cos.append(fb[base + off:base + off + size])
        base = fb.find(_MAGIC, end)  # the next bundle starts after this one's last entry
    assert cos, "no gfx950 code object in the library"
    return cos


def code_object_kernels(co):
    """{kernel symbol: (VGPRs allocated per lane, function symbol size)} of one code object"""
    secs = _sections(co)
    symtab = next(s for s in secs if s["type"] == 2)  # SHT_SYMTAB
    strtab = secs[symtab["link"]]
    syms = {}
    for k in range(symtab["size"] // symtab["entsize"]):
        name, info, other, shndx, value, size = struct.unpack_from("<IBBHQQ", co, symtab["off"] + k * symtab["entsize"])
        end = co.index(b"\0", strtab["off"] + name)
        syms[co[strtab["off"] + name:end].decode()] = (shndx, value, size)
    out = {}
    for sym, (shndx, value, _) in syms.items():
        if not sym.endswith(".kd"):
            continue
        sec = secs[shndx]
        kd = co[sec["off"] + value - sec["addr"]:][:64]
        rsrc1, = struct.unpack_from("<I", kd, 48)
        out[sym[:-3]] = (((rsrc1 & 0x3F) + 1) * 8, syms[sym[:-3]][2])
    return out


def library_kernels(path=LIB):
    """{kernel symbol: (VGPRs, function size)} over all gfx950 code objects of
    the library, and the number of kernels in each code object"""
    merged, counts = {}, []
    for co in _gfx950_code_objects(open(path, "rb").read()):
        kernels = code_object_kernels(co)
        for k, v in kernels.items():
            # a template launched from two translation units is compiled in both, to the same code
            assert merged.setdefault(k, v) == v, f"{k} differs between code objects: {merged[k]} vs {v}"
        counts.append(len(kernels))
    return merged, counts


@pytest.mark.skipif(not os.path.exists(LIB), reason="library not built")
def test_every_kernel_allocates_at_least_64_vgprs():
    kernels, counts = library_kernels()
    alloc = {k: v[0] for k, v in kernels.items()}
    assert len(alloc) > 50, "kernel descriptors not found"
    assert any("k_tensor2" in k for k in alloc) and any("k_eltwise" in k for k in alloc)
    # every translation unit with kernels is read, not only the first bundle
    assert any("k_ks_inner" in k for k in alloc), f"keyswitch.hip's kernels not read ({counts})"
    assert any("k_scale_round" in k for k in alloc), f"bfv_kernels.hpp's kernels not read ({counts})"
    low = {k: v for k, v in alloc.items() if v < 64}
    assert not low, f"kernels below the 64-VGPR floor: {low}"
