"""The two-quad fused block pass (k_block<MODE_FUSED, SPQ, NR = 2, SK = 0, QP = 2>)
fits three workgroups per CU: at most 168 VGPRs, no scratch, and the one-set
kernel's 34 816 bytes of LDS.  Its register allocation is tight (the number of
early Hadamard-operand loads and the twist's fetch groups were chosen for it,
csrc/ntt_kernels.hpp block_body_q2), so a change that makes it spill should
fail here, on the build host, and not show up as a slower benchmark.  Read from
the kernel descriptors of the built library -- no GPU needed."""
import os
import re
import struct

import pytest

from test_vgpr_floor import LIB, _gfx950_code_objects, _sections


def _descriptors(co):
    """{kernel symbol: (VGPRs, scratch bytes, LDS bytes)} of one code object"""
    secs = _sections(co)
    symtab = next(s for s in secs if s["type"] == 2)  # SHT_SYMTAB
    strtab = secs[symtab["link"]]
    out = {}
    for k in range(symtab["size"] // symtab["entsize"]):
        name, _, _, shndx, value, _ = struct.unpack_from("<IBBHQQ", co, symtab["off"] + k * symtab["entsize"])
        end = co.index(b"\0", strtab["off"] + name)
        sym = co[strtab["off"] + name:end].decode()
        if not sym.endswith(".kd"):
            continue
        sec = secs[shndx]
        kd = co[sec["off"] + value - sec["addr"]:][:64]
        lds, scratch = struct.unpack_from("<II", kd, 0)  # group / private segment fixed size
        rsrc1, = struct.unpack_from("<I", kd, 48)
        out[sym[:-3]] = (((rsrc1 & 0x3F) + 1) * 8, scratch, lds)
    return out


@pytest.mark.skipif(not os.path.exists(LIB), reason="library not built")
def test_two_quad_block_pass_fits_three_workgroups_per_cu():
    kernels = {}
    for co in _gfx950_code_objects(open(LIB, "rb").read()):
        kernels.update(_descriptors(co))
    # k_block<2 (MODE_FUSED), SPQ, 2, 0, 2>: special primes and generic moduli
    octets = {k: v for k, v in kernels.items() if re.search(r"7k_blockILi2ELb[01]ELi2ELi0ELi2EEE", k)}
    assert len(octets) == 2, sorted(k for k in kernels if "k_block" in k)
    one_set = [k for k in kernels if re.search(r"7k_blockILi2ELb[01]ELi2ELi0ELi1EEE", k)]
    assert len(one_set) == 2  # N = 2^17 keeps one quad per thread
    for k, (vgprs, scratch, lds) in octets.items():
        assert vgprs <= 168, (k, vgprs)
        assert scratch == 0, (k, scratch)
        assert lds == 34816, (k, lds)
