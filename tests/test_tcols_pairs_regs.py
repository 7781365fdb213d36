"""The two-columns-per-thread forward column pass (k_tcols<false, SPQ, false,
16, 2>) sends its two column sets through the one-set tile one after the
other, so it keeps that kernel's 34 816 bytes of LDS and four workgroups per
CU: at most 128 VGPRs and no scratch.  The inverse pass, N = 2^17 and the
lifted forward pass keep one column per thread.  Read from the kernel
descriptors of the built library -- no GPU needed."""
import os
import re

import pytest

from test_block_octets_regs import _descriptors
from test_vgpr_floor import LIB, _gfx950_code_objects

# k_tcols<INV, SPQ, SWS, LOGN, CPT>
NAME = r"7k_tcolsILb([01])ELb([01])ELb([01])ELi(\d+)ELi(\d+)EEE"


@pytest.mark.skipif(not os.path.exists(LIB), reason="library not built")
def test_column_pair_kernels_fit_four_workgroups_per_cu():
    kernels = {}
    for co in _gfx950_code_objects(open(LIB, "rb").read()):
        kernels.update(_descriptors(co))
    tcols = {}
    for k, v in kernels.items():
        m = re.search(NAME, k)
        if m:
            tcols[tuple(int(x) for x in m.groups())] = v
    names = sorted(tcols)
    # the forward pass ships with two columns per thread, special primes and generic moduli
    pairs = {k: v for k, v in tcols.items() if k[4] == 2}
    assert sorted(pairs) == [(0, spq, 0, 16, 2) for spq in (0, 1)], names
    for k, (vgprs, scratch, lds) in pairs.items():
        assert scratch == 0, (k, scratch)
        assert lds == 34816, (k, lds)
        assert vgprs <= 128, (k, vgprs)
    # one column per thread: N = 2^17 (the 8 | 9 split), the fallback and the inverse at 2^16,
    # the lift (forward only) at both sizes
    for logn in (16, 17):
        for spq in (0, 1):
            assert (0, spq, 0, logn, 1) in tcols and (1, spq, 0, logn, 1) in tcols, names
            assert (0, spq, 1, logn, 1) in tcols, names
