"""The two-columns-per-thread inverse column pass (k_tcols_inv2<SPQ>) sends its
two column sets through the one-set tile one after the other and fetches its
first round's per-lane twiddles at most four entries at a time, so the
kernel's own resources are those of the one-column kernel and would allow four
workgroups per CU: 34 816 bytes of LDS, at most 128 VGPRs and no scratch, for
special primes and for generic moduli.  (The launcher runs it at three per CU
by adding dynamic LDS, which the descriptor does not show.)  Read from the
kernel descriptors of the built library -- no GPU needed."""
import os
import re

import pytest

from test_block_octets_regs import _descriptors
from test_vgpr_floor import LIB, _gfx950_code_objects

# k_tcols_inv2<SPQ>
NAME = r"12k_tcols_inv2ILb([01])EEE"


@pytest.mark.skipif(not os.path.exists(LIB), reason="library not built")
def test_inverse_column_pair_kernels_fit_four_workgroups_per_cu():
    kernels = {}
    for co in _gfx950_code_objects(open(LIB, "rb").read()):
        kernels.update(_descriptors(co))
    pairs = {}
    for k, v in kernels.items():
        m = re.search(NAME, k)
        if m:
            pairs[int(m.group(1))] = v
    assert sorted(pairs) == [0, 1], sorted(kernels)
    for spq, (vgprs, scratch, lds) in pairs.items():
        assert scratch == 0, (spq, scratch)
        assert lds == 34816, (spq, lds)
        assert vgprs <= 128, (spq, vgprs)
