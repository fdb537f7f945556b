"""Register / scratch budget of scan_rows_kernel<ONE, OuFilter> (trxn_chi2_grid_ou), read from the
code object's notes (test_build_resources.kernel_resources; no GPU needed).

The kernel keeps a trip's tables -- eight values of the stamps and the seven products of the scan -- and two rows' state in
registers: two instantiations (ONE: a row is a single trip and the tables are formed once per wave; the other: once per
trip), neither with scratch memory -- a local array indexed at run time would go there -- and neither above 128 VGPRs."""
import os

import pytest

from test_build_resources import READELF, instantiations, kernel_resources
from triceratops_amd import _lib


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not installed")
def test_ou_reduction_kernel_two_instantiations_no_scratch_128_vgprs():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libtrx.so not built")
    seen = instantiations(kernel_resources(_lib.LIB_PATH), "scan_rows_kernel", "OuFilter")
    print("scan_rows_kernel<ONE, OuFilter> (VGPRs, SGPRs, scratch B, LDS B):", sorted(seen.items()))
    assert len(seen) == 2, sorted(seen)
    assert sorted("ILb1E" in name for name in seen) == [False, True], sorted(seen)          # <false> and <true>
    for name, (vgprs, _, scratch, lds) in seen.items():
        assert scratch == 0, "%s uses %d B of scratch per lane" % (name, scratch)
        assert lds == 0, "%s uses %d B of LDS" % (name, lds)
        assert vgprs <= 128, "%s needs %d VGPRs" % (name, vgprs)
