"""Register / scratch budget of chi2_rows_kernel<STAGE, Terms> (trx_chi2_grid_weighted, trx_chi2_grid_offset,
trx_chi2_grid_baseline), read from the code object's notes (test_build_resources.kernel_resources;
no GPU needed).

The kernel keeps one accumulator per sum and row in registers, their number a template argument of the Terms policy:
twelve instantiations (STAGE x Chi2Plain, Chi2Offset, Chi2Baseline<K = 1 .. 4>), none with scratch memory -- a local array
indexed at run time would go there -- and none above 128 VGPRs."""
import os

import pytest

from test_build_resources import READELF, instantiations, kernel_resources
from triceratops_amd import _lib


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not installed")
def test_row_reduction_kernels_twelve_instantiations_no_scratch_128_vgprs():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libtrx.so not built")
    seen = instantiations(kernel_resources(_lib.LIB_PATH), "chi2_rows_kernel")
    print("chi2_rows_kernel (VGPRs, SGPRs, scratch B, LDS B):", sorted(seen.items()))
    assert len(seen) == 12, sorted(seen)
    per_policy = {p: len(instantiations(seen, "chi2_rows_kernel", p)) for p in ("Chi2Plain", "Chi2Offset", "Chi2Baseline")}
    assert per_policy == {"Chi2Plain": 2, "Chi2Offset": 2, "Chi2Baseline": 8}, sorted(seen)
    for name, (vgprs, _, scratch, _) in seen.items():
        assert scratch == 0, "%s uses %d B of scratch per lane" % (name, scratch)
        assert vgprs <= 128, "%s needs %d VGPRs" % (name, vgprs)
