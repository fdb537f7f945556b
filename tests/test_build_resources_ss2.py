"""Register / scratch budget of scan_rows_kernel<ONE, Ss2Filter> (trxs_chi2_grid_ss2), read from the
code object's notes (test_build_resources.kernel_resources; no GPU needed).

The kernel keeps a trip's tables in registers -- four values of the stamps, seven of the lane's own pair and the seven 2 x 2
products of the scan, 39 doubles -- next to two rows' state: two instantiations (ONE: a row is a single trip and the tables
are formed once per wave; the other: once per trip), neither with scratch memory -- a local array indexed at run time
would go there.  The ceiling is 128 VGPRs, the step at which four waves a SIMD are resident (512 registers a lane and
SIMD): the kernel has no LDS, so the registers alone decide the residency, trxs_chi2_grid_ss2 caps the grid at the four
blocks of 256 threads a CU that this step admits -- as trxn_chi2_grid_ou does --, and with two rows a wave in flight four
waves are what keeps the grid's loads ahead of the scan.  One step down (three waves at up to 168 VGPRs) the capped grid
would no longer be resident at once."""
import os

import pytest

from test_build_resources import READELF, instantiations, kernel_resources
from triceratops_amd import _lib

VGPR_CEILING = 128           # four waves a SIMD


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not installed")
def test_ss2_kernel_two_instantiations_no_scratch_128_vgprs():
    assert VGPR_CEILING <= 256
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libtrx.so not built")
    seen = instantiations(kernel_resources(_lib.LIB_PATH), "scan_rows_kernel", "Ss2Filter")
    print("scan_rows_kernel<ONE, Ss2Filter> (VGPRs, SGPRs, scratch B, LDS B):", sorted(seen.items()))
    assert len(seen) == 2, sorted(seen)
    assert sorted("ILb1E" in name for name in seen) == [False, True], sorted(seen)          # <false> and <true>
    for name, (vgprs, _, scratch, lds) in seen.items():
        assert scratch == 0, "%s uses %d B of scratch per lane" % (name, scratch)
        assert lds == 0, "%s uses %d B of LDS" % (name, lds)
        assert vgprs <= VGPR_CEILING, "%s needs %d VGPRs" % (name, vgprs)
