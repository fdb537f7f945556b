"""Register / scratch budget of chi2_robust_kernel<STAGE> (trxr_chi2_grid_robust), read from the code
object's notes (test_build_resources.kernel_resources; no GPU needed).

Two instantiations, STAGE = false and true.  Every value costs one inlined exp and one inlined log1p, two rows are in flight
per wave: neither instantiation may reach scratch memory, and neither may need more than 128 VGPRs -- four waves a SIMD of the
512-register file, the least that keeps the VALU port busy while a wave waits for its loads."""
import os

import pytest

from test_build_resources import READELF, instantiations, kernel_resources
from triceratops_amd import _lib


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not installed")
def test_chi2_robust_kernel_two_instantiations_no_scratch_128_vgprs():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libtrx.so not built")
    seen = instantiations(kernel_resources(_lib.LIB_PATH), "chi2_robust_kernel")
    for name in sorted(seen):
        print("%s: %d VGPRs, %d SGPRs, scratch %d B, %d B of static LDS" % ((name,) + seen[name]))
    assert len(seen) == 2, sorted(seen)
    for stage in (0, 1):
        assert sum("ILb%dEE" % stage in name for name in seen) == 1, (stage, sorted(seen))
    for name, (vgprs, _, scratch, _) in seen.items():
        assert scratch == 0, "%s uses %d B of scratch per lane" % (name, scratch)
        assert vgprs <= 128, "%s needs %d VGPRs" % (name, vgprs)
