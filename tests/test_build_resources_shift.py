"""Register / scratch budget of softmin_rows_kernel<J> (trxt_softmin_rows), read from the code object's
notes (test_build_resources.kernel_resources; no GPU needed).

Eight instantiations, J = 1 .. 8 nodes.  A lane holds its row's J values in a local array indexed by unrolled loops: none may
reach scratch memory, none may use LDS, and none may need more than 64 VGPRs -- eight waves a SIMD, which is what keeps enough
loads in flight for a pass that only streams."""
import os

import pytest

from test_build_resources import READELF, instantiations, kernel_resources
from triceratops_amd import _lib


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not installed")
def test_softmin_rows_kernel_eight_instantiations_no_scratch_no_lds_64_vgprs():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libtrx.so not built")
    seen = instantiations(kernel_resources(_lib.LIB_PATH), "softmin_rows_kernel")
    for name in sorted(seen):
        print("%s: %d VGPRs, %d SGPRs, scratch %d B, %d B of LDS" % ((name,) + seen[name]))
    assert len(seen) == 8, sorted(seen)
    for j in range(1, 9):
        assert sum("ILi%dEE" % j in name for name in seen) == 1, (j, sorted(seen))
    for name, (vgprs, _, scratch, lds) in seen.items():
        assert scratch == 0, "%s uses %d B of scratch per lane" % (name, scratch)
        assert vgprs <= 64, "%s needs %d VGPRs" % (name, vgprs)
        assert lds == 0, "%s uses %d B of LDS" % (name, lds)
