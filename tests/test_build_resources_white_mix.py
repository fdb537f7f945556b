"""Register / scratch budget of chi2_white_mix_kernel<STAGE, J> (trxv_chi2_grid_white_mix), read from
the code object's notes (test_build_resources.kernel_resources; no GPU needed).

Sixteen instantiations: J = 1 .. 8 candidates, STAGE (flux and the J weight vectors staged in LDS) and the other (read
through the caches).  The per-candidate sums of two rows are local arrays indexed by unrolled loops: none may reach scratch
memory, and none may need more than 128 VGPRs -- four waves a SIMD, the eight blocks a CU that the launcher's cap counts
on.  The LDS is dynamic: none of it is static."""
import os

import pytest

from test_build_resources import READELF, instantiations, kernel_resources
from triceratops_amd import _lib


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not installed")
def test_chi2_white_mix_kernel_sixteen_instantiations_no_scratch_128_vgprs():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libtrx.so not built")
    seen = instantiations(kernel_resources(_lib.LIB_PATH), "chi2_white_mix_kernel")
    for name in sorted(seen):
        print("%s: %d VGPRs, %d SGPRs, scratch %d B, %d B of static LDS" % ((name,) + seen[name]))
    # exactly what the dispatch creates: <false, J> and <true, J>, J = 1 .. 8
    assert len(seen) == 16, sorted(seen)
    for stage in (0, 1):
        for j in range(1, 9):
            assert sum("ILb%dELi%dEE" % (stage, j) in name for name in seen) == 1, (stage, j, sorted(seen))
    for name, (vgprs, _, scratch, lds) in seen.items():
        assert scratch == 0, "%s uses %d B of scratch per lane" % (name, scratch)
        assert vgprs <= 128, "%s needs %d VGPRs" % (name, vgprs)
        assert lds == 0, "%s has %d B of static LDS" % (name, lds)


def test_both_libraries_hold_the_same_instantiations():
    if not (os.path.exists(READELF) and os.path.exists(_lib.LIB_PATH) and os.path.exists(_lib.TESTING_LIB_PATH)):
        pytest.skip("libraries or llvm-readelf missing")
    a = instantiations(kernel_resources(_lib.LIB_PATH), "chi2_white_mix_kernel")
    b = instantiations(kernel_resources(_lib.TESTING_LIB_PATH), "chi2_white_mix_kernel")
    assert sorted(a) == sorted(b) and len(a) == 16
