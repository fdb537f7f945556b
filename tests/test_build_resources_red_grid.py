"""Register / scratch budget of ou_mix_kernel<ONE, J> (trxm_chi2_grid_ou_mix), read from the code
object's notes (test_build_resources.kernel_resources; no GPU needed).

Sixteen instantiations: J = 1 .. 8 candidates, ONE (a row is a single trip; the candidates' trip tables in registers up
to J = 4, in LDS past that) and the other (formed per trip).  The per-candidate carry / acc of two rows are local arrays
indexed by unrolled loops: none may reach scratch memory, and none may need more than 256 VGPRs -- two waves a SIMD, which
with two rows a wave is what hides the load latency."""
import os

import pytest

from test_build_resources import READELF, instantiations, kernel_resources
from triceratops_amd import _lib


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not installed")
def test_ou_mix_kernel_sixteen_instantiations_no_scratch_256_vgprs():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libtrx.so not built")
    seen = instantiations(kernel_resources(_lib.LIB_PATH), "ou_mix_kernel")
    for name in sorted(seen):
        print("%s: %d VGPRs, %d SGPRs, scratch %d B, %d B of LDS" % ((name,) + seen[name]))
    assert len(seen) == 16, sorted(seen)
    # <false, J> and <true, J>, J = 1 .. 8
    for one in (0, 1):
        for j in range(1, 9):
            assert sum("ILb%dELi%dEE" % (one, j) in name for name in seen) == 1, (one, j, sorted(seen))
    # (J <= 2 is launched four blocks a CU -- four waves a SIMD --, as the OU filter's kernel is)
    assert all(seen[name][0] <= 128 for name in seen if "ELi1EE" in name or "ELi2EE" in name)
    for name, (vgprs, _, scratch, lds) in seen.items():
        assert scratch == 0, "%s uses %d B of scratch per lane" % (name, scratch)
        assert vgprs <= 256, "%s needs %d VGPRs" % (name, vgprs)
        assert lds <= 64 << 10, "%s needs %d B of LDS" % (name, lds)
    assert "scan_rows_kernel" not in "".join(seen)
