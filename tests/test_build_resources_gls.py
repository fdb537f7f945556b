"""Register / scratch budget of gls_ou_kernel<ONE, K> (trxg_chi2_grid_ou_baseline), read from the code
object's notes as tests/test_build_resources_red_grid.py reads ou_mix_kernel's (no GPU needed).

Eight instantiations, ONE = false / true times K = 1 .. 4 columns.  Next to chi2_ou_kernel's registers a lane holds the
pair of every column and, per row in flight, K further sums: none may reach scratch memory; K <= 2 may not need more than
128 VGPRs -- four waves a SIMD, what chi2_ou_kernel has --, K = 3, 4 not more than 256.  The launcher caps its grid at what
is resident: 4 blocks a CU below kGlsWideFrom columns, 2 from there on (trx_gls.hpp, gls_ou_launch).  That constant is
held against the counts read here: an instantiation is within 128 VGPRs exactly when its K lies below it.  As built:
66 / 82 / 98 / 114 VGPRs (ONE) and 70 / 78 / 86 / 95 (trips) at K = 1 .. 4 against chi2_ou_kernel's 62, so kGlsWideFrom = 5."""
import os
import re
import subprocess

import pytest

from test_build_resources import READELF, _device_objects
from triceratops_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _wide_from():
    text = open(os.path.join(ROOT, "triceratops_amd", "csrc", "trx_gls.hpp")).read()
    m = re.search(r"constexpr int kGlsWideFrom = (\d+);", text)
    assert m, "kGlsWideFrom not found in trx_gls.hpp"
    launcher = open(os.path.join(ROOT, "triceratops_amd", "csrc", "trx_kernels.hip")).read()
    assert "256L * (K < kGlsWideFrom ? 4 : 2)" in launcher, "gls_ou_launch's resident cap has changed: update this test"
    return int(m.group(1))


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not installed")
def test_gls_ou_kernel_eight_instantiations_no_scratch_and_the_launchers_cap(tmp_path):
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libtrx.so not built")
    objs = _device_objects(_lib.LIB_PATH)
    assert objs, "no gfx950 code object in libtrx.so"
    seen = {}
    for k, obj in enumerate(objs):
        f = tmp_path / ("dev%d.co" % k)
        f.write_bytes(obj)
        notes = subprocess.run([READELF, "--notes", str(f)], capture_output=True, text=True, check=True).stdout
        for m in re.finditer(r"\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.name:\s+(\S+)\n(?:.*\n)*?"
                             r"\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)", notes):
            lds, name, scratch, vgprs = int(m.group(1)), m.group(2), int(m.group(3)), int(m.group(4))
            if "gls_ou_kernel" in name:
                seen[name] = (scratch, vgprs, lds)
    for name in sorted(seen):
        print("%s: scratch %d B, %d VGPRs, %d B of static LDS" % ((name,) + seen[name]))
    assert len(seen) == 8, sorted(seen)
    # the existing resource tests count their kernels by these substrings: none may occur in a name here
    for name in seen:
        for other in ("chi2_ou_kernel", "ou_mix_kernel", "chi2_rows_kernel", "chi2_robust_kernel", "softmin_rows_kernel",
                      "Chi2Plain", "Chi2Offset", "Chi2Baseline"):
            assert other not in name, (other, name)
    wide_from = _wide_from()
    print("kGlsWideFrom = %d" % wide_from)
    for one in (0, 1):
        for k in (1, 2, 3, 4):
            names = [name for name in seen if "ILb%dELi%dEE" % (one, k) in name]
            assert len(names) == 1, (one, k, sorted(seen))
            scratch, vgprs, lds = seen[names[0]]
            assert scratch == 0, "%s uses %d B of scratch per lane" % (names[0], scratch)
            assert lds == 0, "%s uses %d B of LDS" % (names[0], lds)
            assert vgprs <= (128 if k <= 2 else 256), "%s needs %d VGPRs" % (names[0], vgprs)
            # the launcher's cap is the residency of this count: 4 blocks a CU up to 128 VGPRs, 2 beyond
            assert (vgprs <= 128) == (k < wide_from), "K = %d: %d VGPRs against kGlsWideFrom = %d" % (k, vgprs, wide_from)
