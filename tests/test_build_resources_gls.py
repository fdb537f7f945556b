"""Register / scratch budget of scan_rows_kernel<ONE, OuColsFilter<K>> (trxg_chi2_grid_ou_baseline),
read from the code object's notes (test_build_resources.kernel_resources; no GPU needed).

Eight instantiations, ONE = false / true times K = 1 .. 4 columns.  Next to the OU filter's registers a lane holds the
pair of every column and, per row in flight, K further sums: none may reach scratch memory; K <= 2 may not need more than
128 VGPRs -- four waves a SIMD, what the OU filter has --, K = 3, 4 not more than 256.  The entry caps its grid at what
is resident: 4 blocks a CU below kGlsWideFrom columns, 2 from there on (trx_gls.hpp, scan_rows_launch).  That constant is
held against the counts read here: an instantiation is within 128 VGPRs exactly when its K lies below it.  As built:
66 / 82 / 98 / 114 VGPRs (ONE) and 70 / 78 / 86 / 95 (trips) at K = 1 .. 4 against the OU filter's 62, so kGlsWideFrom = 5.

The kernels are selected by the skeleton's and the filter's full names behind their length in the mangled name: no other
kernel's name can hold "16scan_rows_kernel" together with "12OuColsFilter", so the guard against the substrings by which the
other resource tests count their kernels is gone."""
import os
import re

import pytest

from test_build_resources import READELF, instantiations, kernel_resources
from triceratops_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _wide_from():
    text = open(os.path.join(ROOT, "triceratops_amd", "csrc", "trx_gls.hpp")).read()
    m = re.search(r"constexpr int kGlsWideFrom = (\d+);", text)
    assert m, "kGlsWideFrom not found in trx_gls.hpp"
    launcher = open(os.path.join(ROOT, "triceratops_amd", "csrc", "trx_kernels.hip")).read()
    assert "K < kGlsWideFrom ? 4 : 2" in launcher and "blocks > 256L * blocks_per_cu" in launcher, \
        "the resident cap of trxg_chi2_grid_ou_baseline has changed: update this test"
    return int(m.group(1))


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not installed")
def test_gls_ou_kernel_eight_instantiations_no_scratch_and_the_launchers_cap():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libtrx.so not built")
    seen = instantiations(kernel_resources(_lib.LIB_PATH), "scan_rows_kernel", "OuColsFilter")
    for name in sorted(seen):
        print("%s: %d VGPRs, %d SGPRs, scratch %d B, %d B of static LDS" % ((name,) + seen[name]))
    assert len(seen) == 8, sorted(seen)
    wide_from = _wide_from()
    print("kGlsWideFrom = %d" % wide_from)
    for one in (0, 1):
        for k in (1, 2, 3, 4):
            names = [name for name in seen if "ILb%dENS_12OuColsFilterILi%dEEEE" % (one, k) in name]
            assert len(names) == 1, (one, k, sorted(seen))
            vgprs, _, scratch, lds = seen[names[0]]
            assert scratch == 0, "%s uses %d B of scratch per lane" % (names[0], scratch)
            assert lds == 0, "%s uses %d B of LDS" % (names[0], lds)
            assert vgprs <= (128 if k <= 2 else 256), "%s needs %d VGPRs" % (names[0], vgprs)
            # the launcher's cap is the residency of this count: 4 blocks a CU up to 128 VGPRs, 2 beyond
            assert (vgprs <= 128) == (k < wide_from), "K = %d: %d VGPRs against kGlsWideFrom = %d" % (k, vgprs, wide_from)
