"""Register / scratch budget of chi2_rows_kernel<STAGE, Terms> (trx_chi2_grid_weighted, trx_chi2_grid_offset,
trx_chi2_grid_baseline), read from the code object's notes as tests/test_build_resources.py reads
them (no GPU needed).

The kernel keeps one accumulator per sum and row in registers, their number a template argument of the Terms policy:
twelve instantiations (STAGE x Chi2Plain, Chi2Offset, Chi2Baseline<K = 1 .. 4>), none with scratch memory -- a local array
indexed at run time would go there -- and none above 128 VGPRs."""
import os
import re
import subprocess

import pytest

from test_build_resources import READELF, _device_objects
from triceratops_amd import _lib


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not installed")
def test_row_reduction_kernels_twelve_instantiations_no_scratch_128_vgprs(tmp_path):
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libtrx.so not built")
    objs = _device_objects(_lib.LIB_PATH)
    assert objs, "no gfx950 code object in libtrx.so"
    seen = {}
    for k, obj in enumerate(objs):
        f = tmp_path / ("dev%d.co" % k)
        f.write_bytes(obj)
        notes = subprocess.run([READELF, "--notes", str(f)], capture_output=True, text=True, check=True).stdout
        for m in re.finditer(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)", notes):
            name, scratch, vgprs = m.group(1), int(m.group(2)), int(m.group(3))
            if "chi2_rows_kernel" in name:
                seen[name] = (scratch, vgprs)
    print("chi2_rows_kernel (scratch B, VGPRs):", sorted(seen.items()))
    assert len(seen) == 12, sorted(seen)
    per_policy = {p: sum(p in name for name in seen) for p in ("Chi2Plain", "Chi2Offset", "Chi2Baseline")}
    assert per_policy == {"Chi2Plain": 2, "Chi2Offset": 2, "Chi2Baseline": 8}, sorted(seen)
    for name, (scratch, vgprs) in seen.items():
        assert scratch == 0, "%s uses %d B of scratch per lane" % (name, scratch)
        assert vgprs <= 128, "%s needs %d VGPRs" % (name, vgprs)
