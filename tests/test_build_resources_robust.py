"""Register / scratch budget of chi2_robust_kernel<STAGE> (trxr_chi2_grid_robust), read from the code
object's notes as tests/test_build_resources_shift.py reads softmin_rows_kernel's (no GPU needed).

Two instantiations, STAGE = false and true.  Every value costs one inlined exp and one inlined log1p, two rows are in flight
per wave: neither instantiation may reach scratch memory, and neither may need more than 128 VGPRs -- four waves a SIMD of the
512-register file, the least that keeps the VALU port busy while a wave waits for its loads."""
import os
import re
import subprocess

import pytest

from test_build_resources import READELF, _device_objects
from triceratops_amd import _lib


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not installed")
def test_chi2_robust_kernel_two_instantiations_no_scratch_128_vgprs(tmp_path):
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
            if "chi2_robust_kernel" in name:
                seen[name] = (scratch, vgprs, lds)
    for name in sorted(seen):
        print("%s: scratch %d B, %d VGPRs, %d B of static LDS" % ((name,) + seen[name]))
    assert len(seen) == 2, sorted(seen)
    for stage in (0, 1):
        assert sum("ILb%dEE" % stage in name for name in seen) == 1, (stage, sorted(seen))
    for name, (scratch, vgprs, _) in seen.items():
        assert scratch == 0, "%s uses %d B of scratch per lane" % (name, scratch)
        assert vgprs <= 128, "%s needs %d VGPRs" % (name, vgprs)
