"""Register / scratch budget of softmin_rows_kernel<J> (trxt_softmin_rows), read from the code object's
notes as tests/test_build_resources_noise.py reads chi2_ou_kernel's (no GPU needed).

Eight instantiations, J = 1 .. 8 nodes.  A lane holds its row's J values in a local array indexed by unrolled loops: none may
reach scratch memory, none may use LDS, and none may need more than 64 VGPRs -- eight waves a SIMD, which is what keeps enough
loads in flight for a pass that only streams."""
import os
import re
import subprocess

import pytest

from test_build_resources import READELF, _device_objects
from triceratops_amd import _lib


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not installed")
def test_softmin_rows_kernel_eight_instantiations_no_scratch_no_lds_64_vgprs(tmp_path):
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
            if "softmin_rows_kernel" in name:
                seen[name] = (scratch, vgprs, lds)
    for name in sorted(seen):
        print("%s: scratch %d B, %d VGPRs, %d B of LDS" % ((name,) + seen[name]))
    assert len(seen) == 8, sorted(seen)
    for j in range(1, 9):
        assert sum("ILi%dEE" % j in name for name in seen) == 1, (j, sorted(seen))
    for name, (scratch, vgprs, lds) in seen.items():
        assert scratch == 0, "%s uses %d B of scratch per lane" % (name, scratch)
        assert vgprs <= 64, "%s needs %d VGPRs" % (name, vgprs)
        assert lds == 0, "%s uses %d B of LDS" % (name, lds)
