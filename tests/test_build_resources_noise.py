"""Register / scratch budget of chi2_ou_kernel<ONE> (trxn_chi2_grid_ou), read from the code object's
notes as tests/test_build_resources_baseline.py reads its kernel (no GPU needed).

The kernel keeps a trip's tables -- eight values of the stamps and the seven products of the scan -- and two rows' state in
registers: two instantiations (ONE: a row is a single trip and the tables are formed once per wave; the other: once per
trip), neither with scratch memory -- a local array indexed at run time would go there -- and neither above 128 VGPRs."""
import os
import re
import subprocess

import pytest

from test_build_resources import READELF, _device_objects
from triceratops_amd import _lib


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not installed")
def test_ou_reduction_kernel_two_instantiations_no_scratch_128_vgprs(tmp_path):
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
            if "chi2_ou_kernel" in name:
                seen[name] = (scratch, vgprs)
    print("chi2_ou_kernel (scratch B, VGPRs):", sorted(seen.items()))
    assert len(seen) == 2, sorted(seen)
    assert sorted("ILb1E" in name for name in seen) == [False, True], sorted(seen)          # <false> and <true>
    for name, (scratch, vgprs) in seen.items():
        assert scratch == 0, "%s uses %d B of scratch per lane" % (name, scratch)
        assert vgprs <= 128, "%s needs %d VGPRs" % (name, vgprs)
