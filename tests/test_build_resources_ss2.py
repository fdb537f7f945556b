"""Register / scratch budget of ss2_kernel<ONE> (trxs_chi2_grid_ss2), read from the code object's
notes as tests/test_build_resources_noise.py reads chi2_ou_kernel's (no GPU needed).

The kernel keeps a trip's tables in registers -- four values of the stamps, seven of the lane's own pair and the seven 2 x 2
products of the scan, 39 doubles -- next to two rows' state: two instantiations (ONE: a row is a single trip and the tables
are formed once per wave; the other: once per trip), neither with scratch memory -- a local array indexed at run time
would go there.  The ceiling is 128 VGPRs, the step at which four waves a SIMD are resident (512 registers a lane and
SIMD): the kernel has no LDS, so the registers alone decide the residency, ss2_launch caps the grid at the four blocks of
256 threads a CU that this step admits -- as chi2_ou_launch does --, and with two rows a wave in flight four waves are what
keeps the grid's loads ahead of the scan.  One step down (three waves at up to 168 VGPRs) the capped grid would no longer be
resident at once."""
import os
import re
import subprocess

import pytest

from test_build_resources import READELF, _device_objects
from triceratops_amd import _lib

VGPR_CEILING = 128           # four waves a SIMD


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not installed")
def test_ss2_kernel_two_instantiations_no_scratch_128_vgprs(tmp_path):
    assert VGPR_CEILING <= 256
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
            if "ss2_kernel" in name:
                seen[name] = (scratch, vgprs)
    print("ss2_kernel (scratch B, VGPRs):", sorted(seen.items()))
    assert len(seen) == 2, sorted(seen)
    assert sorted("ILb1E" in name for name in seen) == [False, True], sorted(seen)          # <false> and <true>
    for name, (scratch, vgprs) in seen.items():
        assert scratch == 0, "%s uses %d B of scratch per lane" % (name, scratch)
        assert vgprs <= VGPR_CEILING, "%s needs %d VGPRs" % (name, vgprs)
