"""Register / scratch budget of ou_mix_kernel<ONE, J> (trxm_chi2_grid_ou_mix), read from the code
object's notes as tests/test_build_resources_noise.py reads chi2_ou_kernel's (no GPU needed).

Sixteen instantiations: J = 1 .. 8 candidates, ONE (a row is a single trip; the candidates' trip tables in registers up
to J = 4, in LDS past that) and the other (formed per trip).  The per-candidate carry / acc of two rows are local arrays
indexed by unrolled loops: none may reach scratch memory, and none may need more than 256 VGPRs -- two waves a SIMD, which
with two rows a wave is what hides the load latency."""
import os
import re
import subprocess

import pytest

from test_build_resources import READELF, _device_objects
from triceratops_amd import _lib


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not installed")
def test_ou_mix_kernel_sixteen_instantiations_no_scratch_256_vgprs(tmp_path):
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
            if "ou_mix_kernel" in name:
                seen[name] = (scratch, vgprs, lds)
    for name in sorted(seen):
        print("%s: scratch %d B, %d VGPRs, %d B of LDS" % ((name,) + seen[name]))
    assert len(seen) == 16, sorted(seen)
    # <false, J> and <true, J>, J = 1 .. 8
    for one in (0, 1):
        for j in range(1, 9):
            assert sum("ILb%dELi%dEE" % (one, j) in name for name in seen) == 1, (one, j, sorted(seen))
    # (J <= 2 is launched four blocks a CU -- four waves a SIMD --, as chi2_ou_kernel is)
    assert all(seen[name][1] <= 128 for name in seen if "ELi1EE" in name or "ELi2EE" in name)
    for name, (scratch, vgprs, lds) in seen.items():
        assert scratch == 0, "%s uses %d B of scratch per lane" % (name, scratch)
        assert vgprs <= 256, "%s needs %d VGPRs" % (name, vgprs)
        assert lds <= 64 << 10, "%s needs %d B of LDS" % (name, lds)
    assert "chi2_ou_kernel" not in "".join(seen)
