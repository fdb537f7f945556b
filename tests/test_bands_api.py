"""trx_grid_quantiles (the column quantiles behind target.fit_bands) is part of the C ABI at every layer -- header, Python
binding, exports of the built library -- and its kernel keeps out of scratch memory.  No GPU needed."""
import os
import re
import subprocess

import pytest

from test_build_resources import READELF, _device_objects

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "trx_grid_quantiles"


def test_grid_quantiles_is_declared_bound_and_exported():
    import __graft_entry__ as g
    from triceratops_amd import _lib
    header = open(os.path.join(ROOT, "include", "trx.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"int\s+%s\s*\(([^)]*)\)" % NAME, header)
    assert m, "%s is not declared in include/trx.h" % NAME
    params = [p.split()[-1].lstrip("*") for p in m.group(1).split(",")]
    assert params == ["grid", "n_grid_rows", "n_cols", "rows", "scale", "n_rows", "q", "n_q", "out", "stream"]
    assert NAME in _lib.ABI_SYMBOLS
    lib_path = g.build()
    out = subprocess.run(["nm", "-D", "--defined-only", lib_path], capture_output=True, text=True, check=True).stdout
    assert NAME in [ln.split()[-1] for ln in out.splitlines() if " T " in ln]
    L = _lib.lib()
    assert len(L.trx_grid_quantiles.argtypes) == len(params)
    assert callable(_lib.grid_quantiles) and os.path.join(ROOT, "triceratops_amd", "csrc", "trx_bands.hpp") in g.DEPS


def test_argument_checks_come_before_any_device_work():
    """(a CPU-only box: a call that got past its checks would fail with a HIP error, not TRX_ERR_ARG)"""
    import ctypes
    from triceratops_amd import _lib
    L = _lib.lib()
    q = (ctypes.c_double * 1)(0.5)
    assert L.trx_grid_quantiles(None, 4, 4, None, None, 4, q, 1, None, None) == 1
    assert b"null pointer" in L.trx_last_error()


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not installed")
def test_band_kernels_use_no_scratch(tmp_path):
    import __graft_entry__ as g
    from triceratops_amd import _lib
    g.build()
    seen = 0
    for path in (_lib.LIB_PATH, _lib.TESTING_LIB_PATH):
        objs = _device_objects(path)
        assert objs, "no gfx950 code object in %s" % path
        for k, obj in enumerate(objs):
            f = tmp_path / ("dev%d.co" % k)
            f.write_bytes(obj)
            notes = subprocess.run([READELF, "--notes", str(f)], capture_output=True, text=True, check=True).stdout
            for m in re.finditer(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n", notes):
                name, scratch = m.group(1), int(m.group(2))
                if "band_" in name:
                    seen += 1
                    assert scratch == 0, "%s uses %d B of scratch per lane" % (name, scratch)
    assert seen >= 2, "band_quantile_kernel is in neither library"
