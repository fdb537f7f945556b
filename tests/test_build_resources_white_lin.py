"""Register / scratch budget of chi2_white_lin_kernel<STAGE, J, K> (trxb_chi2_grid_white_baseline), read
from the code object's notes (test_build_resources.kernel_resources; no GPU needed).

Sixty-four instantiations: J = 1 .. 8 candidates, K = 1 .. 4 columns, STAGE (flux, the J weight vectors and the K columns
staged in LDS) and the other (read through the caches).  The J (1 + K) sums of a row -- of two rows up to 10 sums -- are
local arrays indexed by unrolled loops and folded across the lanes in registers: none may reach scratch memory.  The
launcher's cap of resident blocks (trx_white_lin.hpp, wlin_vgpr_bound; _lib.white_lin_blocks) counts on at most 128 VGPRs
up to 24 sums -- four waves a SIMD --, at most 168 up to 35 -- three -- and at most 256 at 40 -- two.  The LDS is dynamic: none of
it is static.

As built (VGPRs, STAGE / !STAGE):
   J        1      2      3       4        5        6        7        8
   K = 1  42/38  60/56   76/73   93/89  111/107   79/81    87/89    95/97
   K = 2  52/50  78/72   95/93   82/83   87/91    95/99  105/109  119/119
   K = 3  66/64  94/90   84/88   98/99  105/109  117/121  129/133  145/145
   K = 4  82/80 116/111 100/104 118/117 127/131  141/145  155/159  175/173"""
import os
import re

import pytest

from test_build_resources import READELF, instantiations, kernel_resources
from triceratops_amd import _lib


def _table(path):
    seen = instantiations(kernel_resources(path), "chi2_white_lin_kernel")
    out = {}
    for name, res in seen.items():
        m = re.search(r"ILb(\d)ELi(\d)ELi(\d)EE", name)
        assert m, name
        key = tuple(int(v) for v in m.groups())
        assert key not in out, name
        out[key] = res
    return out


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not installed")
def test_chi2_white_lin_kernel_sixty_four_instantiations_no_scratch_within_the_launchers_bound():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libtrx.so not built")
    table = _table(_lib.LIB_PATH)
    for key in sorted(table):
        print("STAGE %d J %d K %d: %d VGPRs, %d SGPRs, scratch %d B, %d B of static LDS" % (key + table[key]))
    # exactly what the dispatch creates: <false | true, J, K>, J = 1 .. 8, K = 1 .. 4
    assert sorted(table) == [(s, j, k) for s in (0, 1) for j in range(1, 9) for k in range(1, 5)]
    for (stage, j, k), (vgprs, _, scratch, lds) in table.items():
        assert scratch == 0, "<%d, %d, %d> uses %d B of scratch per lane" % (stage, j, k, scratch)
        assert lds == 0, "<%d, %d, %d> has %d B of static LDS" % (stage, j, k, lds)
        bound = 128 if j * (1 + k) <= 24 else 168 if j * (1 + k) <= 35 else 256
        assert vgprs <= bound, "<%d, %d, %d> needs %d VGPRs (the launcher's cap assumes %d)" % (stage, j, k, vgprs, bound)
        # the cap of blocks a CU is what that bound leaves resident
        assert _lib.white_lin_blocks(10 ** 6, 4096, j, k) == 256 * (512 // bound)


def test_the_bound_is_the_one_in_the_source():
    text = open(os.path.join(os.path.dirname(_lib.__file__), "csrc", "trx_white_lin.hpp")).read()
    assert re.search(r"kWlinFourWaveSums = 24;", text) and re.search(r"kWlinThreeWaveSums = 35;", text)
    assert re.search(r"kWlinTwoRowSums = 10;", text)
    assert "j * (1 + k) <= kWlinFourWaveSums ? 128 : j * (1 + k) <= kWlinThreeWaveSums ? 168 : 256" in text


def test_both_libraries_hold_the_same_instantiations():
    if not (os.path.exists(READELF) and os.path.exists(_lib.LIB_PATH) and os.path.exists(_lib.TESTING_LIB_PATH)):
        pytest.skip("libraries or llvm-readelf missing")
    a, b = _table(_lib.LIB_PATH), _table(_lib.TESTING_LIB_PATH)
    assert sorted(a) == sorted(b) and len(a) == 64
