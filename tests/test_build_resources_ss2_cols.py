"""Register / scratch budget of scan_rows_kernel<ONE, Ss2ColsFilter<K>> (trxk_chi2_grid_ss2_baseline),
read from the code object's notes (test_build_resources.kernel_resources; no GPU needed).

Eight instantiations, ONE = false / true times K = 1 .. 4 columns.  Next to the two-state filter's registers -- a trip's
tables are 39 doubles -- a lane holds the pair of every column and, per row in flight, K further sums: none may reach
scratch memory, none uses LDS.  The kernel has no LDS, so its registers alone decide what is resident, and the entry caps
its grid at that: kSs2ColsBlocksPerCu[ONE][K - 1] blocks of 256 threads a CU (trx_ss2_cols.hpp) -- 4 at up to 128 VGPRs, 3
at up to 168, 2 at up to 256 (512 registers a lane and SIMD, allotted in eights).  Every entry of that table is held
against the register count read here: the instantiation must fit the residency the table claims, and must not fit the
next one (a table that claims too little leaves a resident slot unused).  _lib.ss2_baseline_blocks mirrors the launcher.
As built: 130 / 138 / 146 / 155 VGPRs (trips) and 116 / 130 / 124 / 162 (ONE) at K = 1 .. 4 against the filter's own 120
and 112."""
import os
import re

import pytest

from test_build_resources import READELF, instantiations, kernel_resources
from triceratops_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CEILING = {4: 128, 3: 168, 2: 256}           # VGPRs at which that many waves a SIMD are resident


def _table():
    """kSs2ColsBlocksPerCu of trx_ss2_cols.hpp as [[trips: K = 1 .. 4], [ONE: K = 1 .. 4]]"""
    text = open(os.path.join(ROOT, "triceratops_amd", "csrc", "trx_ss2_cols.hpp")).read()
    m = re.search(r"constexpr int kSs2ColsBlocksPerCu\[2\]\[kChi2bMaxTerms\] = \{(.*?)\};", text, flags=re.S)
    assert m, "kSs2ColsBlocksPerCu not found in trx_ss2_cols.hpp"
    rows = re.findall(r"\{\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*\}", re.sub(r"//[^\n]*", "", m.group(1)))
    assert len(rows) == 2, rows
    assert "return kSs2ColsBlocksPerCu[one ? 1 : 0][k - 1];" in text
    launcher = open(os.path.join(ROOT, "triceratops_amd", "csrc", "trx_kernels.hip")).read()
    assert "ss2_cols_blocks_per_cu(n_time <= kOuTrip, K)" in launcher and "blocks > 256L * blocks_per_cu" in launcher, \
        "the resident cap of trxk_chi2_grid_ss2_baseline has changed: update this test"
    return [[int(v) for v in row] for row in rows]


def test_the_binding_mirrors_the_headers_table():
    table = _table()
    assert all(v in CEILING for row in table for v in row), table
    assert [list(row) for row in _lib.SS2_COLS_BLOCKS_PER_CU] == table
    for k in (1, 2, 3, 4):
        for n_time, one in ((1, 1), (k, 1), (127, 1), (128, 1), (129, 0), (2049, 0)):
            cap = 256 * table[one][k - 1]
            for n in (0, 1, 3, 4, 5, 4 * cap - 1, 4 * cap, 4 * cap + 1, 8 * cap + 3, 10 ** 7):
                assert _lib.ss2_baseline_blocks(n, n_time, k) == min((n + 3) // 4, cap), (n, n_time, k)


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not installed")
def test_ss2_cols_kernel_eight_instantiations_no_scratch_and_the_launchers_cap():
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libtrx.so not built")
    seen = instantiations(kernel_resources(_lib.LIB_PATH), "scan_rows_kernel", "Ss2ColsFilter")
    for name in sorted(seen):
        print("%s: %d VGPRs, %d SGPRs, scratch %d B, %d B of static LDS" % ((name,) + seen[name]))
    assert len(seen) == 8, sorted(seen)
    table = _table()
    print("kSs2ColsBlocksPerCu = %s" % table)
    for one in (0, 1):
        for k in (1, 2, 3, 4):
            names = [name for name in seen if "ILb%dENS_13Ss2ColsFilterILi%dEEEE" % (one, k) in name]
            assert len(names) == 1, (one, k, sorted(seen))
            vgprs, _, scratch, lds = seen[names[0]]
            assert scratch == 0, "%s uses %d B of scratch per lane" % (names[0], scratch)
            assert lds == 0, "%s uses %d B of LDS" % (names[0], lds)
            blocks = table[one][k - 1]
            assert vgprs <= CEILING[blocks], "%s needs %d VGPRs: %d blocks a CU are not resident" % (names[0], vgprs, blocks)
            assert blocks == 4 or vgprs > CEILING[blocks + 1], \
                "%s needs %d VGPRs: %d blocks a CU would be resident, the table says %d" % (names[0], vgprs, blocks + 1, blocks)
    # the plain two-state filter's instantiations are not these
    assert not set(seen) & set(instantiations(kernel_resources(_lib.LIB_PATH), "scan_rows_kernel", "Ss2Filter"))
