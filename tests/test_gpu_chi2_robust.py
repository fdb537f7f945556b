"""chi2_robust_kernel<STAGE> through _lib.chi2_grid_robust (trxr_chi2_grid_robust) against
_numerics.robust_halfchi2 in long double, on the inputs of tests/test_datasets_outliers_api.py.

Shapes: n_time in {1, 2, 63, 64, 65, 129, 333, 2048, 2049} (one lane, one pair, one trip less / exactly / more than a wave, an
odd tail, the last staged length and the first unstaged one) x n in {1, 2, 3, 257} (a wave without a second row, with one,
an odd count, more than one block); (65, 8195) and (2048, 5123): past the cap of resident blocks, so waves take further
passes; 3 rows of 70 001 stamps.  The rows past 257 repeat the first 257 (row r holds row r % 257): the reference is
computed once per n_time for 257 rows and serves every n, and a repeated row must repeat its bits.

Bars, none of them chosen from results:
  |h - reference| <= 1e-12 sum_t (1 + lo_t) + 1e-12 per row (the bar of the host statement, test_datasets_outliers_api.py);
  h >= 0;  h <= H + T c0 + bar and h <= k2 H + T c1 + bar, H what chi2_grid_weighted gives on the same inputs;
  the same bits for a view one double off the 16-byte boundary, for a second call, and for a row at position 0, at n - 1
        and alone;
  the +inf mask is chi2_grid_weighted's, a NaN depth included; accumulation is out + h in IEEE arithmetic.
"""
import ctypes

import numpy as np
import pytest
import torch

from test_datasets_outliers_api import LD, OFFS, PAIRS, robust_inputs, robust_reference
from triceratops_amd import _lib
from triceratops_amd.datasets import robust_constants

pytestmark = pytest.mark.gpu

BASE = 257
SHAPES = ([(t, n) for t in (1, 2, 63, 64, 65, 129, 333, 2048, 2049) for n in (1, 2, 3, 257)]
          + [(65, 8195), (2048, 5123), (70001, 3)])
_cache = {}


def _case(n_time, off):
    """the device inputs of (n_time, off) for the 257 base rows (fewer at 70 001 stamps) and, per pair of constants, the
    long-double reference and the bar: made once"""
    key = (n_time, off)
    if key not in _cache:
        rows = 3 if n_time > 4096 else BASE
        flux, w, grid = robust_inputs(n_time, rows, off)
        refs = {}
        for pair in PAIRS:
            refs[pair] = robust_reference(flux, w, grid, robust_constants(*pair))
        _cache[key] = (_lib.dev(flux), _lib.dev(w), _lib.dev(grid), refs)
    return _cache[key]


def _rows(grid_d, n):
    """n rows: row r is base row r % 257"""
    base = grid_d.shape[0]
    if n <= base:
        return grid_d[:n].contiguous()
    return grid_d.repeat(-(-n // base), 1)[:n].contiguous()


@pytest.mark.parametrize("n_time,n", SHAPES)
def test_against_the_long_double_statement_and_the_bounds(n_time, n):
    worst = 0.0
    for off in OFFS:
        f_d, w_d, base_d, refs = _case(n_time, off)
        grid_d = _rows(base_d, n)
        plain = _lib.chi2_grid_weighted(f_d, w_d, grid_d).cpu().numpy()
        for pair in PAIRS:
            c0, c1, k2 = robust_constants(*pair)
            got_d = _lib.chi2_grid_robust(f_d, w_d, grid_d, c0, c1, k2)
            again = _lib.chi2_grid_robust(f_d, w_d, grid_d, c0, c1, k2)
            got = got_d.cpu().numpy()
            assert got.shape == (n,) and got.tobytes() == again.cpu().numpy().tobytes()
            want, bar = refs[pair]
            idx = np.arange(n) % base_d.shape[0]
            err = np.abs((got.astype(LD) - want[idx]).astype(np.float64))
            worst = max(worst, float(np.max(err / bar[idx])))
            assert (err <= bar[idx]).all(), (pair, off, float(np.max(err / bar[idx])))
            assert (got >= 0).all()
            assert (got <= plain + n_time * c0 + bar[idx]).all()
            assert (got <= k2 * plain + n_time * c1 + bar[idx]).all()
            # a repeated row repeats its bits: neither the row's position nor the wave's pass enters
            if n > base_d.shape[0]:
                assert got.tobytes() == got[:base_d.shape[0]][idx].tobytes()
    print("n_time %d, n %d: max |h - reference| / bar %.3g" % (n_time, n, worst))


@pytest.mark.parametrize("n_time", [1, 2, 63, 65, 333, 2048, 2049])
def test_bits_do_not_depend_on_alignment_or_position(n_time):
    n = 9
    c = robust_constants(0.05, 10.0)
    f_d, w_d, base_d, _ = _case(n_time, 5.0)
    grid_d = base_d[:n].contiguous()
    want = _lib.chi2_grid_robust(f_d, w_d, grid_d, *c).cpu().numpy()
    # a view one double off the 16-byte boundary
    buf = torch.empty(n * n_time + 1, dtype=torch.float64, device=grid_d.device)
    assert buf.data_ptr() % 16 == 0
    view = buf[1:].view(n, n_time)
    view.copy_(grid_d)
    assert view.data_ptr() % 16 == 8
    assert _lib.chi2_grid_robust(f_d, w_d, view, *c).cpu().numpy().tobytes() == want.tobytes()
    # ... and flux / inv_var likewise
    fw = torch.empty(2 * n_time + 3, dtype=torch.float64, device=grid_d.device)
    f1, w1 = fw[1:1 + n_time], fw[n_time + 2 + (n_time & 1):][:n_time]
    f1.copy_(f_d)
    w1.copy_(w_d)
    assert _lib.chi2_grid_robust(f1, w1, grid_d, *c).cpu().numpy().tobytes() == want.tobytes()
    # row 4 at position 0, at n - 1 and alone
    k = 4
    first = torch.cat([grid_d[k:k + 1], grid_d[:n - 1]]).contiguous()
    last = torch.cat([grid_d[:k], grid_d[k + 1:], grid_d[k:k + 1]]).contiguous()
    alone = grid_d[k:k + 1].contiguous()
    assert _lib.chi2_grid_robust(f_d, w_d, first, *c).cpu().numpy()[0].tobytes() == want[k].tobytes()
    assert _lib.chi2_grid_robust(f_d, w_d, last, *c).cpu().numpy()[n - 1].tobytes() == want[k].tobytes()
    assert _lib.chi2_grid_robust(f_d, w_d, alone, *c).cpu().numpy()[0].tobytes() == want[k].tobytes()


@pytest.mark.parametrize("n_time", [2, 65, 2049])
def test_mask_accumulation_and_nan(n_time):
    n = 11
    c = robust_constants(0.01, 5.0)
    f_d, w_d, base_d, _ = _case(n_time, 5.0)
    grid_d = base_d[:n].contiguous()
    h = _lib.chi2_grid_robust(f_d, w_d, grid_d, *c).cpu().numpy()
    assert np.isfinite(h).all()
    # the secondary-eclipse mask: chi2_grid_weighted's, a NaN depth included
    sec = np.array([0.0, 1e-3, 2e-3, np.nan, 1.5e-3, np.inf, -1.0, 1.4999e-3, np.nan, 3e-3, 0.0])
    sec_d = _lib.dev(sec)
    for limit in (1.5e-3, float("inf"), 0.0):
        got = _lib.chi2_grid_robust(f_d, w_d, grid_d, *c, secdepth=sec_d, sec_limit=limit).cpu().numpy()
        ref = _lib.chi2_grid_weighted(f_d, w_d, grid_d, sec_d, limit).cpu().numpy()
        assert np.array_equal(np.isposinf(got), np.isposinf(ref))
        with np.errstate(invalid="ignore"):
            assert np.array_equal(np.isposinf(got), sec >= limit)
        assert got[~np.isposinf(got)].tobytes() == h[~np.isposinf(got)].tobytes()
    # accumulation onto finite, +inf and NaN values; +inf stays +inf also where the row is masked
    prev = np.array([1.5, np.inf, np.nan, 0.0, 1e300, -2.0, np.inf, 3.25, np.nan, 7.0, 1e-300])
    out = _lib.dev(prev.copy())
    back = _lib.chi2_grid_robust(f_d, w_d, grid_d, *c, secdepth=sec_d, sec_limit=1.5e-3, out=out)
    assert back.data_ptr() == out.data_ptr()
    with np.errstate(invalid="ignore"):
        want = prev + np.where(sec >= 1.5e-3, np.inf, h)
    assert out.cpu().numpy().tobytes() == want.tobytes()
    # a NaN in a row gives NaN, for that row alone; an inf likewise gives no finite value
    bad = grid_d.clone()
    bad[3, n_time - 1] = float("nan")
    bad[6, 0] = float("nan")
    got = _lib.chi2_grid_robust(f_d, w_d, bad, *c).cpu().numpy()
    assert np.isnan(got[[3, 6]]).all()
    keep = np.ones(n, dtype=bool)
    keep[[3, 6]] = False
    assert got[keep].tobytes() == h[keep].tobytes()
    # n == 0 succeeds and leaves the output untouched
    sentinel = _lib.dev(np.array([4.0, 5.0]))
    torch.cuda.synchronize()
    rc = _lib.lib().trxr_chi2_grid_robust(f_d.data_ptr(), w_d.data_ptr(), grid_d.data_ptr(), n_time, 0, None,
                                          ctypes.c_double(float("inf")), 0, sentinel.data_ptr(), *c,
                                          torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert sentinel.cpu().numpy().tolist() == [4.0, 5.0]
    empty = _lib.chi2_grid_robust(f_d, w_d, grid_d[:0], *c)
    assert empty.shape == (0,)
