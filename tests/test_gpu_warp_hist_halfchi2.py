"""trxw_hist_from_halfchi2 against numpy: the weight histogram of one branch from chi^2/2
values, a prior column and draw indices already on the device -- the export the datasets path feeds its adaptive
importance maps from.

The pre-map uniforms come from the draw dump (tests/test_gpu_warp.py: _operator, _expected_hist), never from a second
implementation of the generator.  The bar per bin is test_gpu_warp's: |device - numpy| <= the number of weighted rows in
that bin (the device's exp against numpy's moves a floor by at most one).  Everything else is exact."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from test_gpu_posterior_chain import _calls
from test_gpu_warp import CONSUMED, KINDS, _expected_hist, _grid, _operator

pytestmark = pytest.mark.gpu

WG = 256                      # threads of a workgroup of warp_hist_kernel
THREADS = 256 * WG            # ... and of its launch (kWarpHistBlocks workgroups): one row per thread up to here
C0 = -0.5 * np.log(2 * np.pi)


def _words(t):
    return t.cpu().numpy().view(np.uint64)


def _export(a, h, lp, idx, lnsigma):
    from triceratops_amd import _lib
    dev = _lib.compute_device()
    h_d = _lib.dev(np.ascontiguousarray(h, dtype=np.float64), dev)
    lp_d = None if lp is None else _lib.dev(np.ascontiguousarray(lp, dtype=np.float64), dev)
    idx_d = torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int64)).to(dev)
    return _words(_lib.warp_hist_from_halfchi2(a, h_d, lp_d, idx_d, lnsigma))


# ---- the real branches ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["TTP", "PTP", "TEB", "BEB"])
@pytest.mark.parametrize("mapped", [False, True])
def test_real_branches_are_numpys_histogram(kind, mapped, monkeypatch):
    from triceratops_amd import _lib
    _lib.require_gpu()
    call = _calls()[KINDS[kind]]
    y = _operator(call, None, monkeypatch)["dump"]                       # the pre-map uniforms of this seed
    # (unmapped: the call as it is -- TTP and TEB then have no prior column: the NULL path)
    run = _operator(call, _grid() if mapped else None, monkeypatch)
    a, lnsigma = run["scen"].a, float(np.log(run["scen"].sigma))
    masks = [run["mask"]] + ([] if run["mask_twin"] is None else [run["mask_twin"]])
    assert len(masks) == (1 if kind in ("TTP", "PTP") else 2)
    got = []
    for m, h in zip(masks, run["h"]):
        idx = np.flatnonzero(m)
        got.append(_export(a, h, None if run["lnprior"] is None else run["lnprior"][idx], idx, lnsigma))
    got = np.stack(got)
    X = np.ascontiguousarray(got[:, 0]).view(np.float64)
    used = CONSUMED[kind]
    for b, (n_rows, bins, rows) in enumerate(_expected_hist(run, y, used, X)):       # (asserts |X - nanmax(x)| < 1e-9)
        assert got[b, 1] == n_rows and n_rows > 0 and np.all(got[b, 2:8] == 0)
        dev = got[b, 8:].astype(np.float64).reshape(7, 64)
        worst = np.max(np.abs(dev - bins) - rows)
        print("%s %s branch %d: %d rows with weight, worst |device - numpy| - rows in bin = %g"
              % (kind, "mapped" if mapped else "unmapped", b, n_rows, worst))
        assert np.all(np.abs(dev - bins) <= rows)
        for s in range(7):
            if s not in used:
                assert not got[b, 8 + 64 * s:8 + 64 * (s + 1)].any()
        sums = [int(got[b, 8 + 64 * s:8 + 64 * (s + 1)].sum(dtype=np.uint64)) for s in used]
        assert len(set(sums)) == 1 and sums[0] > 0, sums                # every row enters every consumed slot once


# ---- synthetic rows --------------------------------------------------------------------------------------------------------
_src = {}


def _source(monkeypatch):
    """a PTP call's draw arguments, pre-map uniforms and masked indices (five consumed slots), made once"""
    if not _src:
        run = _operator(_calls()[KINDS["PTP"]], None, monkeypatch)
        _src["a"], _src["y"], _src["masked"] = run["scen"].a, run["dump"], np.flatnonzero(run["mask"])
        assert _src["masked"].size > 100
    return _src["a"], _src["y"], _src["masked"]


LNSIGMA = -6.5


def _numpy_block(y, used, h, lp, idx):
    """the block numpy forms: (words 0 .. 7 less X, X, bins [7][64], weighted rows per bin [7][64]); all zero without a
    finite X"""
    bins, rows = np.zeros((7, 64)), np.zeros((7, 64))
    with np.errstate(invalid="ignore"):
        x = (C0 - LNSIGMA) - h
        if lp is not None:
            x = x + lp
    if x.size == 0 or np.isnan(x).all():
        return 0, None, bins, rows
    X = np.nanmax(x)
    if not np.isfinite(X):
        return 0, None, bins, rows
    with np.errstate(invalid="ignore"):
        d = x - X
        keep = d > -80.0
    q = np.floor(np.minimum(np.exp(d[keep]), 1.0) * 2.0 ** 32)
    for s in used:
        k = np.minimum((y[s][idx][keep] * 64).astype(int), 63)
        np.add.at(bins[s], k, q)
        np.add.at(rows[s], k, 1.0)
    return int(keep.sum()), X, bins, rows


def _check(got, want, used):
    n_rows, X, bins, rows = want
    if X is None:
        assert not got.any()
        return
    assert abs(np.ascontiguousarray(got[:1]).view(np.float64)[0] - X) < 1e-9
    assert got[1] == n_rows and not got[2:8].any()
    dev = got[8:].astype(np.float64).reshape(7, 64)
    assert np.all(np.abs(dev - bins) <= rows)
    for s in range(7):
        if s not in used:
            assert not dev[s].any()
    assert len({int(got[8 + 64 * s:8 + 64 * (s + 1)].sum(dtype=np.uint64)) for s in used}) == 1


def _rows(n, pattern, masked, seed):
    rng = np.random.default_rng(seed)
    idx = rng.choice(masked, size=n, replace=True)                        # with repeats, in no order
    h = rng.uniform(0.0, 30.0, n) ** 2 / 8.0                              # 0 .. 112: rows on both sides of the cut
    lp = rng.normal(0.0, 3.0, n)
    if pattern == "one_row_inside_the_cut" and n:
        h = 500.0 + h
        lp = np.zeros(n)
        h[n // 3] = 1.0
    elif pattern == "inf_and_nan" and n:
        h[::5] = np.inf
        h[1::7] = np.nan
        lp[2::11] = -np.inf
    elif pattern == "all_inf":
        h[:] = np.inf
    elif pattern == "one_minus_inf" and n:
        h[n // 2] = -np.inf
    return idx, h, lp


SIZES = [0, 1, WG - 1, WG, WG + 1, THREADS - 1, THREADS, THREADS + 1, 70001]


@pytest.mark.parametrize("with_prior", [True, False])
@pytest.mark.parametrize("n", SIZES)
def test_synthetic_rows_of_every_size(n, with_prior, monkeypatch):
    from triceratops_amd import _lib
    _lib.require_gpu()
    a, y, masked = _source(monkeypatch)
    idx, h, lp = _rows(n, "random", masked, 1000 + n)
    if not with_prior:
        lp = None
    got = _export(a, h, lp, idx, LNSIGMA)
    want = _numpy_block(y, CONSUMED["PTP"], h, lp, idx)
    assert (want[1] is None) == (n == 0)
    if n > 1:
        assert 0 < want[0] < n                                            # some rows beyond the cut, some inside
    _check(got, want, CONSUMED["PTP"])


@pytest.mark.parametrize("with_prior", [True, False])
@pytest.mark.parametrize("n", [1, WG + 1, 70001])
@pytest.mark.parametrize("pattern", ["one_row_inside_the_cut", "inf_and_nan", "all_inf", "one_minus_inf"])
def test_synthetic_row_patterns(pattern, n, with_prior, monkeypatch):
    from triceratops_amd import _lib
    _lib.require_gpu()
    a, y, masked = _source(monkeypatch)
    idx, h, lp = _rows(n, pattern, masked, 2000 + n)
    if not with_prior:
        lp = None
    got = _export(a, h, lp, idx, LNSIGMA)
    want = _numpy_block(y, CONSUMED["PTP"], h, lp, idx)
    if pattern in ("all_inf", "one_minus_inf"):
        assert want[1] is None and not got.any()                          # X = -inf / +inf: the zero block
    elif pattern == "one_row_inside_the_cut":
        assert want[0] == 1 and got[1] == 1
        for s in CONSUMED["PTP"]:
            assert int(got[8 + 64 * s:8 + 64 * (s + 1)].sum(dtype=np.uint64)) == 2 ** 32         # its weight is exp(0) = 1
    elif n > 1:
        assert 0 < want[0] < n - n // 5                                   # the +inf and NaN rows carry no weight
    _check(got, want, CONSUMED["PTP"])


def test_two_calls_give_the_same_bytes_and_a_dirty_block_does_not_matter(monkeypatch):
    from triceratops_amd import _lib
    import ctypes
    _lib.require_gpu()
    a, y, masked = _source(monkeypatch)
    idx, h, lp = _rows(70001, "inf_and_nan", masked, 5)
    first = _export(a, h, lp, idx, LNSIGMA)
    assert first[1] > 0 and first.tobytes() == _export(a, h, lp, idx, LNSIGMA).tobytes()
    dev = _lib.compute_device()
    h_d, lp_d, idx_d = _lib.dev(h, dev), _lib.dev(lp, dev), torch.from_numpy(np.ascontiguousarray(idx)).to(dev)
    out = torch.full((_lib.WARP_BRANCH,), 0x7123456789abcdef, dtype=torch.int64, device=dev)
    ws = _lib.workspace(dev)
    with torch.cuda.device(dev):
        rc = _lib.lib().trxw_hist_from_halfchi2(ctypes.addressof(a), h_d.data_ptr(), lp_d.data_ptr(), idx_d.data_ptr(),
                                                    h.size, LNSIGMA, out.data_ptr(), ws.data_ptr(), ws.numel() * 8,
                                                    _lib._stream(h_d))
    assert rc == 0
    assert _words(out).tobytes() == first.tobytes()
    # ... nor the order of the rows: integer sums
    p = np.random.default_rng(9).permutation(h.size)
    assert _export(a, h[p], lp[p], idx[p], LNSIGMA).tobytes() == first.tobytes()
