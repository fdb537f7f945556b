"""The selection stage of a scenario call -- lme_partial_kernel<true> with scenario_final (csrc/trx_reduce.hpp,
csrc/trx_device.hpp) and table_kernel (csrc/trx_scenario.hip) -- on chi^2 vectors designed here, through
trx_debug_select_from_halfchi2 (include/trx_debug.h): the probe runs for ONE branch exactly what trx_scenario_enqueue
runs behind the likelihood kernels, with the masked count on the device and the launch sized for N.

Everything is compared with plain numpy on the host, from the same arrays:
  best draw   the order of torch.argmin: the first NaN row if there is one (ties: the NaN count), else the first row of
              h.min() (ties: (h == h.min()).sum(); -0.0 ties with 0.0); the record's columns are cols[:, r], for the
              twin branch cols[:, N - 1 - r], by bytes; n = 0: cols_pad[:, 0], lnZ = -inf, count 0, ties 0
  evidence, moments, post_x
              x formed as the kernel forms it -- (c0 - h), then + lnprior[pos], each rounded on its own -- and folded by
              tests/test_gpu_reductions.py's _reference; _bounds / _check of that file unchanged (scenario_final's fold
              is lme_final_kernel's: partials l, l + 64, ..., then the butterfly, so the chain lengths of that
              derivation hold).  post_x equals the reference's maximum exactly; NaN where an x is +inf or a row holds
              the "never written" mark, -inf where no x is finite
  status      1, and NaN for lnZ, lnM2, lnWmax and post_x, where a row holds the mark (UNWRITTEN_BITS); an ordinary NaN
              at the same row: status 0 and a finite lnZ
  table       order = np.argsort(h, kind="stable") (NaN last, ties in row order); slot 14 = h[order[:K + 1]], NaN beyond
              n; row j < min(n, K): cols[:, pos(order[j])]; row j >= n: cols_pad[:, j - n]; by bytes, in order
What no kernel writes (the record's slots between the count and slot 16, the table's column K and, for a planet, its
rows 11 .. 13) must still hold the probe's fill, 0x7f7f7f7f7f7f7f7f.

The columns are position-coded (column c at position p holds c 2^27 + p + 0.25), the unused positions of the dense
prior hold +700 and the doubles behind h hold -1e300: a read beside the intended element shows.

Every comparison of a finite evidence prints its error beside its bound (lines "REDUCTIONS-ERR ...", pytest -s); each
test ends with the largest so far ("SELECTION-MAX ...").  Largest absolute errors measured on an MI355X over the whole
file, lnZ / lnM2 / lnWmax, beside the imported bounds at those cases:
    lnZ     7.11e-15  (bound 2.42e-14; n = 3, all rows equal, with the prior)
    lnM2    7.11e-15  (bound 3.42e-14; n = 2, all rows equal)
    lnWmax  8.88e-16  (bound 1.18e-14; n = 2047, narrow base)
-- multiples of the spacing of the result, as in tests/test_gpu_reductions.py: the roundings of the final expression,
never a term of the sum.  Every other comparison (best draw, ties, count, status, post_x, table) is exact.

That the file can fail was shown on scratch builds of the testing library, one change each: table_kernel advancing its
base by the whole tile (caught by the table tests from n = 1921 on), table_before breaking ties towards the later row
(the table tests from n = 2 on), argmin_merge keeping its own row among equals (the fold tests from n = 511 on), the odd
tail's twin prior read one position up (every odd n), scenario_final gathering the twin's best draw unmirrored (nearly
every test).
"""
import math

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from triceratops_amd import _lib
from test_gpu_reductions import C0, LNSIGMA, _bounds, _check, _lme_blocks, _reference

pytestmark = pytest.mark.gpu

UNWRITTEN_BITS = 0x7ff8dead0badc0de           # kUnwrittenBits, csrc/trx_cells.hpp:759 (rowc_kernel's "never written" mark)
MARK = np.array([UNWRITTEN_BITS], dtype=np.uint64).view(np.float64)[0]
FILL = np.frombuffer(b"\x7f" * 8, dtype=np.float64)[0]          # the probe's fill of what no kernel writes
TIES, STATUS, LNM2, LNWMAX = 16, 17, 18, 19   # record slots (include/trx.h)
EXTRA_TOTAL = 777                             # n_total - N
PAD = 8                                       # doubles behind every device vector
TRIP = 1920                                   # new rows per trip of table_kernel (kTableTile - kTableKeep)

MAX_ERR = {"lnZ": (0.0, 0.0, ""), "lnM2": (0.0, 0.0, ""), "lnWmax": (0.0, 0.0, "")}     # (err, its bound, case)


# ---------------------------------------------------------------------------------------------------------------------
# the probe
def _select(h_d, lp_d, cols_d, pad_d, n, N, n_total, ncol, twin, K, moments):
    """trx_debug_select_from_halfchi2 on device tensors -> (record [18 or 20], post_x, table [15][K + 1] or None)"""
    L = _lib.lib()
    assert L.trx_testing
    rec, px = np.empty(20 if moments else 18), np.empty(1)
    table = np.empty(15 * (K + 1)) if K else None
    with torch.cuda.device(h_d.device):
        rc = L.trx_debug_select_from_halfchi2(h_d.data_ptr(), None if lp_d is None else lp_d.data_ptr(), cols_d.data_ptr(),
                                              pad_d.data_ptr(), n, N, n_total, ncol, twin, K, int(moments), LNSIGMA,
                                              rec.ctypes.data, px.ctypes.data, None if table is None else table.ctypes.data,
                                              _lib._stream(h_d))
    _lib.check(rc)
    return rec, float(px[0]), None if table is None else table.reshape(15, K + 1)


_cols_cache = {}


def _cols_dev(ncol, N):
    """[ncol][N + PAD] position-coded columns, made on the device (the last one kept)"""
    key = (ncol, N)
    if key not in _cols_cache:
        _cols_cache.clear()
        p = torch.arange(N, dtype=torch.float64, device="cuda") + 0.25
        c = torch.arange(ncol, dtype=torch.float64, device="cuda") * float(2 ** 27)
        flat = torch.full((ncol * N + PAD,), -3e300, dtype=torch.float64, device="cuda")
        flat[:ncol * N] = (c[:, None] + p[None, :]).reshape(-1)
        _cols_cache[key] = flat
    return _cols_cache[key]


def _cols_host(ncol, pos):
    return np.arange(ncol, dtype=np.float64)[:, None] * float(2 ** 27) + np.asarray(pos, dtype=np.float64)[None, :] + 0.25


def _pad_host(ncol, K):
    """cols_pad [ncol][max(K, 1)]: the stand-in draws"""
    return -(np.arange(ncol, dtype=np.float64)[:, None] * 1024.0 + np.arange(max(K, 1), dtype=np.float64)[None, :] + 0.5)


def _pos(rows, N, twin):
    rows = np.asarray(rows)
    return N - 1 - rows if twin else rows


def _h_dev(h):
    return _lib.dev(np.concatenate((h, np.full(PAD, -1e300))))


def _prior_dev(lp_rows, N, twin):
    dense = np.full(N + PAD, 700.0)
    dense[_pos(np.arange(lp_rows.size), N, twin)] = lp_rows
    return _lib.dev(dense)


# ---------------------------------------------------------------------------------------------------------------------
# the yardstick
def _expect(h, lp_rows, n_total):
    """(best row or -1, ties, mark present, _reference's tuple) of the rows h [n] with their priors, in row order"""
    n = h.size
    best, ties = -1, 0
    if n:
        nan = np.isnan(h)
        same = nan if nan.any() else (h == h.min())
        best, ties = int(np.flatnonzero(same)[0]), int(same.sum())
    with np.errstate(invalid="ignore"):
        x = C0 - h
        if lp_rows is not None:
            x = x + lp_rows
    mark = bool((h.view(np.uint64) == np.uint64(UNWRITTEN_BITS)).any())
    return best, ties, mark, _reference(x, n_total)


def _same_bytes(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _verify(label, got, h, exp, N, n_total, ncol, twin, K, moments):
    """one answer of trx_debug_select_from_halfchi2 against the yardstick"""
    rec, px, table = got
    best, ties, mark, ref = exp
    n = h.size
    pad = _pad_host(ncol, K)
    want_cols = pad[:, 0] if n == 0 else _cols_host(ncol, [_pos(best, N, twin)])[:, 0]
    assert _same_bytes(rec[:ncol], want_cols), (label, "best draw", best, rec[:ncol], want_cols)
    assert rec[ncol + 1] == n and rec[TIES] == ties and rec[STATUS] == (1.0 if mark else 0.0), (label, rec, best, ties)
    assert _same_bytes(rec[ncol + 2:TIES], np.full(TIES - ncol - 2, FILL)), (label, rec)
    evid = [rec[ncol]] + ([rec[LNM2], rec[LNWMAX]] if moments else [])
    if mark:
        assert np.isnan(evid).all() and np.isnan(px), (label, evid, px)
    else:
        _check(evid, ref, n_total, label)
        if np.isfinite(ref[0]):
            for name, g, r, b in zip(("lnZ", "lnM2", "lnWmax"), evid, ref, _bounds(ref, n_total)):
                if abs(g - r) > MAX_ERR[name][0]:
                    MAX_ERR[name] = (abs(g - r), b, label)
        if ref[0] == np.inf:
            assert np.isnan(px), (label, px)
        else:
            assert px == ref[3], (label, px, ref[3])          # (-inf where no x is finite)
    if not K:
        return
    order = np.argsort(h, kind="stable")
    want14 = np.full(K + 1, np.nan)
    m = min(n, K + 1)
    want14[:m] = h[order[:m]]
    assert _same_bytes(table[14], want14), (label, "slot 14", table[14], want14)
    r = min(n, K)
    want = np.empty((ncol, K))
    want[:, :r] = _cols_host(ncol, _pos(order[:r], N, twin))
    want[:, r:] = pad[:, :K - r]
    bad = np.flatnonzero((table[:ncol, :K].view(np.uint64) != want.view(np.uint64)).any(axis=0))
    assert bad.size == 0, (label, "table rows", bad[:8], table[0, bad[:8]], want[0, bad[:8]])
    assert _same_bytes(table[:14, K], np.full(14, FILL)) and _same_bytes(table[ncol:14], np.full((14 - ncol, K + 1), FILL)), label


def _report():
    print("SELECTION-MAX " + " ".join("%s %.3g/%.3g (%s)" % ((k,) + MAX_ERR[k]) for k in MAX_ERR))


COMBOS = [(twin, prior, wide) for twin in (0, 1) for prior in (0, 1) for wide in (0, 1)]


def _run(label, vectors, lp_rows, K, moments, combos=COMBOS):
    """every vector of `vectors` (name -> h) through trx_debug_select_from_halfchi2 with twin 0 and 1, without and with
    the prior, with N == n (as near as N >= max(n, K, 1) allows) and N ~ 3 n; each answer twice, byte for byte"""
    n = lp_rows.size
    for twin, prior, wide in combos:
        N = max(3 * n + 1 if wide else n, K, 1)
        ncol = 14 if (twin or wide) else 11
        n_total = N + EXTRA_TOTAL
        cols_d, pad_d = _cols_dev(ncol, N), _lib.dev(_pad_host(ncol, K))
        lp_d = _prior_dev(lp_rows, N, twin) if prior else None
        for name, h in vectors.items():
            assert h.size == n
            h_d = _h_dev(h)
            args = (h_d, lp_d, cols_d, pad_d, n, N, n_total, ncol, twin, K, moments)
            got = _select(*args)
            case = "%s %s twin=%d prior=%d N=%d K=%d" % (label, name, twin, prior, N, K)
            _verify(case, got, h, _expect(h, lp_rows if prior else None, n_total), N, n_total, ncol, twin, K, moments)
            again = _select(*args)
            assert _same_bytes(got[0], again[0]) and _same_bytes(np.float64(got[1]), np.float64(again[1])), case
            assert K == 0 or _same_bytes(got[2], again[2]), case


# ---------------------------------------------------------------------------------------------------------------------
# the fold: blocks, segments, the odd tail, the argmin with its tie count
def _partition(n):
    """(blocks, pairs per segment, pairs) of lme_partial_body's vector path: one segment per block, a multiple of 256
    pairs; the odd last row is thread 0's of block 0"""
    nv_all, nb = n // 2, _lme_blocks(n)
    seg = (((nv_all + nb - 1) // nb) + 255) & ~255
    return nb, seg, nv_all


def _block_starts(n):
    """first rows of the non-empty blocks"""
    nb, seg, nv_all = _partition(n)
    return [2 * seg * b for b in range(nb) if seg * b < nv_all] or [0]


def _min_rows(n):
    """row 0, row n - 1, each side of every block seam, the last row of the last non-empty block"""
    rows = {0, n - 1, max(2 * (n // 2) - 1, 0)}
    for s in _block_starts(n)[1:]:
        rows |= {s - 1, s}
    return sorted(rows)


def _lnprior_rows(rng, n):
    lp = rng.uniform(-5.0, 0.0, n)
    if n > 8:
        lp[rng.integers(0, n, max(1, n // 500))] = -np.inf
        lp[[0, n // 2, n - 1]] = [-1.25, -1.0, -0.5]       # finite where the arrangements put their special rows
    return lp


LOW = 5.0          # the placed minimum: 15 below the base's 20 .. 22, which still weighs (e^-15 a row)


def _fold_vectors(n, rng):
    base = rng.uniform(20.0, 22.0, n)          # narrow: every row weighs about 1 / n, a lost one 1e-4 .. 1e-7 of the sum
    if n == 0:
        return {"empty": base}
    starts = _block_starts(n)
    last = starts[-1]
    v = {"base": base}
    broad = rng.uniform(200.0, 3000.0, n)      # the queue arm (tests/test_gpu_reductions.py, `third`)
    k = rng.random(n) < 0.3
    broad[k] = rng.normal(20.0, 0.5, int(k.sum()))
    v["broad"] = broad
    for r in _min_rows(n):
        h = base.copy()
        h[r] = LOW
        v["min@%d" % r] = h
    # ties: in every block; a lower row on a higher lane / wave than a later one (rows 74 and 140 against 518 and 522:
    # threads 37 and 70 in their first trip, threads 3 and 5 in their second); scattered; the odd tail and row 0
    h = base.copy()
    h[[min(s + 7, n - 1) for s in starts]] = LOW
    v["ties_every_block"] = h
    for name, rows in (("ties_lanes", (74, 522)), ("ties_waves", (140, 518))):
        if n > rows[1]:
            h = base.copy()
            h[list(rows)] = LOW
            v[name] = h
    h = base.copy()
    h[rng.integers(0, n, 16)] = LOW
    v["ties_scattered"] = h
    h = base.copy()
    h[[0, n - 1]] = LOW
    v["ties_tail_and_row0"] = h
    v["all_equal"] = np.full(n, 33.25)
    v["all_inf"] = np.full(n, np.inf)
    # NaN: one in the last block with the numeric minimum in the first; several; -inf (x = +inf)
    h = base.copy()
    h[min(3, n - 1)] = LOW
    h[min(last + 2, n - 1)] = np.nan
    v["nan_last_block"] = h
    h = base.copy()
    h[[min(s + 11, n - 1) for s in starts] + [n - 1]] = np.nan
    v["nan_several"] = h
    h = base.copy()
    h[n // 2] = -np.inf
    v["neg_inf"] = h
    return v


FOLD_SIZES = [0, 1, 2, 3, 511, 512, 513, 2047, 2048, 2049, 2050, 4097, 8193]


@pytest.mark.parametrize("n", FOLD_SIZES)
def test_fold_argmin_and_record_at_every_seam(n):
    """the sizes at which the index arithmetic of lme_partial_body<true> changes: no pair / one pair / the odd tail
    alone; one thread-row of pairs; two blocks with the seam at row 1024 and the odd tail; 8193: five blocks, the
    last one's segment empty"""
    if n == 8193:
        nb, seg, nv_all = _partition(n)
        assert nb == 5 and seg * 4 >= nv_all            # block 4 has nothing to read
    rng = np.random.default_rng([17, n])
    _run("fold n=%d" % n, _fold_vectors(n, rng), _lnprior_rows(rng, n), 0, 1)
    _report()


def test_fold_with_more_partials_than_lanes():
    """131072 + 2049 rows: 66 partials, so lanes 0 and 1 of the final fold merge two each"""
    n = 131072 + 2049
    assert _lme_blocks(n) == 66
    rng = np.random.default_rng([17, n])
    v = _fold_vectors(n, rng)
    keep = {k: v[k] for k in ("base", "ties_every_block", "nan_several", "min@%d" % (n - 1), "ties_lanes")}
    _run("fold n=%d" % n, keep, _lnprior_rows(rng, n), 0, 1, combos=[(1, 1, 1), (0, 0, 0)])
    _report()


def test_fold_at_the_block_cap():
    """2048 * 2048 + 4099 rows: the block count capped at 2048, 32 partials per lane of the final fold, block 1640 with
    one pair and the blocks behind it with empty segments; the minimum repeated in every non-empty block, the odd tail
    and row 1"""
    n = 2048 * 2048 + 4099
    nb, seg, nv_all = _partition(n)
    assert nb == 2048 and seg * 1640 + 1 == nv_all
    rng = np.random.default_rng([17, n])
    h = rng.uniform(20.0, 22.0, n)
    h[[min(s + 7, 2 * nv_all - 1) for s in _block_starts(n)] + [1, n - 1]] = LOW
    N, twin, ncol = n + 3, 1, 11
    lp_rows = _lnprior_rows(rng, n)
    args = (_h_dev(h), _prior_dev(lp_rows, N, twin), _cols_dev(ncol, N), _lib.dev(_pad_host(ncol, 0)), n, N, N + EXTRA_TOTAL,
            ncol, twin, 0, 1)
    got = _select(*args)
    exp = _expect(h, lp_rows, N + EXTRA_TOTAL)
    assert exp[0] == 1 and exp[1] == 1641 + 2
    _verify("fold n=%d ties_every_block" % n, got, h, exp, N, N + EXTRA_TOTAL, ncol, twin, 0, 1)
    again = _select(*args)
    assert _same_bytes(got[0], again[0]) and _same_bytes(np.float64(got[1]), np.float64(again[1]))
    _cols_cache.clear()
    _report()


@pytest.mark.parametrize("n", [1, 513, 2049, 8193])
def test_never_written_mark_against_an_ordinary_nan(n):
    """the mark at the odd tail (thread 0's scalar row), at row 0, beside a block seam and in the last pair: status 1 and
    NaN for lnZ, lnM2, lnWmax and post_x; an ordinary NaN at the same row: status 0, a finite lnZ, the same best draw"""
    rng = np.random.default_rng([23, n])
    base = rng.uniform(20.0, 22.0, n)
    lp_rows = _lnprior_rows(rng, n)
    for row in sorted({0, n - 1, max(n - 2, 0), _block_starts(n)[-1]}):
        for twin, prior in ((0, 1), (1, 0)):
            N = 2 * n + 5
            ncol, n_total = 14, N + EXTRA_TOTAL
            cols_d, pad_d = _cols_dev(ncol, N), _lib.dev(_pad_host(ncol, 0))
            lp_d = _prior_dev(lp_rows, N, twin) if prior else None
            rec = {}
            for name, value in (("mark", MARK), ("nan", np.nan)):
                h = base.copy()
                h[row] = value
                got = _select(_h_dev(h), lp_d, cols_d, pad_d, n, N, n_total, ncol, twin, 0, 1)
                label = "%s at row %d of %d twin=%d" % (name, row, n, twin)
                _verify(label, got, h, _expect(h, lp_rows if prior else None, n_total), N, n_total, ncol, twin, 0, 1)
                rec[name] = got
            r, px, _ = rec["mark"]
            assert r[STATUS] == 1.0 and np.isnan([r[ncol], r[LNM2], r[LNWMAX], px]).all(), (row, r, px)
            r2, px2, _ = rec["nan"]
            assert r2[STATUS] == 0.0 and _same_bytes(r[:ncol], r2[:ncol]) and r2[TIES] == r[TIES] == 1.0
            assert (np.isfinite(r2[ncol]) and np.isfinite(px2)) if n > 1 else (r2[ncol] == -np.inf and px2 == -np.inf)


# ---------------------------------------------------------------------------------------------------------------------
# the table of the K best draws
def _table_vectors(n, K, rng):
    base = rng.uniform(10.0, 20.0, n)
    if n == 0:
        return {"empty": base}
    v = {"ascending": np.sort(base),                    # after the first trip nothing enters: the sort is skipped
         "descending": np.sort(base)[::-1].copy()}      # every trip sorts
    k = min(K, n)
    h = base.copy()
    h[n - k:] = rng.uniform(0.0, 1.0, k)
    v["best_in_last_trip"] = h
    h = base.copy()
    rows = (np.arange(0, n, TRIP) + 17)
    rows = rows[rows < n][:K]
    h[rows] = rng.uniform(0.0, 1.0, rows.size)
    v["one_per_trip"] = h
    h = base.copy()
    for i, r in enumerate((1919, 1920, 1921)):
        if r < n:
            h[r] = 0.5 - 0.125 * i
    v["beside_the_trip_seam"] = h
    h = base.copy()
    h[np.unique(np.linspace(0, n - 1, 3 * K).astype(np.int64))] = 2.0        # the lowest rows must win
    v["repeated_3K"] = h
    h = base.copy()
    i = np.arange(n)
    h[i % 3 != 2] = np.where(i % 2 == 1, 0.0, -0.0)[i % 3 != 2]
    v["signed_zeros"] = h
    some = np.unique(np.linspace(0, n - 1, max(K // 2, 1)).astype(np.int64))
    h = np.full(n, np.nan)
    h[some] = rng.uniform(0.0, 1.0, some.size)
    v["few_then_nan"] = h
    h = np.full(n, np.inf)
    h[some] = rng.uniform(0.0, 1.0, some.size)
    v["inf_tail"] = h
    return v


def _table_sizes(K):
    return sorted({0, 1, K - 1, K, K + 1, 128, 129, 1919, 1920, 1921, 2048, 3840, 3841, 70001})


TABLE_CASES = [(K, n) for K in (2, 100, 127) for n in _table_sizes(K)]


@pytest.mark.parametrize("K,n", TABLE_CASES, ids=["K%d-n%d" % c for c in TABLE_CASES])
def test_table_rows_in_order_at_every_trip_seam(K, n):
    """table_kernel streams 1920 new rows per trip next to the 128 kept: counts below, at and above K, the 128 kept, one,
    two and many trips; the record of the same call is checked beside the table (stride 18: no moments)"""
    rng = np.random.default_rng([29, K, n])
    _run("table n=%d" % n, _table_vectors(n, K, rng), _lnprior_rows(rng, n), K, 0)
    _report()


# ---------------------------------------------------------------------------------------------------------------------
def test_probe_leaves_the_persistent_block_clean_for_the_next_scenario_call():
    """scenario call, trx_debug_select_from_halfchi2, scenario call on ONE stream: the last record equals, byte for byte,
    the record the same call gives on a stream of its own.  The first call on the shared stream is the larger one (a
    binary: two branches), so that the stream's scratch does not grow -- and clear its persistent block -- behind the
    probe, and so that a record the last call failed to write would show as the binary's, left in the pinned block"""
    from test_gpu_posterior import _native
    n = 8193
    rng = np.random.default_rng(31)
    v = _fold_vectors(n, rng)
    lp_rows = _lnprior_rows(rng, n)
    fresh, shared = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(fresh):
        want = _native("planet", 0)[0]
    with torch.cuda.stream(shared):
        first = _native("binary", 0)[0]
        _run("clean n=%d" % n, {k: v[k] for k in ("base", "nan_several", "ties_every_block")}, lp_rows, 100, 1,
             combos=[(0, 1, 1), (1, 0, 0)])
        after = _native("planet", 0)[0]
    written = np.r_[0:13, TIES, STATUS]             # a planet's record: 11 columns, lnZ, the count; ties, status
    assert np.isfinite(want[written]).all() and want[STATUS] == 0.0
    assert not _same_bytes(first[written], want[written])
    assert _same_bytes(after[written], want[written]), (want, after)


def test_argument_checks():
    """a pointer off its 16-byte boundary is TRX_ERR_ARG, as lme_draws has it; so are N < n, N < K, K = 1 and a column
    count that no scenario has"""
    L = _lib.lib()
    n, N, ncol = 64, 200, 11
    h_d = _h_dev(np.full(n + 1, 30.0))
    cols_d, pad_d = _cols_dev(ncol, N), _lib.dev(_pad_host(ncol, 100))
    rec, px, table = np.empty(20), np.empty(1), np.empty(15 * 128)

    def call(h_ptr, n=n, N=N, ncol=ncol, K=0):
        return L.trx_debug_select_from_halfchi2(h_ptr, None, cols_d.data_ptr(), pad_d.data_ptr(), n, N, N, ncol, 0, K, 0,
                                                LNSIGMA, rec.ctypes.data, px.ctypes.data, table.ctypes.data,
                                                _lib._stream(h_d))

    assert h_d.data_ptr() % 16 == 0 and call(h_d.data_ptr()) == 0
    assert call(h_d.data_ptr() + 8) == 1                    # TRX_ERR_ARG
    assert call(h_d.data_ptr(), N=n - 1) == 1 and call(h_d.data_ptr(), K=1) == 1 and call(h_d.data_ptr(), ncol=12) == 1
    assert call(h_d.data_ptr(), n=10, N=50, K=100) == 1 and call(h_d.data_ptr(), n=10, N=100, K=100) == 0
