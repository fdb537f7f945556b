"""One row per wave: a full evaluation hands its rows to the waves dearest first (trx_cells.hpp: row_cost_key,
order_file_rows, row_order_at).

A row's chi^2 is a direct sum in cell order, by the row's own wave from its own block, so WHICH wave takes a row cannot
change a bit of any output: every comparison here is an equality of 64-bit patterns, not a tolerance.

  * the same bits with the order on and off (trx_set_row_order), on a uniform grid (the stencil instantiation: 384 stamps
    at 0.24 exposures per step, above the 320 of the one-row variant) and on the same stamps jittered (the other one-row
    instantiation), for 1, 63, 64, 65 (one row more than a wave of rowc_kernel), 1000 and 4097 rows (one more than the
    chip's 4096 wave slots), a TP and an EB family with the secondary rule's rows skipped and evaluated;
  * the order itself, read back (trx_debug_row_order): every row exactly once, the counts sum to the rows, every row in
    the bucket of its key -- computed HERE from the window in the row blocks, by the kernel's own sequence of IEEE
    operations --, hence no row of a bucket cheaper than a row of the next, and the rows that are never evaluated last;
  * a captured and replayed call gives the bits of an eager one (the lists are scratch of the call).

The grid lies off conjunction, [0.02, 0.15] d, so that hand-made rows reach every kind of window: the whole curve, one or
two cells (a ladder of impact parameters whose windows end around the first stamps), none of the span, none at all (the
body passes the star by), the hull of the two passages of an e = 0.9 orbit seen along its major axis, a NaN parameter, an
EB row that the secondary rule excludes.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from triceratops_amd import _lib, synth
from triceratops_amd.constants import Rearth, Rsun

pytestmark = pytest.mark.gpu

N_TIME = 384
COUNTS = (1, 63, 64, 65, 1000, 4097)
N_MAX = max(COUNTS)
N_LADDER = 128
BUCKETS, SHARDS = 16, 4
TWO_PI = 6.283185307179586
# RowC (trx_device.hpp): the doubles of a row block that the key reads
I_T0, I_NMOT, I_WLO, I_WHI, I_EXCL = 1, 2, 10, 11, 18

# (the e = 0.9 row with a second near-side passage of tests/test_gpu_kernels.py, as an EB row)
HULL_EB = np.array([9.62080439e-01, 2.93357695e-05, 1.23513199e+01, 6.48158862e+01, 1.59025933e+12, 1.38005527e+00,
                    1.52880035e-01, 5.74606889e-02, 9.00000000e-01, 1.05234974e+02, 2.09587868e-01])


def _tp_row(k, per, b, a_R, R_s=1.0, ecc=0.0, argp=0.0, fr=0.0):
    inc = np.degrees(np.arccos(b / a_R))
    return np.array([k * R_s * Rsun / Rearth, per, inc, a_R * R_s * Rsun, R_s, 0.4, 0.25, ecc, argp, fr])


def _hand_made_tp():
    rows = [
        _tp_row(0.15, 30.0, 0.0, 8.0, R_s=2.0),                 # a transit of more than a day: the whole curve
        _tp_row(0.1, 10.0, 0.3, 20.0),                         # half width 0.09 d: part of the span
        _tp_row(0.05, 5.0, 0.2, 60.0),                         # half width 0.014 d: ends before the first stamp
        _tp_row(0.1, 10.0, 1.5, 20.0),                         # passes the star by: no window at all
        np.array([HULL_EB[0] * Rsun / Rearth, *HULL_EB[2:]]),       # e = 0.9, two passages
        _tp_row(0.1, 10.0, 0.3, 20.0),                         # (becomes the NaN row below)
    ]
    rows[-1][1] = np.nan
    # the ladder: half widths from 0.029 d down to nothing, in steps of half a cell around the first stamp (0.02 d)
    rows += [_tp_row(0.1, 10.0, b, 20.0) for b in np.linspace(1.04, 1.10, N_LADDER)]
    return np.stack(rows, axis=1)


def _hand_made_eb():
    tp = _hand_made_tp()
    n = tp.shape[1]
    eb = np.empty((11, n))
    eb[0] = tp[0] * Rearth / Rsun            # R_EB
    eb[1] = 1e-5                             # a faint companion: the secondary rule excludes nothing
    eb[2:] = tp[1:]
    eb[:, 4] = HULL_EB
    # a deep secondary eclipse: excluded by the rule, settled by rowc_kernel's quick test at the secondary conjunction
    excluded = np.array([0.8, 0.4, 3.0, 89.5, 10.0 * Rsun, 1.0, 0.4, 0.25, 0.0, 0.0, 0.0])
    return np.concatenate([excluded[:, None], eb], axis=1)


@pytest.fixture(scope="module")
def inputs():
    """Built once and never changed: the two grids, the light curve, the two row blocks (hand-made rows first, so that
    every count from 63 on holds the first of them and 1000 and 4097 all)."""
    _lib.require_gpu()
    rng = np.random.default_rng(synth.SEED + 800)
    t_uni = np.linspace(0.02, 0.15, N_TIME)
    dt = t_uni[1] - t_uni[0]
    assert 0.111 < dt / synth.EXPTIME < 0.3          # what launch_header asks of a grid for the stencil
    t_jit = np.sort(t_uni + rng.uniform(-0.3, 0.3, N_TIME) * dt)
    ref = _tp_row(0.1, 10.0, 0.3, 20.0)[:, None]
    grids = {}
    for name, t in (("uniform", t_uni), ("jittered", t_jit)):
        t_d = _lib.dev(t)
        curve, _ = _lib.flux_grid(_lib.MODEL_TP, 0, t_d, _lib.dev(ref), synth.EXPTIME, synth.NSAMPLES, False)
        flux = synth.noisy_light_curve(np.random.default_rng(synth.SEED + 801), curve[0].cpu().numpy())
        grids[name] = (t, t_d, _lib.dev(flux))
    tp_hand, eb_hand = _hand_made_tp(), _hand_made_eb()
    tp = np.concatenate([tp_hand, synth.family_rows(rng, synth.FAMILIES[3], N_MAX - tp_hand.shape[1])], axis=1)   # PTP
    eb = np.concatenate([eb_hand, synth.family_rows(rng, synth.FAMILIES[4], N_MAX - eb_hand.shape[1])], axis=1)   # PEB
    return {"grids": grids, "tp": np.ascontiguousarray(tp), "eb": np.ascontiguousarray(eb)}


FAMILIES = (("tp", _lib.MODEL_TP, 0), ("eb", _lib.MODEL_EB, 0), ("eb", _lib.MODEL_EB, _lib.FLAG_EVALUATE_EXCLUDED))
CASES = [(g, f) for g in ("uniform", "jittered") for f in range(len(FAMILIES))]
IDS = ["%s-%s%s" % (g, FAMILIES[f][0], "-evaluate-excluded" if FAMILIES[f][2] else "") for g, f in CASES]


def _call(inputs, grid, fam, n, out=None, rows_d=None):
    key, model, flags = FAMILIES[fam]
    _, t_d, f_d = inputs["grids"][grid]
    if rows_d is None:
        rows_d = _lib.dev(np.ascontiguousarray(inputs[key][:, :n]))
    return _lib.lnl_batch(model, flags, t_d, f_d, synth.SIGMA, rows_d, synth.EXPTIME, synth.NSAMPLES, out=out)


def _row_order(on):
    assert _lib.lib().trx_set_row_order(1 if on else 0) == 0


@pytest.mark.parametrize("grid,fam", CASES, ids=IDS)
def test_same_bits_with_the_order_on_and_off(inputs, grid, fam):
    try:
        for n in COUNTS:
            _row_order(True)
            on = _call(inputs, grid, fam, n).cpu().numpy()
            _row_order(False)
            off = _call(inputs, grid, fam, n).cpu().numpy()
            assert np.array_equal(on.view(np.uint64), off.view(np.uint64)), (grid, FAMILIES[fam], n)
            assert np.array_equal(np.isnan(on), np.isnan(off)) and np.array_equal(np.isposinf(on), np.isposinf(off))
            if n >= 1000:
                # (the hand-made rows are what they were made to be: a NaN row -- which the secondary rule turns into
                # +inf, as np.min does in the reference --, and under the rule a +inf row)
                assert np.isfinite(on).any()
                if FAMILIES[fam][0] == "eb":
                    assert np.isposinf(on[0]) and np.isposinf(on[6])      # (+inf whether or not its light curve was evaluated)
                else:
                    assert np.isnan(on[5])
    finally:
        _row_order(True)


def _host_keys(blocks, t, settled):
    """row_cost_key of trx_cells.hpp, operation for operation (numpy rounds every one of them as the device does)."""
    n_time = t.size
    wlo, whi, nmot, t0 = blocks[:, I_WLO], blocks[:, I_WHI], blocks[:, I_NMOT], blocks[:, I_T0]
    tg0, tg1 = t[0], t[-1]
    keys = np.zeros(blocks.shape[0], dtype=np.int64)
    with np.errstate(all="ignore"):
        w = whi - wlo
        live = ~settled & (w >= 0.0) & (nmot > 0.0) & (nmot < np.inf)
        whole = live & (w >= TWO_PI)
        keys[whole] = n_time
        part = live & ~whole
        pa, pb = nmot * (tg0 - t0), nmot * (tg1 - t0)
        part &= (np.abs(pa) < 1e15) & (np.abs(pb) < 1e15)
        xa, xb = pa - wlo, pb - wlo
        fa, fb = np.floor(xa / TWO_PI), np.floor(xb / TWO_PI)
        ra = np.minimum(np.maximum(xa - TWO_PI * fa, 0.0), w)
        rb = np.minimum(np.maximum(xb - TWO_PI * fb, 0.0), w)
        inside = (fb * w + rb) - (fa * w + ra)
        step = (pb - pa) / float(n_time - 1)
        cells = inside / step
        part &= cells > 0.0
        cells = np.minimum(cells, float(n_time))
        keys[part] = (cells[part] + 0.5).astype(np.int64)
    return keys


def _bucket(keys):
    return BUCKETS - 1 - np.clip((keys * BUCKETS) // (N_TIME + 1), 0, BUCKETS - 1)


@pytest.mark.parametrize("grid,fam", CASES, ids=IDS)
def test_the_order_is_a_permutation_sorted_by_cost(inputs, grid, fam):
    key, model, flags = FAMILIES[fam]
    skipping = model == _lib.MODEL_EB and not (flags & _lib.FLAG_EVALUATE_EXCLUDED)
    t = inputs["grids"][grid][0]
    _row_order(True)
    for n in COUNTS:
        _call(inputs, grid, fam, n)
        counts, lists, blocks = _lib.debug_row_order()
        assert blocks.shape == (n, 19) and counts.shape == (BUCKETS, SHARDS)
        assert int(counts.sum()) == n
        filed = np.concatenate(lists)
        assert np.array_equal(np.sort(filed), np.arange(n)), "every row exactly once"
        bucket_of = np.empty(n, dtype=np.int64)
        for s, rows in enumerate(lists):
            bucket_of[rows] = s // SHARDS
            assert np.all((rows // 64) % SHARDS == s % SHARDS)        # a 64-row block files under shard (block & 3)
        # The keys, from the window the kernel used.  A row that the secondary rule excludes counts as never evaluated
        # when rowc_kernel itself settled it; one that sec_scan_kernel settled afterwards was filed under its window.
        none = np.zeros(n, dtype=bool)
        keys = _host_keys(blocks, t, none)
        if skipping:
            excl = blocks[:, I_EXCL] != 0.0
            keys = np.where(excl & (bucket_of == BUCKETS - 1), 0, keys)
        assert np.array_equal(_bucket(keys), bucket_of), (grid, key, n)
        for b in range(BUCKETS - 1):
            here, nxt = keys[bucket_of == b], keys[bucket_of > b]
            if here.size and nxt.size:
                assert here.min() >= nxt.max(), (b, n)
        assert np.all(bucket_of[keys == 0] == BUCKETS - 1)
        if n >= 1000:
            off = 1 if key == "eb" else 0            # (the EB block's first row is the excluded one)
            kh = keys[off:off + 6 + N_LADDER]
            assert kh[0] >= N_TIME - 1                   # the whole curve
            assert 0 < kh[1] < N_TIME                    # part of the span
            assert kh[2] == 0 and blocks[off + 2, I_WHI] > blocks[off + 2, I_WLO]      # a window, none of it in the span
            assert kh[3] == 0 and blocks[off + 3, I_WHI] < blocks[off + 3, I_WLO]      # no window
            assert kh[5] == 0 and np.isnan(blocks[off + 5, I_NMOT])                   # the NaN row
            assert np.isin(kh[6:], (1, 2)).any()         # the ladder reaches windows of one or two cells
            if key == "eb":
                assert blocks[0, I_EXCL] != 0.0
                assert (bucket_of[0] == BUCKETS - 1) == skipping


def test_a_captured_call_replays_to_the_bits_of_an_eager_one(inputs):
    n = 1000
    rows_d = _lib.dev(np.ascontiguousarray(inputs["eb"][:, :n]))
    eager = _call(inputs, "uniform", 1, n, rows_d=rows_d).cpu().numpy()
    out = torch.empty(n, dtype=torch.float64, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _call(inputs, "uniform", 1, n, out=out, rows_d=rows_d)              # warm-up
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _call(inputs, "uniform", 1, n, out=out, rows_d=rows_d)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint64), eager.view(np.uint64))
