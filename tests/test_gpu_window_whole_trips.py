"""Uniform time grids: pass 1 of cells_kernel's stencil instantiation files a 64-cell trip that lies wholly inside a transit
window as it stands, without looking at its cells (trx_cells.hpp, window_trips: the whole trips).

Whole trips are a subset of the trips whose every cell the per-cell test would file, so the in-window list is the same
cells in the same order and no output may move by a bit: every comparison between the switch on and off
(trx_set_whole_trips, testing library) is an equality of 64-bit patterns -- chi^2/2 of trx_lnl_batch, the flux grid, the
evaluation census.  Against the CPU oracle the project's bars hold: 1e-9 relative in chi^2/2, 5e-13 in flux.

Grids of 384 (six trips), 449 (a partial last trip) and 2113 points (a pass seam at 2048 and a partial trip), each at
0.12, 0.18 and 0.29 exposures per step.  Conjunction lies at cell 95.5 of every grid, so a circular row's window is
symmetric about the middle of trip 1 (cells 64 .. 127), and its half width in time follows from the window's own rule
(oracle/bench_window_skip.h: |X| < 1 + k on a circular orbit of radius a is the arc asin((1 + k) / a) either side of
conjunction, plus half an exposure): the rows are built for a window whose first and last cells are (64, 127) -- exactly
one trip --, (63, 128), (62, 129), (65, 126), (80, 111) -- shorter than a trip, strictly inside one --, the whole curve and
more, and (61, 130) at a period of 192 cells -- an epoch every three trips, a whole trip in each.  Edges sit half a cell
from the nearest stamp.  The tests read the window the kernel used from the row blocks (trx_debug_row_order) and check
those indices before anything else.  Further rows: a window that wraps round +-pi (an exposure as long as the orbit), a
NaN dilution (an ordinary window, a NaN result), a NaN period (no window arithmetic holds), a flat row (the body passes
the star by), and EB rows on both sides of the secondary rule.

Counters (trx_debug_whole_trips), one launch per row: whole + walked with the switch on equals walked with it off (the
trips that cannot hold an in-window cell are in neither: skipped = trips - walked); every trip with an in-window cell is
walked or whole; whole is at least the number of trips that lie two cells or more inside the window and at most the
number of trips all of whose cells are in-window cells, both counted here in float64 from the row block; whole is 0 for
the wrap-around and the NaN-period rows and for a launch that a stale memo sends to the stencil instantiation with
radius 0.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import oracle as O
from triceratops_amd import _lib, synth
from triceratops_amd.constants import Rearth, Rsun

pytestmark = pytest.mark.gpu

SIZES = (384, 449, 2113)
CADENCES = (0.12, 0.18, 0.29)
GRIDS = [(n, c) for n in SIZES for c in CADENCES]
IDS = ["%d-%.2f" % g for g in GRIDS]
CENTRE = 95.5                  # conjunction, in cells
PASS = 2048                    # cells of a window pass of the one-row kernel
TWO_PI = 6.283185307179586
RTOL_ORACLE = 1e-9
ATOL_FLUX = 5e-13
I_T0, I_NMOT, I_WLO, I_WHI, I_EXCL = 1, 2, 10, 11, 18      # RowC (trx_device.hpp)
K_TP, K_EB, K_EB_DEEP = 0.05, 0.3, 0.8

# (name, first, last) of the designed windows; None: the whole curve and five cells more on either side
DESIGNED = (("one-trip", 64, 127), ("one-spare", 63, 128), ("two-spare", 62, 129), ("one-short", 65, 126),
            ("inside", 80, 111), ("whole-curve", None, None))
TWO_EPOCHS = ("two-epochs", 61, 130, 192)      # ... and the period in cells


def _orbit_for(half_width, k, period=None):
    """(P, a / R_s) of a circular orbit whose window has this half width in time: n W = asin(R / a) + margin."""
    if period is None:
        period = TWO_PI * half_width / 0.2
    n = TWO_PI / period
    arc = n * half_width - (0.5 * n * synth.EXPTIME * (1.0 + 1e-9) + 1e-11)
    assert 0.0 < arc < 0.5 * np.pi, (half_width, period, arc)
    return period, ((1.0 + k) * (1.0 + 1e-9) + 1e-12) / np.sin(arc)


def _tp_row(k, per, b, a_R, fr=0.0):
    inc = np.degrees(np.arccos(b / a_R))
    return np.array([k * Rsun / Rearth, per, inc, a_R * Rsun, 1.0, 0.4, 0.25, 0.0, 0.0, fr])


def _eb_row(k, eb_fr, per, a_R):
    return np.array([k, eb_fr, per, 90.0, a_R * Rsun, 1.0, 0.4, 0.25, 0.0, 0.0, 0.0])


def _half_width(n_time, dt, first, last):
    if first is None:
        return (max(CENTRE, n_time - 1 - CENTRE) + 5.5) * dt
    assert first + last == 2 * CENTRE
    return 0.5 * (last - first + 1) * dt


def _build(n_time, cadence):
    dt = cadence * synth.EXPTIME
    t = (np.arange(n_time) - CENTRE) * dt
    tp, names, design = [], [], {}
    for name, first, last in DESIGNED:
        per, a_R = _orbit_for(_half_width(n_time, dt, first, last), K_TP)
        tp.append(_tp_row(K_TP, per, 0.0, a_R))
        names.append(name)
        design[name] = (first, last)
    name, first, last, cells = TWO_EPOCHS
    per, a_R = _orbit_for(_half_width(n_time, dt, first, last), K_TP, period=cells * dt)
    tp.append(_tp_row(K_TP, per, 0.0, a_R))
    names.append(name)
    per, a_R = _orbit_for(_half_width(n_time, dt, 63, 128), K_TP)
    tp.append(_tp_row(K_TP, 0.0015, 0.0, 1.5)); names.append("wrap")              # an exposure of 0.93 orbits
    tp.append(_tp_row(K_TP, per, 0.0, a_R, fr=np.nan)); names.append("nan-dilution")
    tp.append(_tp_row(K_TP, np.nan, 0.0, a_R)); names.append("nan-period")
    tp.append(_tp_row(K_TP, per, 1.5, a_R)); names.append("flat")
    eb = []
    for k, eb_fr in ((K_EB, 1e-5), (K_EB_DEEP, 0.4)):
        per, a_R = _orbit_for(_half_width(n_time, dt, 63, 128), k)
        eb.append(_eb_row(k, eb_fr, per, a_R))
    return {"t": t, "dt": dt, "tp": np.ascontiguousarray(np.stack(tp, axis=1)), "tp_names": names, "design": design,
            "eb": np.ascontiguousarray(np.stack(eb, axis=1)), "eb_names": ["eb-kept", "eb-excluded"]}


@pytest.fixture(scope="module")
def grids():
    """Built once and never changed: per grid the stamps, the rows, a noisy light curve of the (63, 128) row, and what
    the oracle says about all of it."""
    _lib.require_gpu()
    out = {}
    for gi, (n_time, cadence) in enumerate(GRIDS):
        g = _build(n_time, cadence)
        curve = O.flux_grid(O.MODEL_TP, g["t"], g["tp"][:, 1:2], exptime=synth.EXPTIME, nsamples=synth.NSAMPLES)[0][0]
        g["flux"] = synth.noisy_light_curve(np.random.default_rng(synth.SEED + 900 + gi), curve)
        for key, omodel in (("tp", O.MODEL_TP), ("eb", O.MODEL_EB)):
            g["oracle_h_" + key] = O.lnl_batch(omodel, g["t"], g["flux"], synth.SIGMA, g[key], exptime=synth.EXPTIME,
                                               nsamples=synth.NSAMPLES)
            g["oracle_grid_" + key] = O.flux_grid(omodel, g["t"], g[key], exptime=synth.EXPTIME, nsamples=synth.NSAMPLES)[0]
        g["t_d"], g["f_d"] = _lib.dev(g["t"]), _lib.dev(g["flux"])
        out[(n_time, cadence)] = g
    return out


BLOCKS = (("tp", _lib.MODEL_TP), ("eb", _lib.MODEL_EB))


def _whole_trips(on):
    assert _lib.lib().trx_set_whole_trips(1 if on else 0) == 0


def _lnl(g, model, rows_d, out=None):
    return _lib.lnl_batch(model, 0, g["t_d"], g["f_d"], synth.SIGMA, rows_d, synth.EXPTIME, synth.NSAMPLES, out=out)


def _in_window(block, tt):
    """The per-cell test of pass 1 in float64 (in_window, trx_device.hpp), from the row block's window."""
    t0, nmot, wlo, whi = block[I_T0], block[I_NMOT], block[I_WLO], block[I_WHI]
    with np.errstate(all="ignore"):
        ph = nmot * (tt - t0)
        d = ph - TWO_PI * np.rint(ph / TWO_PI)
        slack = 1e-15 * np.abs(ph)
        lo, hi = wlo - slack, whi + slack
        out = ((d < lo) & ~(d + TWO_PI <= hi)) | ((d > hi) & ~(d - TWO_PI >= lo))
    return ~out


def _trip_classes(block, g):
    """Per trip of the window passes: (any in-window cell, all cells in-window, ... and two cells more on either side)."""
    n = g["t"].size
    ext = (np.arange(-2, n + 2) - CENTRE) * g["dt"]
    inw = _in_window(block, ext)                      # cell j at inw[j + 2]
    some, full, deep = [], [], []
    for p0 in range(0, n, PASS):
        p1 = min(p0 + PASS, n)
        for s in range(p0, p1, 64):
            e = min(s + 64, p1)
            some.append(inw[s + 2:e + 2].any())
            full.append(inw[s + 2:e + 2].all())
            deep.append(inw[s:e + 4].all())
    return np.array(some), np.array(full), np.array(deep)


def _blocks(g, key, model):
    """The row blocks of a launch over all rows of the family, as the kernels read them (trx_debug_row_order)."""
    _lnl(g, model, _lib.dev(g[key]))
    blocks = _lib.debug_row_order()[2]
    assert blocks.shape == (g[key].shape[1], 19)
    return blocks


@pytest.mark.parametrize("grid", GRIDS, ids=IDS)
def test_the_rows_have_the_windows_they_were_built_for(grids, grid):
    g = grids[grid]
    n = g["t"].size
    blocks = _blocks(g, "tp", _lib.MODEL_TP)
    by_name = dict(zip(g["tp_names"], blocks))
    for name, (first, last) in g["design"].items():
        cells = np.flatnonzero(_in_window(by_name[name], g["t"]))
        # (the epoch at conjunction; the 2113-point grids are longer than the short rows' periods and see later epochs
        # too, at whatever places their periods put them)
        cells = cells[cells < CENTRE + np.pi / (by_name[name][I_NMOT] * g["dt"])]
        want = (0, n - 1) if first is None else (first, last)
        assert (cells[0], cells[-1]) == want and cells.size == want[1] - want[0] + 1, (name, cells[0], cells[-1])
    name, first, last, period = TWO_EPOCHS
    cells = np.flatnonzero(_in_window(by_name[name], g["t"]))
    want = np.concatenate([np.arange(first + m * period, last + m * period + 1) for m in range(-1, n // period + 1)])
    assert np.array_equal(cells, want[(want >= 0) & (want < n)]), name
    some, full, deep = _trip_classes(by_name[name], g)
    assert deep[1] and deep[4] and not full[0] and not full[2]                   # a whole trip in each epoch
    wrap = by_name["wrap"]
    assert wrap[I_WLO] <= -np.pi + 1e-6 or wrap[I_WHI] >= np.pi - 1e-6
    assert np.isnan(by_name["nan-period"][I_NMOT])
    assert not _trip_classes(by_name["inside"], g)[1][:3].any()                  # shorter than a trip: no whole trip there
    assert _trip_classes(by_name["one-trip"], g)[1][1] and not _trip_classes(by_name["one-trip"], g)[2][1]
    assert _trip_classes(by_name["whole-curve"], g)[2].all()                     # every trip whole
    eb = _blocks(g, "eb", _lib.MODEL_EB)
    assert eb[0, I_EXCL] == 0.0 and eb[1, I_EXCL] != 0.0                          # both sides of the secondary rule


@pytest.mark.parametrize("grid", GRIDS, ids=IDS)
def test_same_bits_with_whole_trips_on_and_off_and_the_oracle_bars(grids, grid):
    g = grids[grid]
    try:
        for key, model in BLOCKS:
            r_d = _lib.dev(g[key])
            got = {}
            for on in (True, False):
                _whole_trips(on)
                got[on] = (_lnl(g, model, r_d).cpu().numpy(),
                           _lib.flux_grid(model, 0, g["t_d"], r_d, synth.EXPTIME, synth.NSAMPLES, False)[0].cpu().numpy(),
                           _lib.flux_grid(model, _lib.FLAG_COUNT_EVALUATIONS, g["t_d"], r_d, synth.EXPTIME, synth.NSAMPLES,
                                          False)[0].cpu().numpy())
            for what, a, b in zip(("chi2/2", "flux grid", "census"), got[True], got[False]):
                assert np.array_equal(a.view(np.uint64), b.view(np.uint64)), (grid, key, what)
            h, flux, count = got[True]
            want = g["oracle_h_" + key]
            assert np.array_equal(np.isnan(want), np.isnan(h)) and np.array_equal(np.isposinf(want), np.isposinf(h))
            fin = np.isfinite(want)
            rel = np.abs(h[fin] - want[fin]) / np.abs(want[fin])
            wgrid = g["oracle_grid_" + key]
            # (the NaN-period row: NaN in chi^2/2 on both sides; which cells of its flux grid a NaN phase leaves at 1 is
            # not the oracle's to say)
            known = np.ones(wgrid.shape[0], dtype=bool)
            if key == "tp":
                known[g["tp_names"].index("nan-period")] = False
            assert np.array_equal(np.isnan(wgrid[known]), np.isnan(flux[known]))
            gfin = np.isfinite(wgrid)
            err = np.abs(flux[gfin] - wgrid[gfin]).max()
            print("%s %s: chi2/2 vs oracle %.3g, flux vs oracle %.3g" % (IDS[GRIDS.index(grid)], key, rel.max(), err))
            assert rel.max() < RTOL_ORACLE, (grid, key, rel.max())
            assert err < ATOL_FLUX, (grid, key, err)
            if key == "tp":
                names = g["tp_names"]
                assert np.isnan(h[names.index("nan-dilution")]) and np.isnan(h[names.index("nan-period")])
                assert np.all(wgrid[names.index("flat")] == 1.0) and count[names.index("flat")].max() == 0.0
                assert np.any(count == 1.0)                   # the stencil instantiation: a cell that cost its centre alone
            else:
                assert np.isfinite(h[0]) and np.isposinf(h[1])
    finally:
        _whole_trips(True)


def _counted_launch(g, model, rows_d, on):
    """chi^2/2 and (whole, walked) of one launch (trx_debug_whole_trips)."""
    _whole_trips(on)
    _lib.debug_whole_trips(reset=True)
    h = _lnl(g, model, rows_d).cpu().numpy()
    return h, _lib.debug_whole_trips(reset=True)


@pytest.mark.parametrize("grid", GRIDS, ids=IDS)
def test_the_counters_against_the_window_in_float64(grids, grid):
    g = grids[grid]
    n = g["t"].size
    trips = sum((min(p0 + PASS, n) - p0 + 63) // 64 for p0 in range(0, n, PASS))
    try:
        for key, model in BLOCKS:
            blocks = _blocks(g, key, model)
            for r, name in enumerate(g[key + "_names"]):
                r_d = _lib.dev(np.ascontiguousarray(g[key][:, r:r + 1]))
                h_on, (whole, walked) = _counted_launch(g, model, r_d, True)
                h_off, (whole_off, walked_off) = _counted_launch(g, model, r_d, False)
                assert np.array_equal(h_on.view(np.uint64), h_off.view(np.uint64)), (grid, name)
                some, full, deep = _trip_classes(blocks[r], g)
                assert some.size == trips
                print("%s %s: trips %d, walked %d -> whole %d + walked %d; float64: any %d, all %d, two cells inside %d"
                      % (IDS[GRIDS.index(grid)], name, trips, walked_off, whole, walked, some.sum(), full.sum(), deep.sum()))
                assert whole_off == 0
                if name == "eb-excluded":                       # never evaluated: no pass 1
                    assert (whole, walked, walked_off) == (0, 0, 0)
                    continue
                assert whole + walked == walked_off               # + skipped (= trips - walked_off) == trips
                assert some.sum() <= walked_off <= trips
                if name in ("wrap", "nan-period"):
                    assert whole == 0 and walked == trips
                    continue
                assert deep.sum() <= whole <= full.sum(), (grid, name, whole)
                if name == "whole-curve":
                    assert whole == trips and walked == 0
                if name == "inside" and n < PASS:                # (one epoch in the short grids, and that inside trip 1)
                    assert full.sum() == 0 and whole == 0
                if name == "two-epochs":
                    assert whole >= 2
                if name in ("one-trip", "one-spare", "two-spare", "nan-dilution"):
                    assert whole >= 1                              # (edges half a cell off the stamps: far beyond the margin)
    finally:
        _whole_trips(True)


def test_a_stale_memo_with_radius_zero_files_no_whole_trip(grids):
    """The stencil instantiation on stamps that are no uniform grid: a first launch on a uniform grid leaves the verdict
    "stencil" under the light curve's address, the stamps at that address are then replaced by jittered ones, and the next
    launch enqueues the stencil instantiation alone, which finds radius 0 and walks every trip."""
    g = grids[(384, 0.18)]
    n = g["t"].size
    rng = np.random.default_rng(synth.SEED + 950)
    jittered = np.sort(g["t"] + rng.uniform(-0.3, 0.3, n) * g["dt"])
    r_d = _lib.dev(g["tp"][:, :6].copy())
    rows = 6
    got = {}
    try:
        for on in (True, False):
            t_d = _lib.dev(g["t"].copy())
            stale = dict(g, t_d=t_d)
            _whole_trips(on)
            for _ in range(2):                                # (the second: whatever verdict the address held before)
                _lnl(stale, _lib.MODEL_TP, r_d).cpu()
            t_d.copy_(torch.from_numpy(jittered))
            torch.cuda.synchronize()
            _lib.debug_whole_trips(reset=True)
            got[on] = _lnl(stale, _lib.MODEL_TP, r_d).cpu().numpy()
            whole, walked = _lib.debug_whole_trips(reset=True)
            assert whole == 0 and walked == rows * ((n + 63) // 64), (on, whole, walked)
        assert np.array_equal(got[True].view(np.uint64), got[False].view(np.uint64))
        want = O.lnl_batch(O.MODEL_TP, jittered, g["flux"], synth.SIGMA, g["tp"][:, :6], exptime=synth.EXPTIME,
                           nsamples=synth.NSAMPLES)
        assert np.max(np.abs(got[True] - want) / np.abs(want)) < RTOL_ORACLE
    finally:
        _whole_trips(True)


def test_a_captured_call_replays_to_the_bits_of_an_eager_one(grids):
    """(the default queue count; the graph holds rowc_kernel, the memset of the order's counters and both instantiations)"""
    g = grids[(2113, 0.18)]
    r_d = _lib.dev(g["tp"])
    n = g["tp"].shape[1]
    eager = _lnl(g, _lib.MODEL_TP, r_d).cpu().numpy()
    out = torch.empty(n, dtype=torch.float64, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _lnl(g, _lib.MODEL_TP, r_d, out=out)              # warm-up
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _lnl(g, _lib.MODEL_TP, r_d, out=out)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint64), eager.view(np.uint64))
    _whole_trips(False)
    try:
        off = _lnl(g, _lib.MODEL_TP, r_d).cpu().numpy()
    finally:
        _whole_trips(True)
    assert np.array_equal(off.view(np.uint64), eager.view(np.uint64))
