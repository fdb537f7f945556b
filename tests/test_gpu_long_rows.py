"""Light curves longer than one window pass of cells_kernel's one-row-per-wave instantiations (csrc/trx_cells.hpp,
cells_body: `for (win0 = 0; win0 < ncell; win0 += wstep)`, TRX_CELLS_WINDOW = 2048 cells).  Every pass rebuilds the
in-window list, the stencil's carry, the heavy-cell list and the bitmap of window_trips, reads the launch header's trip
sums at kHdrTrip + (win0 >> 6) + lane, and -- bounded evaluation -- runs a probe phase and a verdict of its own; the row's
chi^2 (lacc) is carried across the passes.  The rest of the suite has one cell in a second pass at most where that
matters (tests/test_gpu_window_trips.py: 2049 points).

Which shape reaches what (SEAM = a multiple of 2048; t = 0, the conjunction of every row, lies at cell 2047.5 + shift, and
half the TP rows and every third EB row have the period 2048 dt / m, m = 1 .. 4, so that a conjunction lies at EVERY seam):
  uniform 4096 / 4097 / 4500 / 6209 stamps at 0.12, 0.18, 0.29 exposures per step (np.linspace: the launch header takes
        stamps within 4 ulp of t0 + j dt) -- cells_kernel<.., LONG, ST>: window_trips and the trip sums of passes 2 - 4 (4096: two
        full passes and nothing behind them; 4097: a pass of one cell; 4500: a pass of six trips and 20 cells; 6209: a
        fourth pass of one trip and one cell), the stencil's carry reset at a seam -- the kStM = 8 cells on either side of it
        have no neighbours beyond it and take their own nodes through the lazy tiers --, contact cells of the second sweep
        next to a seam (shift +13, -5);
  the same grids jittered by +-0.4 steps and sorted (4097, 4500) -- cells_kernel<.., LONG> without the stencil: the carried
        cells (kCarry) and the heavy list across passes;
  70 001 jittered stamps, 8 rows -- 35 passes, cell numbers above 65 535 (the in-window list holds 16-bit offsets from
        win0), a conjunction on the seam 65 536;
  trx_lnl_batch_weighted on the 4500-point grids -- cells_kernel<.., LONG, [ST,] WT>, weights that are zero except within
        40 cells of a seam;
  trx_set_debug_bounded_lnl(1) and trx_lnz_scenario -- cells_kernel<.., LONG, PRUNE>: the probe phase and the verdict of
        every pass, the bound carried over;
  calc_probs_many at 2300 points and calc_probs_datasets at 2600 -- the launch chains and the dataset layer on two passes.

Conditions on the INPUTS, asserted on the oracle's grid when a case is made, before anything is compared (_conditions):
at every seam at least 20 TP rows are below 1 in both cells s - 1 and s (28 .. 71 on these cases), and at least 3 have a
limb contact within kStM cells of it -- some but not all of the cells s - 9 .. s + 8 below 1 (8 .. 21; the block's six
short transits see to it at a shift of 0, where the other rows' contacts lie further out); the EB block at least 20 and 3
straddling rows at the first and the later seams.  The 70 001-point case has 8 rows: a transit on the seam 65 536 and
transits behind it.

Bars -- none chosen here -- and the largest value measured on an MI355X next to each:
  ATOL_FLUX = 5e-13       device flux against the oracle (tests/test_gpu_kernels.py): 6.6e-14 within 16 cells of a seam,
                          5.5e-14 elsewhere (EB rows; TP 1.3e-14 and 1.2e-14)
  3e-13                   stencil against no stencil / every sub-exposure
                          (test_gpu_kernels.py::test_centre_value_stencil_on_dense_uniform_grids): 1.3e-15 / 7.8e-14 next to a
                          seam, 4.0e-15 / 5.0e-14 elsewhere; the same stamps at other cell numbers (test 4): 2.6e-15 with the
                          stencil, 5.6e-16 without
  RTOL_H = 1e-9           chi^2/2 against the oracle (tests/test_gpu_kernels.py): 8.2e-14; 70 001 points 1.0e-14; the seam
                          cells alone 5.3e-13
  max(1e-12, 2.2e-16 n)   chi^2/2 against the host's extended-precision sum over the device's own flux grid: both add the
                          same n non-negative terms, the kernel in some order in fp64 -- each partial sum is rounded once,
                          relative error <= (n - 1) x 1.1e-16 of the total whatever the order -- and the two orders a
                          kernel may choose (lanes, then passes) make it 2 x 1.1e-16 x n; the project's 1e-12
                          (tests/test_gpu_window_trips.py, RTOL_DIRECT) up to 4500 points: 2.7e-16
  RTOL_ROUTES = 1e-12     trx_lnl_batch_weighted against trx_flux_grid + trx_chi2_grid_weighted
                          (tests/test_gpu_lnl_weighted.py): 2.9e-16
  bounded evaluation      tests/test_gpu_bounded.py: exact to 1e-11 relative or a lower bound above hmin + 90 - 1e-6 (two rows
                          in three abandoned at 4097 and 4500 points, one in four of the 1500 per family at 70 001); lnZ to
                          1e-13 relative: 2.0e-16, the three bounded runs the same bits
  end to end              |d lnZ| <= 1e-12 hmax + 1e-12 (tests/test_gpu_lnl_weighted.py): 2.3e-13, 1.6e-4 of the bound
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import oracle as O
from triceratops_amd import _lib, synth

pytestmark = pytest.mark.gpu

WINDOW = 2048                 # TRX_CELLS_WINDOW
ST_M = 8                      # kStM
ATOL_FLUX = 5e-13
ATOL_STENCIL = 3e-13
RTOL_H = 1e-9
RTOL_ROUTES = 1e-12
INF = float("inf")
RSUN, REARTH = 69570000000.0, 637810000.0
BLOCKS = (("tp", _lib.MODEL_TP), ("eb", _lib.MODEL_EB))
# (stamps, step / exposure, shift of conjunction against the seam in cells): every length, every spacing and every shift
UNIFORM = ((4096, 0.18, 0), (4097, 0.12, 0), (4097, 0.29, -5), (4500, 0.18, 0), (4500, 0.12, -5), (4500, 0.29, 13),
           (6209, 0.18, 13), (6209, 0.29, 0), (6209, 0.12, -5))
IRREGULAR = ((4097, 0.18, 0), (4500, 0.18, -5))
HUGE = (70001, 0.18, 0)
_ID = lambda c: "%d-u%.2f-s%+d" % c


def _seams(n_time):
    return list(range(WINDOW, n_time, WINDOW))


def _stamps(n_time, u, shift, irregular):
    dt = u * synth.EXPTIME
    first = -(WINDOW - 0.5 + shift) * dt
    t = np.linspace(first, first + (n_time - 1) * dt, n_time)
    if irregular:
        rng = np.random.default_rng(synth.SEED + 900 + n_time)
        t = np.sort(t + rng.uniform(-0.4, 0.4, n_time) * dt)
    return t, dt


def _tp_block(rng, n, dt):
    """TP rows [10][<= n + 3] in the style of tests/golden/make_window_trips.py::tp_block: the first half with the periods
    2048 dt / m, m = 1 .. 4 (a conjunction on every seam), the rest log-uniform from 0.05 to 40 d; a / R log-uniform from
    1.5 to 40, half the rows eccentric up to 0.9, inclinations from 80 to 90 degrees; then that generator's two flat rows
    and its row whose dilution is NaN"""
    R_s = rng.uniform(0.3, 2.0, n)
    k = rng.uniform(0.02, 0.4, n)
    free = 10 ** rng.uniform(np.log10(0.05), np.log10(40.0), n)
    per = np.where(np.arange(n) < n // 2, WINDOW * dt / (1 + np.arange(n) % 4), free)
    a_R = 10 ** rng.uniform(np.log10(1.5), np.log10(40.0), n)
    ecc = np.where(rng.random(n) < 0.5, 0.0, rng.uniform(0.0, 0.9, n))
    argp = rng.uniform(0.0, 360.0, n)
    inc = rng.uniform(80.0, 90.0, n)
    rows = np.stack([k * R_s * RSUN / REARTH, per, inc, a_R * R_s * RSUN, R_s, rng.uniform(0.1, 0.6, n),
                     rng.uniform(0.05, 0.4, n), ecc, argp, np.where(rng.random(n) < 0.5, 0.0, rng.uniform(0.01, 0.5, n))])
    rows = rows[:, a_R * (1.0 - ecc) > 1.0 + k]
    # six short transits on every seam (m = 3, 4), five cells from first to last contact -- with the exposure's 1 / u cells
    # fewer than the 2 kStM + 2 cells around a seam, so that a limb contact lies next to it at every shift: circular, impact
    # parameters 0.5 .. 0.85, a / R from the duration (27 .. 40)
    short = rows[:, :6].copy()
    m = 3.0 + np.arange(6) % 2
    b = np.array([0.5, 0.7, 0.85])[np.arange(6) % 3]
    ks = 0.05 + 0.03 * np.arange(6)
    a_Rs = WINDOW * np.sqrt((1.0 + ks) ** 2 - b ** 2) / (m * np.pi * 5.0)
    short[0] = ks * short[4] * RSUN / REARTH
    short[1] = WINDOW * dt / m
    short[2] = np.degrees(np.arccos(b / a_Rs))
    short[3] = a_Rs * short[4] * RSUN
    short[7] = 0.0
    rows = np.concatenate([rows, short], axis=1)
    special = rows[:, :3].copy()
    special[1] = (3.0, 17.0, 3.0)                 # periods
    special[2] = (60.0, 55.0, 89.0)               # inclinations: the first two pass the star by
    special[3] = 12.0 * special[4] * RSUN
    special[7] = 0.0
    special[9] = (0.0, 0.2, 1.0)                  # companion flux ratio 1: an infinite dilution, NaN
    return np.ascontiguousarray(np.concatenate([rows, special], axis=1))


def _eb_block(rng, n, dt):
    """synth.eb_rows(has_companion=True) -- both sides of the secondary-eclipse rule --, every third row with a period of
    2048 dt / m in place of its own"""
    rows = synth.eb_rows(rng, n, has_companion=True)
    rows[2, ::3] = WINDOW * dt / (1 + np.arange(rows[2, ::3].size) % 4)
    return np.ascontiguousarray(rows)


def _census(grid, n_time):
    """per seam: (seam, rows below 1 in both cells next to it, rows with a limb contact within kStM cells of it)"""
    low = grid < 1.0
    out = []
    for s in _seams(n_time):
        near = low[:, s - ST_M - 1:min(n_time, s + ST_M + 1)]
        out.append((s, int((low[:, s - 1] & low[:, s]).sum()), int((near.any(axis=1) & ~near.all(axis=1)).sum())))
    return out


def _conditions(c):
    census = _census(c["tp"]["grid"], c["n_time"])
    print("%s: (seam, straddling TP rows, TP rows with a contact next to it) %s" % (c["name"], census))
    if c["n_time"] == HUGE[0]:
        # 8 rows: a transit on the seam 65 536 and transits behind it
        low = c["tp"]["grid"] < 1.0
        assert (low[:, 65535] & low[:, 65536]).any() and low[:, 65536 + 100:].any()
        return
    for s, straddling, contacts in census:
        assert straddling >= 20 and contacts >= 3, (c["name"], s, straddling, contacts)
    # (the EB block: eclipses on the first seam -- every row's conjunction -- and on the later ones)
    for s, straddling, _ in _census(c["eb"]["grid"], c["n_time"]):
        assert straddling >= (20 if s == WINDOW else 3), (c["name"], "eb", s, straddling)


_cases = {}


def _case(n_time, u, shift, irregular=False):
    """stamps, a noisy light curve with a transit on every seam, the two blocks with the oracle's grids and secondary
    depths, everything on the device; made once, its input conditions asserted then"""
    key = (n_time, u, shift, irregular)
    if key not in _cases:
        rng = np.random.default_rng(5 + n_time + int(100 * u) + shift)
        t, dt = _stamps(n_time, u, shift, irregular)
        ref = synth.reference_tp_row()
        ref[1] = WINDOW * dt
        flux = synth.noisy_light_curve(rng, O.flux_grid(O.MODEL_TP, t, ref)[0][0])
        huge = n_time == HUGE[0]
        c = dict(name="%s%s" % (_ID((n_time, u, shift)), "-irr" if irregular else ""), n_time=n_time, dt=dt, t=t, flux=flux,
                 t_d=_lib.dev(t), f_d=_lib.dev(flux))
        tp = _tp_block(rng, 90, dt)
        if huge:
            # 8 rows: two with a period of 2048 dt / m, one with a period of its own, two short ones, the flat ones, NaN
            last = tp.shape[1] - 1
            tp = np.ascontiguousarray(tp[:, [0, 1, last - 9, last - 8, last - 7, last - 2, last - 1, last]])
        for key_b, rows in (("tp", tp), ("eb", _eb_block(rng, 8 if huge else 64, dt))):
            grid, sec = O.flux_grid(O.MODEL_TP if key_b == "tp" else O.MODEL_EB, t, rows)
            c[key_b] = dict(rows=rows, rows_d=_lib.dev(rows), grid=grid, sec=sec)
        if huge:
            assert c["tp"]["rows"].shape[1] == 8
        _conditions(c)
        _cases[key] = c
    return _cases[key]


def _half_chi2(flux, grid, w):
    """0.5 sum_t w_t (flux_t - grid_rt)^2 per row in extended precision"""
    d = flux.astype(np.longdouble)[None, :] - grid.astype(np.longdouble)
    return np.asarray(0.5 * np.sum(d * d * np.asarray(w, dtype=np.longdouble), axis=1), dtype=np.float64)


def _rel(got, want, what):
    assert np.array_equal(np.isposinf(want), np.isposinf(got)), what
    assert np.array_equal(np.isnan(want), np.isnan(got)), what
    fin = np.isfinite(want)
    return float((np.abs(got[fin] - want[fin]) / np.maximum(np.abs(want[fin]), 1e-300)).max()) if fin.any() else 0.0


def _near_seams(n_time, reach):
    m = np.zeros(n_time, dtype=bool)
    for s in _seams(n_time):
        m[max(0, s - reach):s + reach] = True
    return m


def _grid(c, key, model, flags, t_d=None):
    return _lib.flux_grid(model, flags, c["t_d"] if t_d is None else t_d, c[key]["rows_d"], synth.EXPTIME, synth.NSAMPLES,
                          False)[0].cpu().numpy()


# ---------------------------------------------------------------------------------------
# 1. the flux grid across the seams, stencil on
@pytest.mark.parametrize("shape", UNIFORM, ids=_ID)
def test_flux_grid_across_the_seams_with_the_stencil(shape):
    c = _case(*shape)
    n_time = c["n_time"]
    seam32 = _near_seams(n_time, 16)
    for key, model in BLOCKS:
        want = c[key]["grid"]
        on, off, every, count = (_grid(c, key, model, f) for f in (0, _lib.FLAG_NO_STENCIL, _lib.FLAG_ALL_SUBEXPOSURES,
                                                                   _lib.FLAG_COUNT_EVALUATIONS))
        # the stencil ran in the passes behind the first, and nowhere within kStM cells of a seam
        single = count == 1.0
        # (pass 3: the TP block, whose rows of period 2048 dt / m cross the disc slowly enough there; the EB rows that
        # meet a later seam do so with a short period on a wide orbit, every cell of the eclipse next to a contact)
        passes = [p for p in ((1, 2) if key == "tp" else (1,)) if (p + 1) * WINDOW <= n_time or n_time - p * WINDOW >= 256]
        for p in passes:
            assert single[:, p * WINDOW:(p + 1) * WINDOW].any(), (c["name"], key, "no stencil cell in pass %d" % (p + 1))
        assert single[:, :WINDOW].any()
        assert not single[:, _near_seams(n_time, ST_M)].any(), (c["name"], key)
        # ... where the cells of a transit take nodes of their own instead
        assert (count[:, _near_seams(n_time, ST_M)] >= 3.0).any()
        if key == "tp":
            assert count[-3:-1].max() == 0.0                         # the flat rows cost nothing
        assert np.array_equal(np.isnan(want), np.isnan(on))
        fin = np.isfinite(want)
        d = np.where(fin, np.abs(on - want), 0.0)
        print("%s %s: |flux - oracle| max %.3g within 16 cells of a seam, %.3g elsewhere"
              % (c["name"], key, d[:, seam32].max(), d[:, ~seam32].max()))
        assert d.max() < ATOL_FLUX, (c["name"], key, d.max())
        for name, other in (("no stencil", off), ("every sub-exposure", every)):
            assert np.array_equal(np.isnan(on), np.isnan(other)) and np.array_equal(on == 1.0, other == 1.0), (key, name)
            d = np.where(np.isnan(on), 0.0, np.abs(on - other))
            print("%s %s: |stencil - %s| max %.3g within 16 cells of a seam, %.3g elsewhere"
                  % (c["name"], key, name, d[:, seam32].max(), d[:, ~seam32].max()))
            assert d.max() < ATOL_STENCIL, (c["name"], key, name, d.max())


# ---------------------------------------------------------------------------------------
# 2. chi^2 across the seams: the stencil instantiation (uniform) and the plain one-row one (irregular)
@pytest.mark.parametrize("shape,irregular", [(s, False) for s in UNIFORM] + [(s, True) for s in IRREGULAR + (HUGE,)],
                         ids=[_ID(s) for s in UNIFORM] + [_ID(s) + "-irr" for s in IRREGULAR + (HUGE,)])
def test_chi2_across_the_seams(shape, irregular):
    c = _case(*shape, irregular=irregular)
    n_time = c["n_time"]
    w = np.full(n_time, 1.0 / synth.SIGMA ** 2)
    for key, model in BLOCKS:
        b = c[key]
        got = _lib.lnl_batch(model, _lib.FLAG_FULL_EVALUATION, c["t_d"], c["f_d"], synth.SIGMA, b["rows_d"], synth.EXPTIME,
                             synth.NSAMPLES).cpu().numpy()
        want = _half_chi2(c["flux"], b["grid"], w)
        if key == "eb":
            want[~(b["sec"] < 1.5 * synth.SIGMA)] = np.inf           # the oracle's rule (oracle/trx_oracle.c)
        r_oracle = _rel(got, want, (c["name"], key, "oracle"))
        print("%s %s: chi^2/2 against the oracle %.3g" % (c["name"], key, r_oracle))
        assert r_oracle < RTOL_H, (c["name"], key, r_oracle)
        if n_time != HUGE[0]:
            host = _half_chi2(c["flux"], _grid(c, key, model, 0), w)
            host[np.isposinf(got)] = np.inf
            r_host = _rel(got, host, (c["name"], key, "host sum"))
            print("%s %s: chi^2/2 against the host's sum over the device's grid %.3g" % (c["name"], key, r_host))
            assert r_host < max(1e-12, 2.2e-16 * n_time), (c["name"], key, r_host)
        if key == "tp":
            flat = np.all(b["grid"] == 1.0, axis=1)
            assert flat[-3] and flat[-2]
            assert np.unique(got[flat].view(np.uint64)).size == 1
            assert np.isnan(got[-1])
        else:
            assert np.isposinf(got).any() and np.isfinite(got).any()         # both sides of the secondary-eclipse rule


# ---------------------------------------------------------------------------------------
# 3. chi^2 of the cells next to the seams alone
@pytest.mark.parametrize("shape,irregular", [(UNIFORM[3], False), (IRREGULAR[1], True)], ids=["uniform", "irregular"])
def test_seam_weighted_chi2(shape, irregular):
    """weights 1 / sigma^2 within 40 cells of a seam and 0 elsewhere: a seam cell wrong by 1e-9 in flux hides in a
    whole-curve chi^2 at 1e-9 relative; here it weighs 4500 / 160 times as much"""
    c = _case(*shape, irregular=irregular)
    n_time = c["n_time"]
    assert n_time == 4500
    w = np.where(_near_seams(n_time, 40), 1.0 / synth.SIGMA ** 2, 0.0)
    assert int((w > 0).sum()) == 160
    w_d = _lib.dev(w)
    for key, model in BLOCKS:
        b = c[key]
        limit = 1.5 * synth.SIGMA if key == "eb" else INF
        got_d = _lib.lnl_batch_weighted(model, 0, c["t_d"], c["f_d"], w_d, b["rows_d"], synth.EXPTIME, synth.NSAMPLES, limit)
        got = got_d.cpu().numpy()
        want = _half_chi2(c["flux"], b["grid"], w)
        if key == "eb":
            want[b["sec"] >= limit] = np.inf
            assert 0 < np.isposinf(want).sum() < want.size
        r_oracle = _rel(got, want, (c["name"], key, "oracle"))
        grid, sec = _lib.flux_grid(model, 0, c["t_d"], b["rows_d"], synth.EXPTIME, synth.NSAMPLES)
        route = _lib.chi2_grid_weighted(c["f_d"], w_d, grid, sec if key == "eb" else None, limit).cpu().numpy()
        r_route = _rel(got, route, (c["name"], key, "grid route"))
        print("%s %s, seam cells only: against the oracle %.3g, against the grid route %.3g" % (c["name"], key, r_oracle, r_route))
        assert r_oracle < RTOL_H and r_route < RTOL_ROUTES, (c["name"], key, r_oracle, r_route)
        # the accumulate form: the values are added to `out`, and +inf stays +inf
        rng = np.random.default_rng(3)
        pre = rng.uniform(0.0, 1e4, got.size)
        pre[1] = np.inf
        pre_d = _lib.dev(pre)
        acc = _lib.lnl_batch_weighted(model, 0, c["t_d"], c["f_d"], w_d, b["rows_d"], synth.EXPTIME, synth.NSAMPLES, limit,
                                      out=pre_d.clone())
        acc = acc.cpu().numpy()
        assert np.array_equal(acc, pre + got, equal_nan=True), (c["name"], key)
        assert np.isposinf(acc[1])
        if key == "tp":
            assert np.isnan(got[-1]) and np.isnan(acc[-1])


# ---------------------------------------------------------------------------------------
# 4. the same stamps at other cell numbers
@pytest.mark.parametrize("shape,irregular", [(IRREGULAR[1], True), (UNIFORM[3], False)], ids=["irregular", "uniform"])
def test_a_cell_does_not_depend_on_where_the_seams_fall(shape, irregular):
    """flux_grid on t and on t[s:]: the seams of the second call lie s cells later in the light curve.  A cell's value
    depends on its row and its stamp alone, but NOT bit for bit: measured on an MI355X, 3 .. 130 of 400 000 cells of the
    irregular grid differ, by one or two ulp (<= 3.4e-16), with the same number of evaluations in either call, and they
    are cells whose place in the in-window list changed (behind a seam for s = 64, everywhere for s = 1).  A cell's node
    terms are added to its sum in LDS (ds_add_f64) by the lanes that hold its (cell, node) pairs, 64 pairs per trip of
    the pair loop: where the pairs fall in the trips -- all in one instruction, or split between two -- follows from the
    cell's place in its chunk, and the grouping of a sum of 3 .. 20 terms decides its last bit.  Results repeat from run
    to run; they are not invariant under a renumbering of the cells.  Hence 3e-13, the bar between the stencil and a
    cell's own nodes (test_gpu_kernels.py::test_centre_value_stencil_on_dense_uniform_grids), on both kinds of grid --
    on the uniform one other cells lose their stencil neighbours as well -- and a count: a seam defect would move whole
    runs of cells, reordered sums move a cell here and there (fewer than 1 in 1000)."""
    c = _case(*shape, irregular=irregular)
    for key, model in BLOCKS:
        whole = _grid(c, key, model, 0)
        for s in (1, 37, 64, 1000):
            part = _grid(c, key, model, 0, _lib.dev(c["t"][s:]))
            a, b = whole[:, s:], part
            assert np.array_equal(np.isnan(a), np.isnan(b)), (key, s)
            assert np.array_equal(a == 1.0, b == 1.0), (key, s)
            ok = ~np.isnan(a)
            d = float(np.abs(a[ok] - b[ok]).max())
            moved = int((a[ok] != b[ok]).sum())
            print("%s %s, stamps from %d on: max |difference| %.3g, %d of %d cells not the same bits"
                  % (c["name"], key, s, d, moved, int(ok.sum())))
            assert d < ATOL_STENCIL, (key, s, d)
            if irregular:
                assert moved < 1e-3 * ok.sum(), (key, s, moved)


# ---------------------------------------------------------------------------------------
# 5. bounded evaluation, one row per wave, several passes
def _bounded_light_curve(shape, irregular):
    t, dt = _stamps(*shape, irregular)
    rng = np.random.default_rng(11 + shape[0])
    t_d = _lib.dev(t)
    curve, _ = _lib.flux_grid(0, 0, t_d, _lib.dev(synth.reference_tp_row()), synth.EXPTIME, 20, False)
    flux = synth.noisy_light_curve(rng, curve[0].cpu().numpy())
    return rng, t_d, flux, _lib.dev(flux)


@pytest.mark.parametrize("shape,irregular,n,fp32", [(IRREGULAR[0], True, 6000, False), (UNIFORM[3], False, 6000, False),
                                                    (HUGE, True, 1500, False), (UNIFORM[3], False, 6000, True)],
                         ids=["4097-irr", "4500", "70001-irr", "4500-fp32"])
def test_every_long_row_is_exact_or_a_valid_bound(shape, irregular, n, fp32):
    """tests/test_gpu_bounded.py::test_every_row_is_exact_or_a_valid_bound on light curves of several window passes: per row
    the full chi^2/2, or a lower bound of it above min + 90; the count of bounds is trx_pruned_rows; rows within 90 of the
    best are exact; the same argmin.  fp32: the same rules against the fp64 evaluation, with "exact" meaning within the
    fp32 model's slack sum_t w |r_t| eps + n_time eps^2 w / 2, eps = 2e-6
    (tests/test_gpu_lnl_weighted.py::test_fp32_model_flag_reaches_the_weighted_kernel) -- see the comment below."""
    L = _lib.lib()
    rng, t_d, flux, f_d = _bounded_light_curve(shape, irregular)
    n_time = shape[0]
    cnt = ctypes.c_ulonglong(0)
    total = 0
    try:
        for fam in synth.FAMILIES[:6]:
            rows = synth.family_rows(rng, fam, n)
            rows[:, :3] = rows[:, 3:6]                  # ties
            rows[7 if fam[1] == _lib.MODEL_TP else 8, 5] = np.nan      # a draw with NaN eccentricity
            rows_d = _lib.dev(rows)
            flags = (_lib.FLAG_COMPANION_IS_HOST if fam[2] else 0) | (_lib.FLAG_FP32_MODEL if fp32 else 0)
            L.trx_set_debug_bounded_lnl(0)
            full = _lib.lnl_batch(fam[1], flags, t_d, f_d, synth.SIGMA, rows_d, synth.EXPTIME, 20).cpu().numpy()
            L.trx_set_debug_bounded_lnl(1)
            L.trx_pruned_rows(ctypes.byref(cnt), 1)
            got = _lib.lnl_batch(fam[1], flags, t_d, f_d, synth.SIGMA, rows_d, synth.EXPTIME, 20).cpu().numpy()
            L.trx_pruned_rows(ctypes.byref(cnt), 1)
            total += cnt.value
            assert np.array_equal(np.isnan(full), np.isnan(got))
            assert np.array_equal(full == np.inf, got == np.inf)
            fin = np.isfinite(full)
            if not fp32:
                hmin = full[fin].min()
                exact = np.zeros(n, dtype=bool)
                exact[fin] = np.abs(got[fin] - full[fin]) <= 1e-11 * np.abs(full[fin])
                bound = fin & ~exact
                assert int(bound.sum()) == cnt.value, fam[0]
                assert np.all(got[bound] <= full[bound] * (1 + 1e-9)), fam[0]
                assert np.all(got[bound] > hmin + 90.0 - 1e-6), fam[0]
                assert np.all(exact[fin & (full <= hmin + 90.0)]), fam[0]
                assert np.argmin(np.where(fin, got, np.inf)) == np.argmin(np.where(fin, full, np.inf)), fam[0]
                continue
            # fp32 model.  The reference is the fp64 one: the full evaluation of a uniform grid takes the stencil and the
            # bounded one has no stencil instantiation, so with the fp32 flag the two differ by the fp32 model's error
            # in every cell, not by 1e-11.  slack_r = sum_t w |r_t| eps + n_time eps^2 w / 2 bounds |h32_r - h64_r| for
            # either; the kernel abandons a row above (the smallest fp32 value so far) + 90, and every fp32 value is at
            # least hlow = min_r (h64_r - slack_r).
            L.trx_set_debug_bounded_lnl(0)
            fp64 = _lib.lnl_batch(fam[1], flags & ~_lib.FLAG_FP32_MODEL, t_d, f_d, synth.SIGMA, rows_d, synth.EXPTIME,
                                  20).cpu().numpy()
            grid = _lib.flux_grid(fam[1], flags & ~_lib.FLAG_FP32_MODEL, t_d, rows_d, synth.EXPTIME, 20, False)[0]
            eps, w = 2e-6, 1.0 / synth.SIGMA ** 2
            slack = ((f_d[None, :] - grid).abs().sum(dim=1) * (w * eps) + 0.5 * n_time * eps ** 2 * w).cpu().numpy()
            del grid
            assert np.array_equal(np.isfinite(fp64), fin), fam[0]
            assert not np.array_equal(full[fin], fp64[fin])                  # the flag is not ignored
            assert (np.abs(full[fin] - fp64[fin]) <= slack[fin]).all(), fam[0]
            hlow = (fp64[fin] - slack[fin]).min()
            exact = np.zeros(n, dtype=bool)
            exact[fin] = np.abs(got[fin] - fp64[fin]) <= slack[fin]
            bound = fin & ~exact
            print("%s fp32: %d rows outside the fp32 model's slack of the fp64 value, %d abandoned; largest slack %.3g"
                  % (fam[0], bound.sum(), cnt.value, slack[fin].max()))
            assert int(bound.sum()) <= cnt.value, fam[0]            # (an abandoned row may report a bound within the slack)
            assert np.all(got[bound] <= fp64[bound] + slack[bound]), fam[0]
            assert np.all(got[bound] > hlow + 90.0 - 1e-6), fam[0]
            assert np.all(exact[fin & (fp64 + slack <= hlow + 90.0)]), fam[0]
            best, best64 = np.argmin(np.where(fin, got, np.inf)), np.argmin(np.where(fin, fp64, np.inf))
            assert exact[best] and fp64[best] <= fp64[best64] + slack[best] + slack[best64], fam[0]
    finally:
        L.trx_set_debug_bounded_lnl(0)
    print("%d points: %d of %d rows abandoned" % (n_time, total, 6 * n))
    assert total > 0                                     # the rule does bite


# ---------------------------------------------------------------------------------------
# 6. the evidence
def test_evidence_of_long_rows_does_not_depend_on_which_rows_stop():
    """tests/test_gpu_bounded.py::test_evidence_and_best_draw_do_not_depend_on_which_rows_stop at 4500 irregular stamps: lnZ
    of the bounded evaluation within 1e-13 relative of the full one's, the same best draw, three bounded runs bit for bit"""
    L = _lib.lib()
    rng, t_d, flux, f_d = _bounded_light_curve(IRREGULAR[1], True)
    n = 20000
    cnt = ctypes.c_ulonglong(0)
    try:
        L.trx_pruned_rows(ctypes.byref(cnt), 1)
        for fam in synth.FAMILIES[:6]:
            rows_d = _lib.dev(synth.family_rows(rng, fam, n))
            lp = _lib.dev(np.where(rng.random(n) < 0.1, -np.inf, -rng.exponential(3.0, n)))
            flags = _lib.FLAG_COMPANION_IS_HOST if fam[2] else 0
            out = {}
            for mode in (0, 1, 1, 1):
                L.trx_set_debug_bounded_lnl(mode)
                h, lnz = _lib.lnz_scenario(fam[1], flags, t_d, f_d, synth.SIGMA, rows_d, synth.EXPTIME, 20, lp, n,
                                           float(np.log(synth.SIGMA)))
                out.setdefault(mode, []).append((float(lnz.cpu()[0]), int(torch.argmin(h).cpu())))
            (z0, b0), = out[0]
            print("%s: lnZ %.17g, bounded - full %s" % (fam[0], z0, [z - z0 for z, _ in out[1]]))
            assert np.isfinite(z0)
            assert all(b == b0 for _, b in out[1]), fam[0]
            assert all(abs(z - z0) <= 1e-13 * abs(z0) for z, _ in out[1]), fam[0]
            assert len({z for z, _ in out[1]}) == 1, fam[0]
        L.trx_pruned_rows(ctypes.byref(cnt), 1)
        assert cnt.value > 0
    finally:
        L.trx_set_debug_bounded_lnl(0)


# ---------------------------------------------------------------------------------------
# 7. end to end
def _many(chain):
    """tests/test_gpu_star_chain.py::_many on two targets of 2300 points: a second window pass of 252 cells"""
    import triceratops_amd
    from test_gpu_star_chain import CC, TRI, _tables
    L = _lib.lib()
    triceratops_amd.set_sampling("device")
    try:
        L.trx_set_star_chain(chain)
        jobs = synth.toi_jobs(2, n_time=2300, N=50_000, seed=11, trilegal_fname=TRI, contrast_curve_file=CC)
        torch.manual_seed(11)
        _lib.reset_stats()
        triceratops_amd.calc_probs_many(jobs)
        assert _lib.STATS["native_calls"] == 12 * 2
        return _tables(jobs)
    finally:
        L.trx_set_star_chain(1)
        triceratops_amd.set_sampling("numpy")


def test_launch_chain_on_two_window_passes_equals_the_per_call_chain():
    a, b = _many(1), _many(0)
    for x, y in zip(a, b):
        assert np.array_equal(x, y, equal_nan=True), np.nanmax(np.abs(x - y))
    assert np.isfinite(a[0][0]) and -1e-12 <= a[0][-2] <= 1.0


def _long_dataset():
    """TOI-465.01's folded curve (100 points, tests/golden/toi465_calc_probs.npz) interpolated linearly onto 2600 uniform
    stamps over the same span, each with an error of its own -- sqrt(26) x the curve's sigma x a ramp from 0.6 to 1.8, so
    that the 2600 points carry about the information of the 100 -- and seeded normal noise of that size added"""
    from test_gpu_lnl_weighted import LC
    rng = np.random.default_rng(465)
    t = np.linspace(LC["time"][0], LC["time"][-1], 2600)
    err = LC["sigma"] * np.sqrt(26.0) * np.linspace(0.6, 1.8, 2600)
    flux = np.interp(t, LC["time"], LC["flux"]) + rng.normal(0.0, err)
    return [{"time": t, "flux": flux, "flux_err": err, "exptime": 0.00139, "nsamples": 20}]


def test_calc_probs_datasets_fused_is_the_grid_evaluation_on_two_window_passes(monkeypatch):
    """tests/test_gpu_lnl_weighted.py::test_calc_probs_datasets_fused_is_the_grid_evaluation with one dataset of 2600 points"""
    import triceratops_amd as ta
    import test_gpu_lnl_weighted as W
    mode = ta.get_sampling()
    ta.set_sampling("device")
    try:
        grid = W._pass(monkeypatch, "grid", _long_dataset())
        fused = W._pass(monkeypatch, "fused", _long_dataset())
    finally:
        ta.set_sampling(mode)
    assert fused["stats"]["rows"] == grid["stats"]["rows"] > 0 and fused["stats"]["cells"] == grid["stats"]["cells"]
    assert np.array_equal(fused["best"], grid["best"]) and np.array_equal(fused["u1"], grid["u1"])
    assert np.array_equal(fused["frc"], grid["frc"]) and fused["sigma_ref"] == grid["sigma_ref"]
    fin = np.isfinite(grid["lnZ"])
    assert np.array_equal(fin, np.isfinite(fused["lnZ"])) and fin.sum() >= 10
    assert grid["hmax"].size == fin.size == fused["hmax"].size
    d = np.abs(fused["lnZ"][fin] - grid["lnZ"][fin])
    bound = 1e-12 * grid["hmax"][fin] + 1e-12
    print("2600 points, fused against grid: max |d lnZ| %.3g, max of |d lnZ| / bound %.3g" % (d.max(), (d / bound).max()))
    assert (d <= bound).all(), (d, bound)
    assert len(fused["posterior"]) == len(grid["posterior"]) == fin.size
    for j, (p, q) in enumerate(zip(fused["posterior"], grid["posterior"])):
        assert (p is None) == (q is None)
        if p is None:
            continue
        assert p["row"].shape == (W.N_POST,) and np.array_equal(p["row"], q["row"])
        assert all(np.array_equal(p[k], q[k]) for k in q if k != "lnw")
        assert (np.abs(p["lnw"] - q["lnw"]) <= 1e-12 * grid["hmax"][j] + 1e-12).all()
    assert fused["grids"] == []
