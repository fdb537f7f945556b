"""chi2_ou_kernel<ONE> (trxn_chi2_grid_ou, include/trx_noise.h): the row reduction of a model grid
under white plus exponential (Ornstein-Uhlenbeck) noise,
    g_0 = 0,  g_n = alpha_n g_(n-1) + beta_n y_(n-1),   h = 0.5 sum_n omega_n (y_n - g_n)^2,   y = flux - grid[r].

The yardstick is _numerics.ou_halfchi2 in np.longdouble on the downloaded grid and the same alpha, beta, omega
(datasets.ou_system).  Bar, not chosen from results:
  |d h| <= 1e-12 (1 + 1 / (1 - max alpha)) 0.5 sum_n omega_n (|y_n| + max|y|)^2 + 1e-12: each g_n carries a rounding error
  of a few eps max|y| per step (|g| <= max|y| because alpha + beta <= 1), amplified by at most 1 / (1 - max alpha) through
  the recurrence, and enters z^2 linearly.
phi == 1 (tau = inf) is also held against chi2_grid_offset(sum_w, 1 / s_r^2) and phi == 0 (tau -> 0) against
chi2_grid_weighted with the weights 1 / (sigma^2 + s_r^2), to the same bar.
Shapes: one stamp, one pair, both sides of a lane's last pair (63, 64, 65), of one trip of 128 stamps (128, 129) -- the
two instantiations --, odd lengths (every second row off its 16-byte boundary), many trips (2048, 2049); odd row counts;
and (CAPPED) more rows than the capped grid of 1024 blocks has waves: rows in a wave's second slot and in its second pass.
Measured (one MI355X): the largest |d h| / bar of the whole file, printed by the last test, is 7.3e-5 (max alpha up to
0.9998); phi == 1 against the offset kernel at most 1.4e-8 of the bar at 5123 x 2048."""
import numpy as np
import pytest
import torch

from test_datasets_red_noise_api import PAIRS, SIGMA, row_bar
from triceratops_amd import _lib, _numerics, synth
from triceratops_amd import datasets as D

pytestmark = pytest.mark.gpu

N_TIMES = [1, 2, 63, 64, 65, 128, 129, 333, 2048, 2049]
NS = [1, 2, 3, 257]
CAPPED = [(65, 8195), (2048, 5123)]          # (n_time, n): 4 x 1024 waves
OU_BLOCKS_MAX = 1024
PARAMS = PAIRS + [(3.0, 1e-6), (3.0, float("inf"))]         # (s_r / sigma, tau / cadence): + phi == 0, phi == 1
LEVELS = (0.0, 3.0, 100.0)                   # residual offsets, in mean sigma
INF = float("inf")
LD = np.longdouble
_cases, _systems = {}, {}
_worst = {"h": 0.0}


def _system(n_time, ratio, tau):
    """the light curve's stamps and errors (one per n_time) and the noise system of one parameter pair, on the device"""
    key = (n_time, ratio, tau)
    if key not in _systems:
        rng = np.random.default_rng(synth.SEED + 104729 * n_time)
        t = np.cumsum(rng.uniform(0.3, 1.7, n_time))
        err = SIGMA * rng.uniform(0.6, 1.8, n_time)
        d = D.validate([{"time": t, "flux": np.ones(n_time), "flux_err": err, "red_sigma": ratio * SIGMA,
                         "red_timescale": tau}])[0]
        abw = D.ou_system(d)
        _systems[key] = dict(d=d, abw=abw, abw_d=tuple(_lib.dev(v) for v in abw))
    return _systems[key]


def _case(n_time, n):
    """a random grid near 1 and a light curve per residual level (made once per shape, never changed); the grid also as a
    view one double off the 16-byte boundary"""
    key = (n_time, n)
    if key not in _cases:
        rng = np.random.default_rng(synth.SEED + 7919 * n_time + n)
        g = 1.0 - np.abs(rng.normal(0.0, 2e-3, (n, n_time)))
        base = 1.0 + rng.normal(0.0, SIGMA, n_time)
        pad = torch.empty(n * n_time + 1, dtype=torch.float64, device=_lib.compute_device())
        pad[1:] = _lib.dev(g).reshape(-1)
        g_d = pad[1:].clone().view(n, n_time)
        g_off = pad[1:].view(n, n_time)
        assert g_d.data_ptr() % 16 == 0 and g_off.data_ptr() % 16 == 8
        flux = {k: base + k * 1.2 * SIGMA for k in LEVELS}           # (1.2 SIGMA: the mean of the errors)
        _cases[key] = dict(g=g_d.cpu().numpy(), g_d=g_d, g_off=g_off, flux=flux)
    return _cases[key]


def _check(n_time, n, params, levels):
    c = _case(n_time, n)
    for ratio, tau in params:
        s = _system(n_time, ratio, tau)
        alpha, beta, omega = s["abw"]
        for k in levels:
            flux = c["flux"][k]
            f_d = _lib.dev(flux)
            y = flux[None, :] - c["g"]
            ref = _numerics.ou_halfchi2(y, alpha, beta, omega, dtype=LD)
            bar = row_bar(y, alpha, omega)
            got = _lib.chi2_grid_ou(f_d, c["g_d"], *s["abw_d"])
            ratio_h = float((np.abs(got.cpu().numpy().astype(LD) - ref).astype(np.float64) / bar).max())
            _worst["h"] = max(_worst["h"], ratio_h)
            print("n_time %d n %d s_r %g sigma tau %g level %g sigma: max alpha %.6f, |d h| / bar %.3g (largest so far %.3g)"
                  % (n_time, n, ratio, tau, k, alpha.max(), ratio_h, _worst["h"]))
            assert ratio_h <= 1.0
            assert (got.cpu().numpy() >= 0.0).all()
            # rows one double off their 16-byte boundary: the same bits; and again: the same bits
            assert torch.equal(_lib.chi2_grid_ou(f_d, c["g_off"], *s["abw_d"]), got)
            assert torch.equal(_lib.chi2_grid_ou(f_d, c["g_d"], *s["abw_d"]), got)
            d = s["d"]
            if tau == INF:
                w = 1.0 / d.flux_err ** 2
                other = _lib.chi2_grid_offset(f_d, _lib.dev(w), c["g_d"], float(np.sum(w.astype(LD))), 1.0 / d.red_sigma ** 2)
                r2 = float((np.abs(got.cpu().numpy() - other.cpu().numpy()) / bar).max())
                print("    phi == 1 against chi2_grid_offset: |d h| / bar %.3g" % r2)
                assert r2 <= 1.0
            if tau == 1e-6:
                assert not alpha.any() and not beta.any()
                other = _lib.chi2_grid_weighted(f_d, _lib.dev(1.0 / (d.flux_err ** 2 + d.red_sigma ** 2)), c["g_d"])
                r2 = float((np.abs(got.cpu().numpy() - other.cpu().numpy()) / bar).max())
                print("    phi == 0 against chi2_grid_weighted: |d h| / bar %.3g" % r2)
                assert r2 <= 1.0


@pytest.mark.parametrize("n_time, n", [(t, n) for n in NS for t in N_TIMES])
def test_ou_reduction_matches_longdouble(n_time, n):
    _check(n_time, n, PARAMS, LEVELS)


@pytest.mark.parametrize("n_time, n", CAPPED)
def test_ou_reduction_past_the_capped_grid(n_time, n):
    assert 4 * OU_BLOCKS_MAX < n
    _check(n_time, n, PARAMS, (3.0,))


@pytest.mark.parametrize("n_time, n", [(65, 257), (2049, 257), (65, 8195), (2049, 5123)])
def test_a_rows_bits_are_its_own(n_time, n):
    """the same row at position 0, 1 and n - 1 (behind the capped grid where n says so), in a launch of its own, in a view
    one double off, and on a second run"""
    c = _case(n_time, n)
    for ratio, tau in (PAIRS[1], PAIRS[3], PARAMS[-1]):
        abw = _system(n_time, ratio, tau)["abw_d"]
        f_d = _lib.dev(c["flux"][3.0])
        g = c["g_d"].clone()
        g[1] = g[0]
        g[n - 1] = g[0]
        got = _lib.chi2_grid_ou(f_d, g, *abw)
        h = got.cpu().numpy()
        assert h[0] > 0 and h[0].tobytes() == h[1].tobytes() == h[n - 1].tobytes()
        alone = _lib.chi2_grid_ou(f_d, g[:1].clone(), *abw).cpu().numpy()
        assert alone.tobytes() == h[:1].tobytes()
        pair = _lib.chi2_grid_ou(f_d, g[:2].clone(), *abw).cpu().numpy()
        assert pair.tobytes() == h[:2].tobytes()
        pad = torch.empty(n * n_time + 1, dtype=torch.float64, device=g.device)
        pad[1:] = g.reshape(-1)
        off = pad[1:].view(n, n_time)
        assert off.data_ptr() % 16 == 8
        assert torch.equal(_lib.chi2_grid_ou(f_d, off, *abw), got)
        assert torch.equal(_lib.chi2_grid_ou(f_d, g, *abw), got)
        # the other rows are those of the unchanged grid
        plain = _lib.chi2_grid_ou(f_d, c["g_d"], *abw).cpu().numpy()
        assert np.array_equal(h[2:n - 1], plain[2:n - 1])


@pytest.mark.parametrize("n_time, n", [(64, 257), (333, 257), (2049, 257), CAPPED[0]], ids=["64", "333", "2049", "65-8195"])
def test_accumulates_onto_finite_inf_and_nan(n_time, n):
    c = _case(n_time, n)
    abw = _system(n_time, *PAIRS[1])["abw_d"]
    f_d = _lib.dev(c["flux"][3.0])
    h = _lib.chi2_grid_ou(f_d, c["g_d"], *abw).cpu().numpy()
    out0 = np.random.default_rng(n_time).uniform(0.0, 50.0, n)
    out0[::5] = np.inf
    out0[1::7] = np.nan
    fin = np.isfinite(out0)
    assert fin.sum() > 100 and np.isposinf(out0).sum() > 10 and np.isnan(out0).sum() > 10
    acc = _lib.chi2_grid_ou(f_d, c["g_d"], *abw, out=_lib.dev(out0).clone()).cpu().numpy()
    assert np.array_equal(acc[fin], out0[fin] + h[fin])
    assert np.array_equal(np.isposinf(acc), np.isposinf(out0)) and np.array_equal(np.isnan(acc), np.isnan(out0))
    # with a rule of its own: +inf from either side
    sec = np.linspace(0.0, 1.0, n)
    acc = _lib.chi2_grid_ou(f_d, c["g_d"], *abw, _lib.dev(sec), 0.5, out=_lib.dev(out0).clone()).cpu().numpy()
    assert np.array_equal(np.isposinf(acc), (np.isposinf(out0) | (sec >= 0.5)) & ~np.isnan(out0))


@pytest.mark.parametrize("n_time", [65, 2049])
def test_secondary_rule_is_the_weighted_kernels(n_time):
    c = _case(n_time, 257)
    s = _system(n_time, *PAIRS[1])
    abw = s["abw_d"]
    f_d = _lib.dev(c["flux"][3.0])
    rng = np.random.default_rng(n_time)
    sec = rng.uniform(0.0, 1.0, 257)
    sec[:7] = np.nan
    sec[7] = 0.5                                                   # equality excludes
    excluded = sec >= 0.5                                          # (false for NaN)
    assert excluded[7] and not excluded[:7].any() and 0 < excluded.sum() < 257
    sec_d = _lib.dev(sec)
    w_d = _lib.dev(1.0 / s["d"].flux_err ** 2)
    for g in (c["g_d"], c["g_off"]):
        got = _lib.chi2_grid_ou(f_d, g, *abw, sec_d, 0.5).cpu().numpy()
        want = _lib.chi2_grid_weighted(f_d, w_d, g, sec_d, 0.5).cpu().numpy()
        assert np.array_equal(np.isposinf(got), excluded) and np.array_equal(np.isposinf(got), np.isposinf(want))
        assert not np.isnan(got).any()
        free = _lib.chi2_grid_ou(f_d, g, *abw).cpu().numpy()
        assert np.array_equal(got[~excluded], free[~excluded])
        # sec_limit = +inf: the rule is off
        assert np.array_equal(_lib.chi2_grid_ou(f_d, g, *abw, sec_d, INF).cpu().numpy(), free)


@pytest.mark.parametrize("n_time", [1, 2, 65, 129, 333, 2049])
def test_a_nan_in_a_row_is_a_nan_row_and_no_other(n_time):
    n = 257
    c = _case(n_time, n)
    f_d = _lib.dev(c["flux"][3.0])
    spots = sorted({0, n_time - 1, n_time // 2, min(127, n_time - 1), min(128, n_time - 1), (n_time - 1) & ~1})
    rows = [3 + 11 * i for i in range(len(spots))]
    for ratio, tau in (PAIRS[1], PARAMS[-2], PARAMS[-1]):
        abw = _system(n_time, ratio, tau)["abw_d"]
        clean = _lib.chi2_grid_ou(f_d, c["g_d"], *abw).cpu().numpy()
        g = c["g_d"].clone()
        for r, t in zip(rows, spots):
            g[r, t] = float("nan")
        got = _lib.chi2_grid_ou(f_d, g, *abw).cpu().numpy()
        hit = np.zeros(n, dtype=bool)
        hit[rows] = True
        assert np.isnan(got[hit]).all() and np.array_equal(got[~hit], clean[~hit])
        # ... also under accumulation
        acc = _lib.chi2_grid_ou(f_d, g, *abw, out=torch.ones(n, dtype=torch.float64, device=g.device)).cpu().numpy()
        assert np.isnan(acc[hit]).all() and np.array_equal(acc[~hit], 1.0 + clean[~hit])


def test_arguments_and_empty_grid():
    c = _case(63, 3)
    abw = _system(63, *PAIRS[0])["abw_d"]
    f_d = _lib.dev(c["flux"][0.0])
    assert _lib.chi2_grid_ou(f_d, c["g_d"][:0], *abw).shape == (0,)
    with pytest.raises(AssertionError):
        _lib.chi2_grid_ou(f_d, c["g_d"], abw[0][:5], abw[1], abw[2])


def test_zz_report_the_largest_ratio():
    """(runs last in the file: the figure DESIGN.md section 14 quotes)"""
    print("chi2_ou_kernel against np.longdouble: largest |d h| / bar over the file %.3g" % _worst["h"])
    assert _worst["h"] <= 1.0
