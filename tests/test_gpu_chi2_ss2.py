"""ss2_kernel<ONE> (trxs_chi2_grid_ss2, include/trx_ss.h): the row reduction of a model grid under
white noise plus a process with a two-dimensional state (a Matern-3/2 term, two exponential terms),
    u_(-1) = 0,  z_n = y_n - u_(n-1)[0],  u_n = A_n u_(n-1) + g_n y_n,   h = 0.5 sum_n omega_n z_n^2,   y = flux - grid[r].

The yardstick is _numerics.ss2_halfchi2 in np.longdouble on the downloaded grid and the same A, g, omega
(datasets.ss2_system).  Bar, from the tables alone and written before the first run on a device:
  the prediction is linear in the earlier residuals, u_(n-1)[0] = sum_(m<n) c_(n,m) y_m with
  c_(n,m) = e_0^T A_(n-1) ... A_(m+1) g_m, so |u_(n-1)[0]| <= Gamma max|y| with Gamma = max_n sum_m |c_(n,m)|, the
  predictor's l1 gain (computed on the host in long double, `gain`).  Every rounding of the recurrence -- sequential or in
  the scan's spans, whose partial products are products of the same A -- is a perturbation of a few eps Gamma max|y| of some
  u, carried on by the same products and so amplified by at most 1 + Gamma on its way into a later prediction, where it
  enters z^2 linearly:
      |d h| <= 1e-12 (1 + Gamma) 0.5 sum_n omega_n (|y_n| + Gamma max|y|)^2 + 1e-12.
  This is the bar of tests/test_gpu_chi2_ou.py with the predictor's true l1 gain in place of 1 / (1 - max alpha): a
  Matern-3/2 predictor extrapolates a slope, its weights change sign, and no bound of the form alpha + beta <= 1 holds.
Cross-kernel: A = [[alpha, 0], [0, 0]], g = (beta, 0) from datasets.ou_system (shifted by one stamp: u_n is the prediction
for stamp n + 1) is chi2_grid_ou's recurrence: to the sum of the two kernels' bars.
Shapes: one stamp, one pair, both sides of a lane's last pair (63, 64, 65), of one trip of 128 stamps (128, 129) -- the
two instantiations --, odd lengths (every second row off its 16-byte boundary), many trips (2048, 2049); odd row counts;
and (CAPPED) more rows than the capped grid of 1024 blocks has waves: rows in a wave's second slot and in its second pass.
Measured (one MI355X): the largest |d h| / bar of the whole file, printed by the last test, is 2.55e-4 (Gamma up to 1.82); against
chi2_grid_ou on one-state tables at most 4.5e-6 of the summed bars, the same bits wherever alpha = 0."""
import numpy as np
import pytest
import torch

from test_datasets_red_kernel_api import keys
from test_datasets_red_noise_api import PAIRS, SIGMA, row_bar
from triceratops_amd import _lib, _numerics, synth
from triceratops_amd import datasets as D

pytestmark = pytest.mark.gpu

N_TIMES = [1, 2, 63, 64, 65, 128, 129, 333, 2048, 2049]
NS = [1, 2, 3, 257]
CAPPED = [(65, 8195), (2048, 5123)]          # (n_time, n): 4 x 1024 waves
SS2_BLOCKS_MAX = 1024
# (kernel, s / sigma, time scale / cadence): smooth and rough Matern terms, two exponential terms a factor 7 apart
PARAMS = [("matern32", 3.0, 5.0), ("matern32", 10.0, 50.0), ("matern32", 0.3, 0.5), ("ou2", 3.0, 2.0), ("ou2", 10.0, 50.0)]
LEVELS = (0.0, 3.0, 100.0)                   # residual offsets, in mean sigma
INF = float("inf")
LD = np.longdouble
_cases, _systems = {}, {}
_worst = {"h": 0.0, "gamma": 0.0}


def gain(A, g):
    """Gamma = max_n sum_(m<n) |e_0^T A_(n-1) ... A_(m+1) g_m| in long double: after stamp n, w[m] = A_n ... A_(m+1) g_m"""
    A, g = np.asarray(A, dtype=LD), np.asarray(g, dtype=LD)
    T = g.shape[0]
    w0, w1 = np.zeros(T, dtype=LD), np.zeros(T, dtype=LD)
    top = LD(0.0)
    for n in range(T - 1):                   # (the last stamp's tables predict nothing)
        a0, a1 = w0[:n], w1[:n]
        w0[:n], w1[:n] = A[n, 0, 0] * a0 + A[n, 0, 1] * a1, A[n, 1, 0] * a0 + A[n, 1, 1] * a1
        w0[n], w1[n] = g[n, 0], g[n, 1]
        top = max(top, np.sum(np.abs(w0[:n + 1])))
    return float(top)


def ss2_bar(y, gamma, omega):
    y = np.abs(np.asarray(y, dtype=np.float64))
    top = y.max(axis=-1, keepdims=True)
    return 1e-12 * (1.0 + gamma) * 0.5 * np.sum(omega * (y + gamma * top) ** 2, axis=-1) + 1e-12


def _tables(n_time):
    rng = np.random.default_rng(synth.SEED + 104729 * n_time)
    return np.cumsum(rng.uniform(0.3, 1.7, n_time)), SIGMA * rng.uniform(0.6, 1.8, n_time)


def _system(n_time, kernel, ratio, scale):
    """the light curve's stamps and errors (one per n_time) and the noise system of one parameter set, on the device"""
    key = (n_time, kernel, ratio, scale)
    if key not in _systems:
        t, err = _tables(n_time)
        d = D.validate([dict(time=t, flux=np.ones(n_time), flux_err=err, **keys(kernel, ratio, scale))])[0]
        A, g, omega = D.ss2_system(d)
        _systems[key] = dict(d=d, agw=(A, g, omega), agw_d=tuple(_lib.dev(np.ascontiguousarray(v)) for v in (A, g, omega)),
                             gamma=gain(A, g))
        _worst["gamma"] = max(_worst["gamma"], _systems[key]["gamma"])
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
    for kernel, ratio, scale in params:
        s = _system(n_time, kernel, ratio, scale)
        A, g, omega = s["agw"]
        for k in levels:
            flux = c["flux"][k]
            f_d = _lib.dev(flux)
            y = flux[None, :] - c["g"]
            ref = _numerics.ss2_halfchi2(y, A, g, omega, dtype=LD)
            bar = ss2_bar(y, s["gamma"], omega)
            got = _lib.chi2_grid_ss2(f_d, c["g_d"], *s["agw_d"])
            ratio_h = float((np.abs(got.cpu().numpy().astype(LD) - ref).astype(np.float64) / bar).max())
            _worst["h"] = max(_worst["h"], ratio_h)
            print("n_time %d n %d %s s %g sigma scale %g level %g sigma: Gamma %.4f, |d h| / bar %.3g (largest so far %.3g)"
                  % (n_time, n, kernel, ratio, scale, k, s["gamma"], ratio_h, _worst["h"]))
            assert ratio_h <= 1.0
            assert (got.cpu().numpy() >= 0.0).all()
            # rows one double off their 16-byte boundary: the same bits; and again: the same bits
            assert torch.equal(_lib.chi2_grid_ss2(f_d, c["g_off"], *s["agw_d"]), got)
            assert torch.equal(_lib.chi2_grid_ss2(f_d, c["g_d"], *s["agw_d"]), got)


@pytest.mark.parametrize("n_time, n", [(t, n) for n in NS for t in N_TIMES])
def test_ss2_reduction_matches_longdouble(n_time, n):
    _check(n_time, n, PARAMS, LEVELS)


@pytest.mark.parametrize("n_time, n", CAPPED)
def test_ss2_reduction_past_the_capped_grid(n_time, n):
    assert 4 * SS2_BLOCKS_MAX < n
    _check(n_time, n, PARAMS[:2] + PARAMS[-1:], (3.0,))


@pytest.mark.parametrize("n_time, n", [(65, 257), (2049, 257), (65, 8195), (2049, 5123)])
def test_a_rows_bits_are_its_own(n_time, n):
    """the same row at position 0, 1 and n - 1 (behind the capped grid where n says so), in a launch of its own, in a view
    one double off, and on a second run"""
    c = _case(n_time, n)
    for params in (PARAMS[0], PARAMS[-1]):
        agw = _system(n_time, *params)["agw_d"]
        f_d = _lib.dev(c["flux"][3.0])
        g = c["g_d"].clone()
        g[1] = g[0]
        g[n - 1] = g[0]
        got = _lib.chi2_grid_ss2(f_d, g, *agw)
        h = got.cpu().numpy()
        assert h[0] > 0 and h[0].tobytes() == h[1].tobytes() == h[n - 1].tobytes()
        alone = _lib.chi2_grid_ss2(f_d, g[:1].clone(), *agw).cpu().numpy()
        assert alone.tobytes() == h[:1].tobytes()
        pair = _lib.chi2_grid_ss2(f_d, g[:2].clone(), *agw).cpu().numpy()
        assert pair.tobytes() == h[:2].tobytes()
        pad = torch.empty(n * n_time + 1, dtype=torch.float64, device=g.device)
        pad[1:] = g.reshape(-1)
        off = pad[1:].view(n, n_time)
        assert off.data_ptr() % 16 == 8
        assert torch.equal(_lib.chi2_grid_ss2(f_d, off, *agw), got)
        assert torch.equal(_lib.chi2_grid_ss2(f_d, g, *agw), got)
        # the other rows are those of the unchanged grid
        plain = _lib.chi2_grid_ss2(f_d, c["g_d"], *agw).cpu().numpy()
        assert np.array_equal(h[2:n - 1], plain[2:n - 1])


@pytest.mark.parametrize("ratio, tau", PAIRS)
@pytest.mark.parametrize("n_time, n", [(1, 3), (2, 3), (65, 257), (128, 257), (129, 257), (2049, 257)])
def test_one_state_tables_are_the_ou_kernel(n_time, n, ratio, tau):
    c = _case(n_time, n)
    t, err = _tables(n_time)
    d = D.validate([{"time": t, "flux": np.ones(n_time), "flux_err": err, "red_sigma": ratio * SIGMA, "red_timescale": tau}])[0]
    alpha, beta, omega = D.ou_system(d)
    A, g = np.zeros((n_time, 2, 2)), np.zeros((n_time, 2))
    A[:-1, 0, 0], g[:-1, 0] = alpha[1:], beta[1:]
    gamma = gain(A, g)
    assert gamma <= 1.0 + 1e-12                                   # (alpha + beta <= 1: a convex predictor)
    for k in LEVELS:
        flux = c["flux"][k]
        f_d = _lib.dev(flux)
        y = flux[None, :] - c["g"]
        got = _lib.chi2_grid_ss2(f_d, c["g_d"], _lib.dev(A), _lib.dev(g), _lib.dev(omega)).cpu().numpy()
        want = _lib.chi2_grid_ou(f_d, c["g_d"], _lib.dev(alpha), _lib.dev(beta), _lib.dev(omega)).cpu().numpy()
        bar = ss2_bar(y, gamma, omega) + row_bar(y, alpha, omega)
        print("n_time %d s_r %g sigma tau %g level %g: against chi2_grid_ou |d h| / bar %.3g, the same bits in %d of %d rows"
              % (n_time, ratio, tau, k, (np.abs(got - want) / bar).max(), (got == want).sum(), n))
        assert (np.abs(got - want) <= bar).all()


@pytest.mark.parametrize("n_time, n", [(64, 257), (333, 257), (2049, 257), CAPPED[0]], ids=["64", "333", "2049", "65-8195"])
def test_accumulates_onto_finite_inf_and_nan(n_time, n):
    c = _case(n_time, n)
    agw = _system(n_time, *PARAMS[0])["agw_d"]
    f_d = _lib.dev(c["flux"][3.0])
    h = _lib.chi2_grid_ss2(f_d, c["g_d"], *agw).cpu().numpy()
    out0 = np.random.default_rng(n_time).uniform(0.0, 50.0, n)
    out0[::5] = np.inf
    out0[1::7] = np.nan
    fin = np.isfinite(out0)
    assert fin.sum() > 100 and np.isposinf(out0).sum() > 10 and np.isnan(out0).sum() > 10
    acc = _lib.chi2_grid_ss2(f_d, c["g_d"], *agw, out=_lib.dev(out0).clone()).cpu().numpy()
    assert np.array_equal(acc[fin], out0[fin] + h[fin])
    assert np.array_equal(np.isposinf(acc), np.isposinf(out0)) and np.array_equal(np.isnan(acc), np.isnan(out0))
    # an all-+inf target stays +inf
    acc = _lib.chi2_grid_ss2(f_d, c["g_d"], *agw, out=torch.full((n,), INF, dtype=torch.float64, device=f_d.device))
    assert np.isposinf(acc.cpu().numpy()).all()
    # with a rule of its own: +inf from either side
    sec = np.linspace(0.0, 1.0, n)
    acc = _lib.chi2_grid_ss2(f_d, c["g_d"], *agw, _lib.dev(sec), 0.5, out=_lib.dev(out0).clone()).cpu().numpy()
    assert np.array_equal(np.isposinf(acc), (np.isposinf(out0) | (sec >= 0.5)) & ~np.isnan(out0))


@pytest.mark.parametrize("n_time", [65, 2049])
def test_secondary_rule_is_the_weighted_kernels(n_time):
    c = _case(n_time, 257)
    s = _system(n_time, *PARAMS[-1])
    agw = s["agw_d"]
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
        got = _lib.chi2_grid_ss2(f_d, g, *agw, sec_d, 0.5).cpu().numpy()
        want = _lib.chi2_grid_weighted(f_d, w_d, g, sec_d, 0.5).cpu().numpy()
        assert np.array_equal(np.isposinf(got), excluded) and np.array_equal(np.isposinf(got), np.isposinf(want))
        assert not np.isnan(got).any()
        free = _lib.chi2_grid_ss2(f_d, g, *agw).cpu().numpy()
        assert np.array_equal(got[~excluded], free[~excluded])
        # sec_limit = +inf: the rule is off
        assert np.array_equal(_lib.chi2_grid_ss2(f_d, g, *agw, sec_d, INF).cpu().numpy(), free)


@pytest.mark.parametrize("n_time", [1, 2, 65, 129, 333, 2049])
def test_a_nan_in_a_row_is_a_nan_row_and_no_other(n_time):
    n = 257
    c = _case(n_time, n)
    f_d = _lib.dev(c["flux"][3.0])
    spots = sorted({0, n_time - 1, n_time // 2, min(127, n_time - 1), min(128, n_time - 1), (n_time - 1) & ~1})
    rows = [3 + 11 * i for i in range(len(spots))]
    for params in (PARAMS[0], PARAMS[2], PARAMS[-1]):
        agw = _system(n_time, *params)["agw_d"]
        clean = _lib.chi2_grid_ss2(f_d, c["g_d"], *agw).cpu().numpy()
        g = c["g_d"].clone()
        for r, t in zip(rows, spots):
            g[r, t] = float("nan")
        got = _lib.chi2_grid_ss2(f_d, g, *agw).cpu().numpy()
        hit = np.zeros(n, dtype=bool)
        hit[rows] = True
        assert np.isnan(got[hit]).all() and np.array_equal(got[~hit], clean[~hit])
        # ... also under accumulation
        acc = _lib.chi2_grid_ss2(f_d, g, *agw, out=torch.ones(n, dtype=torch.float64, device=g.device)).cpu().numpy()
        assert np.isnan(acc[hit]).all() and np.array_equal(acc[~hit], 1.0 + clean[~hit])


def test_arguments_and_empty_grid():
    c = _case(63, 3)
    agw = _system(63, *PARAMS[0])["agw_d"]
    f_d = _lib.dev(c["flux"][0.0])
    assert _lib.chi2_grid_ss2(f_d, c["g_d"][:0], *agw).shape == (0,)
    with pytest.raises(AssertionError):
        _lib.chi2_grid_ss2(f_d, c["g_d"], agw[0][:5], agw[1], agw[2])
    with pytest.raises(AssertionError):
        _lib.chi2_grid_ss2(f_d, c["g_d"], agw[0], agw[2], agw[2])          # g of [n_time]: half the table
    with pytest.raises(AssertionError):
        _lib.chi2_grid_ss2(f_d[:5], c["g_d"], *agw)


def test_zz_report_the_largest_ratio():
    """(runs last in the file: the figures DESIGN.md section 14 quotes)"""
    print("ss2_kernel against np.longdouble: largest |d h| / bar over the file %.3g, largest Gamma %.4g"
          % (_worst["h"], _worst["gamma"]))
    assert _worst["h"] <= 1.0
