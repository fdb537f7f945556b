"""gls_ou_kernel<ONE, K> (trxg_chi2_grid_ou_baseline, include/trx_gls.h): the row reduction of a model
grid under white plus exponential (Ornstein-Uhlenbeck) noise with K baseline columns marginalised under that noise,
    z = the innovations of y = flux - grid[r],  S2 = sum omega z^2,  b~_k = sum c_k z,  h = 0.5 max(S2 - b~^T M b~, 0),
    coef = M b~,   c_k = omega z[B_k] / sqrt(D_k) and M = A~^-1 from datasets.ou_baseline_system.

The yardstick is _numerics.ou_baseline_halfchi2 in np.longdouble on the downloaded grid and the tables the device holds.
Bars, not chosen from results (gls_bar, coef_bar of tests/test_datasets_red_baseline_api.py):
  |d h| <= 1e-12 (1 + 1 / (1 - max alpha)) 0.5 sum omega_n (|y_n| + max|y|)^2 (1 + 4 sqrt(K / lambda_min)) + 1e-12:
        row_bar of tests/test_gpu_chi2_ou.py -- each innovation carries a few eps max|y| per step, amplified by at most
        1 / (1 - max alpha) -- times the projection factor of tests/test_gpu_chi2_baseline.py: |d b~_k| is bounded by the
        same innovation errors through Cauchy-Schwarz in the unit columns, and a perturbation d b~ moves the quadratic form
        by at most 2 sqrt(S2) |d b~| / sqrt(lambda_min);
  coef_out: 1e-12 (1 + 1 / (1 - max alpha)) sqrt(K sum omega (|y| + max|y|)^2) / lambda_min + 1e-15 per entry;
  minv = 0: the bits of _lib.chi2_grid_ou (S2 is formed term for term the same way; S2 - 0 = S2);
  cross-kernel: tau = inf is white noise plus a constant of prior s_r, so the reduction is chi2_grid_baseline's with the
        ones column under prior s_r prepended; tau = 1e-6 cadences is white noise of variance sigma^2 + s_r^2, so it is
        chi2_grid_baseline's with the weights 1 / (sigma^2 + s_r^2): each to the sum of the two kernels' bars (the other's:
        1e-12 x 0.5 S2 x (1 + 4 sqrt(K' / lambda_min')) + 1e-12 on its own weights and system).
Shapes: as many stamps as columns and one more, both sides of a lane's last pair (63, 64, 65), of one trip of 128 stamps
(128, 129) -- the two instantiations --, odd lengths (every second row off its 16-byte boundary), many trips (333, 2049);
odd row counts; and (CAPPED) more rows than the capped grid of 1024 blocks has waves: rows in a wave's second slot and in
its second pass.  Columns u^p, p = 0 .. K - 1; PARAMS as the OU file; residual levels 0, 3 and 100 mean sigma; flat priors
and A~ + I.  Per shape and K every parameter pair meets both priors, the level rotating so that over K = 1 .. 4 every
(pair, prior) meets every level.
Measured (one MI355X, test_zz_report_the_largest_ratios): the largest |d h| / bar of the whole file 2.1e-5, the largest
|d coef| / bar 7.7e-5 (max alpha up to 0.9998, lambda_min down to 0.027); tau = inf against chi2_grid_baseline at most 5.6e-6
and tau = 1e-6 cadences at most 1.7e-5 of the summed bars."""
import numpy as np
import pytest
import torch

from test_datasets_red_baseline_api import coef_bar, gls_bar
from test_datasets_red_noise_api import PAIRS, SIGMA
from triceratops_amd import _lib, _numerics, synth
from triceratops_amd import datasets as D

pytestmark = pytest.mark.gpu

KS = [1, 2, 3, 4]
N_TIMES = ["K", "K+1", 63, 64, 65, 128, 129, 333, 2049]
NS = [1, 2, 3, 257]
CAPPED = [(4, 65, 8195), (2, 2048, 5123)]    # (K, n_time, n): 4 x 1024 waves
GLS_BLOCKS_MAX = 1024
PARAMS = PAIRS + [(3.0, 1e-6), (3.0, float("inf"))]         # (s_r / sigma, tau / cadence): + phi == 0, phi == 1
LEVELS = (0.0, 3.0, 100.0)                   # residual offsets, in mean sigma
PRIORS = ("flat", "plus_identity")
INF = float("inf")
LD = np.longdouble
_cases, _systems = {}, {}
_worst = {"h": 0.0, "coef": 0.0, "inf": 0.0, "zero": 0.0}


def _n_time(spec, K):
    return K if spec == "K" else K + 1 if spec == "K+1" else spec


def _unit(t):
    return (t - 0.5 * (t[0] + t[-1])) / (0.5 * (t[-1] - t[0])) if t.size > 1 else np.zeros(1)


def _dataset(n_time, ratio, tau):
    """the light curve's stamps and errors (one per n_time: those of tests/test_gpu_chi2_ou.py) with one parameter pair"""
    rng = np.random.default_rng(synth.SEED + 104729 * n_time)
    t = np.cumsum(rng.uniform(0.3, 1.7, n_time))
    err = SIGMA * rng.uniform(0.6, 1.8, n_time)
    return D.validate([{"time": t, "flux": np.ones(n_time), "flux_err": err, "red_sigma": ratio * SIGMA,
                        "red_timescale": tau}])[0]


def _system(n_time, ratio, tau, K, prior, first_power=0):
    """the system of the columns u^p, p = first_power .. first_power + K - 1, under one parameter pair and one prior, and
    its tables on the device"""
    key = (n_time, ratio, tau, K, prior, first_power)
    if key not in _systems:
        d = _dataset(n_time, ratio, tau)
        u = _unit(d.time)
        B = np.stack([u ** p for p in range(first_power, first_power + K)])
        s = D.ou_baseline_system(d, B, INF)
        if prior == "plus_identity":
            s = D.ou_baseline_system(d, B, 1.0 / np.sqrt(s.D))                # 1 / (s_k^2 D_k) = 1
        elif prior != "flat":
            s = D.ou_baseline_system(d, B, prior)                             # (given sigmas)
        assert s.lambda_min >= D.MIN_BASELINE_EIGENVALUE, (key, s.lambda_min)
        _systems[key] = dict(d=d, B=B, s=s, dev=tuple(_lib.dev(v) for v in (s.alpha, s.beta, s.omega, s.c)))
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


def _call(f_d, g_d, S, **kw):
    return _lib.chi2_grid_ou_baseline(f_d, g_d, *S["dev"], S["s"].minv, **kw)


def _check(K, n_time, n, combos, rows=None):
    """combos: (ratio, tau, prior, level); rows: the rows held against the long-double statement (None: all) -- the other
    rows are then held, bit for bit, against launches of at most 4096 rows, which stay below the cap"""
    c = _case(n_time, n)
    rows = np.arange(n) if rows is None else np.asarray(rows)
    for ratio, tau, prior, level in combos:
        S = _system(n_time, ratio, tau, K, prior)
        s = S["s"]
        flux = c["flux"][level]
        f_d = _lib.dev(flux)
        y = flux[None, :] - c["g"][rows]
        ref, cref = _numerics.ou_baseline_halfchi2(y, s, dtype=LD, return_coef=True)
        coef = torch.full((n, K), float("nan"), dtype=torch.float64, device=c["g_d"].device)
        got = _call(f_d, c["g_d"], S, coef_out=coef)
        h = got.cpu().numpy()
        r_h = float((np.abs(h[rows].astype(LD) - ref).astype(np.float64) / gls_bar(y, s)).max())
        r_c = float((np.abs(coef.cpu().numpy()[rows].astype(LD) - cref).astype(np.float64) / coef_bar(y, s)[:, None]).max())
        if rows.size < n:
            for r0 in range(0, n, 4096):
                part_c = torch.empty((min(4096, n - r0), K), dtype=torch.float64, device=coef.device)
                part = _call(f_d, c["g_d"][r0:r0 + 4096], S, coef_out=part_c)
                assert torch.equal(part, got[r0:r0 + 4096]) and torch.equal(part_c, coef[r0:r0 + 4096])
        _worst["h"], _worst["coef"] = max(_worst["h"], r_h), max(_worst["coef"], r_c)
        print("K %d n_time %d n %d s_r %g sigma tau %g %s level %g sigma: max alpha %.6f lambda_min %.3g, |d h| / bar %.3g, "
              "|d coef| / bar %.3g (largest so far %.3g, %.3g)"
              % (K, n_time, n, ratio, tau, prior, level, s.alpha.max(), s.lambda_min, r_h, r_c, _worst["h"], _worst["coef"]))
        assert r_h <= 1.0 and r_c <= 1.0
        assert (h >= 0.0).all()
        # without coef_out, one double off the 16-byte boundary, and again: the same bits
        assert torch.equal(_call(f_d, c["g_d"], S), got)
        coef2 = torch.empty_like(coef)
        assert torch.equal(_call(f_d, c["g_off"], S, coef_out=coef2), got) and torch.equal(coef2, coef)
        assert torch.equal(_call(f_d, c["g_d"], S, coef_out=coef2), got) and torch.equal(coef2, coef)


def _combos(K, salt):
    return [(ratio, tau, prior, LEVELS[(i + j + K + salt) % 3])
            for i, (ratio, tau) in enumerate(PARAMS) for j, prior in enumerate(PRIORS)]


@pytest.mark.parametrize("spec, n", [(t, n) for n in NS for t in N_TIMES])
def test_reduction_matches_longdouble(spec, n):
    for K in KS:
        _check(K, _n_time(spec, K), n, _combos(K, N_TIMES.index(spec) + n))


@pytest.mark.parametrize("K, n_time, n", CAPPED)
def test_reduction_past_the_capped_grid(K, n_time, n):
    assert 4 * GLS_BLOCKS_MAX < n
    # the long-double statement on rows of a wave's first slot, around the start of its second slot, and at the end (the
    # second pass where n > 8192); every row against uncapped launches
    rows = np.unique(np.concatenate([np.arange(64), np.arange(4096 - 32, 4096 + 96), np.arange(n - 64, n)]))
    _check(K, n_time, n, [(ratio, tau, PRIORS[i % 2], 3.0) for i, (ratio, tau) in enumerate(PARAMS)], rows=rows)


@pytest.mark.parametrize("n_time, n", [(1, 3), (2, 257), (65, 257), (128, 3), (129, 257), (333, 2), (2049, 257), (65, 8195)])
def test_minv_zero_gives_the_ou_kernels_bits(n_time, n):
    c = _case(n_time, n)
    for K in KS:
        if K > n_time:
            continue
        for ratio, tau in (PAIRS[1], PAIRS[2], PARAMS[-1]):
            S = _system(n_time, ratio, tau, K, "flat")
            for level in (0.0, 100.0):
                f_d = _lib.dev(c["flux"][level])
                want = _lib.chi2_grid_ou(f_d, c["g_d"], *S["dev"][:3])
                coef = torch.full((n, K), float("nan"), dtype=torch.float64, device=c["g_d"].device)
                got = _lib.chi2_grid_ou_baseline(f_d, c["g_d"], *S["dev"], np.zeros(K * (K + 1) // 2), coef_out=coef)
                assert torch.equal(got, want) and (got > 0).all()
                assert not coef.any()                                      # M = 0: the coefficients are 0
                off = _lib.chi2_grid_ou_baseline(f_d, c["g_off"], *S["dev"], np.zeros(K * (K + 1) // 2))
                assert torch.equal(off, want)


@pytest.mark.parametrize("K, n_time, n", [(1, 65, 257), (3, 65, 257), (4, 2049, 257), (2, 129, 257), (4, 65, 8195),
                                          (2, 2049, 5123)])
def test_a_rows_bits_are_its_own(K, n_time, n):
    """row r of the grid against the same row alone, at position 0, 1 and n - 1 (behind the capped grid where n says so),
    in a view one double off, and on a second run"""
    c = _case(n_time, n)
    for ratio, tau in (PAIRS[1], PAIRS[3], PARAMS[-1]):
        S = _system(n_time, ratio, tau, K, "flat")
        f_d = _lib.dev(c["flux"][3.0])
        plain = _call(f_d, c["g_d"], S).cpu().numpy()
        r = n // 2 + 1
        g = c["g_d"].clone()
        g[0] = g[r]
        g[1] = g[r]
        g[n - 1] = g[r]
        coef = torch.empty((n, K), dtype=torch.float64, device=g.device)
        got = _call(f_d, g, S, coef_out=coef)
        h, cf = got.cpu().numpy(), coef.cpu().numpy()
        assert h[r].tobytes() == plain[r].tobytes() == h[0].tobytes() == h[1].tobytes() == h[n - 1].tobytes()
        assert cf[r].tobytes() == cf[0].tobytes() == cf[1].tobytes() == cf[n - 1].tobytes()
        c1 = torch.empty((1, K), dtype=torch.float64, device=g.device)
        alone = _call(f_d, c["g_d"][r:r + 1].clone(), S, coef_out=c1).cpu().numpy()
        assert alone.tobytes() == plain[r:r + 1].tobytes() and c1.cpu().numpy().tobytes() == cf[r:r + 1].tobytes()
        # ... also where the row alone sits one double off (r * n_time odd or not: both views)
        pad = torch.empty(n_time + 1, dtype=torch.float64, device=g.device)
        pad[1:] = c["g_d"][r]
        assert _call(f_d, pad[1:].view(1, n_time), S).cpu().numpy().tobytes() == alone.tobytes()
        assert torch.equal(_call(f_d, g, S), got)
        # the other rows are those of the unchanged grid
        assert np.array_equal(h[2:n - 1], plain[2:n - 1])


@pytest.mark.parametrize("K", [1, 2, 3])
@pytest.mark.parametrize("n_time, n", [(5, 3), (65, 257), (129, 257), (333, 257), (2049, 3)])
def test_infinite_timescale_is_the_baseline_kernel_with_a_constant(K, n_time, n):
    """tau = inf: K = diag(sigma^2) + s_r^2 1 1^T, a constant of prior s_r under white noise; columns u^1 .. u^K"""
    c = _case(n_time, n)
    sbar = 1.2 * SIGMA
    for sig in (INF, 30.0 * sbar):
        S = _system(n_time, 3.0, INF, K, sig, first_power=1)
        d, s = S["d"], S["s"]
        w = 1.0 / d.flux_err ** 2
        other = D.linear_system(w, np.concatenate([np.ones((1, n_time)), S["B"]]), np.array([d.red_sigma] + [sig] * K))
        assert other.lambda_min >= D.MIN_BASELINE_EIGENVALUE
        for level in LEVELS:
            flux = c["flux"][level]
            f_d = _lib.dev(flux)
            y = flux[None, :] - c["g"]
            got = _call(f_d, c["g_d"], S).cpu().numpy()
            want = _lib.chi2_grid_baseline(f_d, _lib.dev(w), c["g_d"], _lib.dev(other.g), other.minv).cpu().numpy()
            bar = gls_bar(y, s) + 1e-12 * 0.5 * np.sum(w * y * y, axis=1) * (1.0 + 4.0 * np.sqrt((K + 1) / other.lambda_min)) \
                + 1e-12
            r = float((np.abs(got - want) / bar).max())
            _worst["inf"] = max(_worst["inf"], r)
            print("K %d n_time %d prior %g level %g: phi == 1 against chi2_grid_baseline: |d h| / bar %.3g" % (K, n_time, sig, level, r))
            assert r <= 1.0


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("n_time, n", [(5, 3), (65, 257), (129, 257), (333, 257), (2049, 3)])
def test_short_timescale_is_the_baseline_kernel_on_wider_errors(K, n_time, n):
    """tau = 1e-6 cadences: alpha = beta = 0, omega = 1 / (sigma^2 + s_r^2); columns u^0 .. u^(K - 1)"""
    c = _case(n_time, n)
    sbar = 1.2 * SIGMA
    for sig in (INF, 30.0 * sbar):
        S = _system(n_time, 3.0, 1e-6, K, sig)
        d, s = S["d"], S["s"]
        assert not s.alpha.any() and not s.beta.any()
        w = 1.0 / (d.flux_err ** 2 + d.red_sigma ** 2)
        other = D.linear_system(w, S["B"], np.full(K, sig))
        for level in LEVELS:
            flux = c["flux"][level]
            f_d = _lib.dev(flux)
            y = flux[None, :] - c["g"]
            got = _call(f_d, c["g_d"], S).cpu().numpy()
            want = _lib.chi2_grid_baseline(f_d, _lib.dev(w), c["g_d"], _lib.dev(other.g), other.minv).cpu().numpy()
            bar = gls_bar(y, s) + 1e-12 * 0.5 * np.sum(w * y * y, axis=1) * (1.0 + 4.0 * np.sqrt(K / other.lambda_min)) + 1e-12
            r = float((np.abs(got - want) / bar).max())
            _worst["zero"] = max(_worst["zero"], r)
            print("K %d n_time %d prior %g level %g: phi == 0 against chi2_grid_baseline: |d h| / bar %.3g" % (K, n_time, sig, level, r))
            assert r <= 1.0


@pytest.mark.parametrize("K, n_time, n", [(1, 64, 257), (3, 333, 257), (4, 2049, 257), (4, 65, 8195)],
                         ids=["64", "333", "2049", "65-8195"])
def test_accumulates_onto_finite_inf_and_nan(K, n_time, n):
    c = _case(n_time, n)
    S = _system(n_time, *PAIRS[1], K, "flat")
    f_d = _lib.dev(c["flux"][3.0])
    h = _call(f_d, c["g_d"], S).cpu().numpy()
    out0 = np.random.default_rng(n_time).uniform(0.0, 50.0, n)
    out0[::5] = np.inf
    out0[1::7] = np.nan
    fin = np.isfinite(out0)
    assert fin.sum() > 100 and np.isposinf(out0).sum() > 10 and np.isnan(out0).sum() > 10
    acc = _call(f_d, c["g_d"], S, out=_lib.dev(out0).clone()).cpu().numpy()
    assert np.array_equal(acc[fin], out0[fin] + h[fin])
    assert np.array_equal(np.isposinf(acc), np.isposinf(out0)) and np.array_equal(np.isnan(acc), np.isnan(out0))
    # with a rule of its own: +inf from either side
    sec = np.linspace(0.0, 1.0, n)
    acc = _call(f_d, c["g_d"], S, secdepth=_lib.dev(sec), sec_limit=0.5, out=_lib.dev(out0).clone()).cpu().numpy()
    assert np.array_equal(np.isposinf(acc), (np.isposinf(out0) | (sec >= 0.5)) & ~np.isnan(out0))


@pytest.mark.parametrize("K, n_time", [(2, 65), (4, 2049)])
def test_secondary_rule_is_the_weighted_kernels(K, n_time):
    c = _case(n_time, 257)
    S = _system(n_time, *PAIRS[1], K, "plus_identity")
    f_d = _lib.dev(c["flux"][3.0])
    rng = np.random.default_rng(n_time)
    sec = rng.uniform(0.0, 1.0, 257)
    sec[:7] = np.nan
    sec[7] = 0.5                                                   # equality excludes
    excluded = sec >= 0.5                                          # (false for NaN)
    assert excluded[7] and not excluded[:7].any() and 0 < excluded.sum() < 257
    sec_d = _lib.dev(sec)
    w_d = _lib.dev(1.0 / S["d"].flux_err ** 2)
    for g in (c["g_d"], c["g_off"]):
        coef = torch.empty((257, K), dtype=torch.float64, device=g.device)
        got = _call(f_d, g, S, secdepth=sec_d, sec_limit=0.5, coef_out=coef).cpu().numpy()
        want = _lib.chi2_grid_weighted(f_d, w_d, g, sec_d, 0.5).cpu().numpy()
        assert np.array_equal(np.isposinf(got), excluded) and np.array_equal(np.isposinf(got), np.isposinf(want))
        assert not np.isnan(got).any()
        free_coef = torch.empty_like(coef)
        free = _call(f_d, g, S, coef_out=free_coef).cpu().numpy()
        assert np.array_equal(got[~excluded], free[~excluded])
        assert torch.equal(coef, free_coef)                         # an excluded row's coefficients are still its own
        # sec_limit = +inf: the rule is off
        assert np.array_equal(_call(f_d, g, S, secdepth=sec_d, sec_limit=INF).cpu().numpy(), free)


@pytest.mark.parametrize("K, n_time", [(1, 1), (2, 2), (3, 65), (2, 129), (4, 333), (4, 2049)])
def test_a_nan_in_a_row_is_a_nan_row_and_no_other(K, n_time):
    n = 257
    c = _case(n_time, n)
    f_d = _lib.dev(c["flux"][3.0])
    spots = sorted({0, n_time - 1, n_time // 2, min(127, n_time - 1), min(128, n_time - 1), (n_time - 1) & ~1})
    rows = [3 + 11 * i for i in range(len(spots))]
    for ratio, tau in (PAIRS[1], PARAMS[-2], PARAMS[-1]):
        S = _system(n_time, ratio, tau, K, "plus_identity")
        clean = _call(f_d, c["g_d"], S).cpu().numpy()
        g = c["g_d"].clone()
        for r, t in zip(rows, spots):
            g[r, t] = float("nan")
        got = _call(f_d, g, S).cpu().numpy()
        hit = np.zeros(n, dtype=bool)
        hit[rows] = True
        assert np.isnan(got[hit]).all() and np.array_equal(got[~hit], clean[~hit])
        # ... also under accumulation
        acc = _call(f_d, g, S, out=torch.ones(n, dtype=torch.float64, device=g.device)).cpu().numpy()
        assert np.isnan(acc[hit]).all() and np.array_equal(acc[~hit], 1.0 + clean[~hit])


def test_arguments_and_empty_grid():
    c = _case(63, 3)
    S = _system(63, *PAIRS[0], 2, "flat")
    f_d = _lib.dev(c["flux"][0.0])
    assert _call(f_d, c["g_d"][:0], S).shape == (0,)
    a, b, w, cols = S["dev"]
    with pytest.raises(AssertionError):
        _lib.chi2_grid_ou_baseline(f_d, c["g_d"], a[:5], b, w, cols, S["s"].minv)
    with pytest.raises(AssertionError):
        _lib.chi2_grid_ou_baseline(f_d, c["g_d"], a, b, w, cols[:, :5], S["s"].minv)
    with pytest.raises(AssertionError):
        _lib.chi2_grid_ou_baseline(f_d, c["g_d"], a, b, w, cols, S["s"].minv[:2])
    with pytest.raises(AssertionError):
        _lib.chi2_grid_ou_baseline(f_d, c["g_d"], a, b, w, torch.cat([cols, cols, cols]), np.zeros(21))
    with pytest.raises(AssertionError):
        _lib.chi2_grid_ou_baseline(f_d, c["g_d"], a, b, w, cols, S["s"].minv,
                                   coef_out=torch.empty((3, 3), dtype=torch.float64, device=f_d.device))
    # n == 0 through the ABI itself: nothing is launched
    rc = _lib.lib().trxg_chi2_grid_ou_baseline(f_d.data_ptr(), c["g_d"].data_ptr(), 63, 0, None, INF, 0, f_d.data_ptr(),
                                               a.data_ptr(), b.data_ptr(), w.data_ptr(), cols.data_ptr(), 2,
                                               S["s"].minv.ctypes.data, None, None)
    assert rc == 0


def test_zz_report_the_largest_ratios():
    """(runs last in the file: the figures DESIGN.md section 14 and the README quote)"""
    print("gls_ou_kernel against np.longdouble: largest |d h| / bar over the file %.3g, largest |d coef| / bar %.3g; "
          "phi == 1 against chi2_grid_baseline %.3g, phi == 0 %.3g of the summed bars"
          % (_worst["h"], _worst["coef"], _worst["inf"], _worst["zero"]))
    assert max(_worst.values()) <= 1.0
