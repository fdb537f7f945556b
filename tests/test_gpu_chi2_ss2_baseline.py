"""scan_rows_kernel<ONE, Ss2ColsFilter<K>> (trxk_chi2_grid_ss2_baseline, include/trx_ss.h): the row
reduction of a model grid under white noise plus a process with a two-dimensional state (a Matern-3/2 term, two exponential
terms) with K baseline columns marginalised under that noise,
    z = the innovations of y = flux - grid[r],  S2 = sum omega z^2,  b~_k = sum c_k z,  h = 0.5 max(S2 - b~^T M b~, 0),
    coef = M b~,   c_k = omega z[B_k] / sqrt(D_k) and M = A~^-1 from datasets.ss2_baseline_system.

The yardstick is _numerics.ss2_baseline_halfchi2 in np.longdouble on the downloaded grid and the tables the device holds.
Bars, not chosen from results (ss2_gls_bar, ss2_coef_bar of tests/test_datasets_red_kernel_baseline_api.py):
  |d h| <= (ss2_bar - 1e-12) (1 + 4 sqrt(K / lambda_min)) + 1e-12: ss2_bar of tests/test_gpu_chi2_ss2.py -- the roundings
        of the recurrence through the predictor's l1 gain Gamma -- times the projection factor of
        tests/test_gpu_chi2_baseline.py;
  coef_out: 1e-12 (1 + Gamma) sqrt(K sum omega (|y| + Gamma max|y|)^2) / lambda_min + 1e-15 per entry;
  minv = 0: the bits of _lib.chi2_grid_ss2 (the same ss2_innovations, S2 formed term for term the same way; S2 - 0 = S2);
  cross-kernel: A = [[alpha, 0], [0, 0]], g = (beta, 0) from datasets.ou_system (shifted by one stamp: u_n is the prediction
        for stamp n + 1) with the columns and M of datasets.ou_baseline_system is chi2_grid_ou_baseline's reduction: to the
        sum of the two kernels' bars (gls_bar of tests/test_datasets_red_baseline_api.py and ss2_gls_bar on the same system).
Shapes: as many stamps as columns and one more, both sides of a lane's last pair (63, 64, 65), of one trip of 128 stamps
(128, 129) -- the two instantiations --, odd lengths (every second row off its 16-byte boundary), many trips (333, 2049);
odd row counts; and (CAPPED) 8 x the capped grid's blocks + 3 rows: rows in a wave's second slot and in its second pass.
Columns u^p, p = 0 .. K - 1; PARAMS of the ss2 file; residual levels 0, 3 and 100 mean sigma; flat priors and A~ + I.  Per
shape and K every parameter set meets both priors, the level rotating so that over K = 1 .. 4 every (set, prior) meets
every level.
Measured (one MI355X, test_zz_report_the_largest_ratios): the largest |d h| / bar of the whole file 7.3e-5, the largest
|d coef| / bar 2.0e-4 (Gamma up to 1.82, lambda_min down to 0.027); one-state tables against chi2_grid_ou_baseline at most
2.9e-6 of the summed bars, the same bits wherever alpha = 0."""
import numpy as np
import pytest
import torch

from test_datasets_red_baseline_api import coef_bar, gls_bar
from test_datasets_red_kernel_api import keys
from test_datasets_red_kernel_baseline_api import ss2_coef_bar, ss2_gls_bar
from test_datasets_red_noise_api import PAIRS, SIGMA
from test_gpu_chi2_ss2 import PARAMS, gain
from triceratops_amd import _lib, _numerics, synth
from triceratops_amd import datasets as D

pytestmark = pytest.mark.gpu

KS = [1, 2, 3, 4]
N_TIMES = ["K", "K+1", 63, 64, 65, 128, 129, 333, 2049]
NS = [1, 2, 3, 257]
CAPPED = [(4, 65), (2, 2048)]                # (K, n_time); n = 8 x the capped grid's blocks + 3
LEVELS = (0.0, 3.0, 100.0)                   # residual offsets, in mean sigma
PRIORS = ("flat", "plus_identity")
INF = float("inf")
LD = np.longdouble
_cases, _systems, _gains = {}, {}, {}
_worst = {"h": 0.0, "coef": 0.0, "ou": 0.0, "gamma": 0.0, "lambda_min": INF}


def _n_time(spec, K):
    return K if spec == "K" else K + 1 if spec == "K+1" else spec


def _capped_n(K, n_time):
    return 8 * _lib.ss2_baseline_blocks(10 ** 9, n_time, K) + 3


def _unit(t):
    return (t - 0.5 * (t[0] + t[-1])) / (0.5 * (t[-1] - t[0])) if t.size > 1 else np.zeros(1)


def _tables(n_time):
    """the light curve's stamps and errors (one per n_time: those of tests/test_gpu_chi2_ss2.py)"""
    rng = np.random.default_rng(synth.SEED + 104729 * n_time)
    return np.cumsum(rng.uniform(0.3, 1.7, n_time)), SIGMA * rng.uniform(0.6, 1.8, n_time)


def _system(n_time, kernel, ratio, scale, K, prior):
    """the system of the columns u^p, p = 0 .. K - 1, under one parameter set and one prior, its tables on the device and
    the predictor's gain"""
    key = (n_time, kernel, ratio, scale, K, prior)
    if key not in _systems:
        t, err = _tables(n_time)
        d = D.validate([dict(time=t, flux=np.ones(n_time), flux_err=err, **keys(kernel, ratio, scale))])[0]
        u = _unit(d.time)
        B = np.stack([u ** p for p in range(K)])
        s = D.ss2_baseline_system(d, B, INF)
        if prior == "plus_identity":
            s = D.ss2_baseline_system(d, B, 1.0 / np.sqrt(s.D))                # 1 / (s_k^2 D_k) = 1
        assert s.lambda_min >= D.MIN_BASELINE_EIGENVALUE, (key, s.lambda_min)
        if key[:4] not in _gains:
            _gains[key[:4]] = gain(s.A, s.g)
        _systems[key] = dict(d=d, B=B, s=s, gamma=_gains[key[:4]],
                             dev=tuple(_lib.dev(np.ascontiguousarray(v)) for v in (s.A, s.g, s.omega, s.c)))
        _worst["gamma"] = max(_worst["gamma"], _gains[key[:4]])
        _worst["lambda_min"] = min(_worst["lambda_min"], s.lambda_min)
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
    return _lib.chi2_grid_ss2_baseline(f_d, g_d, *S["dev"], S["s"].minv, **kw)


def _check(K, n_time, n, combos, rows=None):
    """combos: (kernel, ratio, scale, prior, level); rows: the rows held against the long-double statement (None: all) --
    the other rows are then held, bit for bit, against launches of 2048 rows: 512 blocks, below every cap, one row a wave"""
    c = _case(n_time, n)
    rows = np.arange(n) if rows is None else np.asarray(rows)
    for kernel, ratio, scale, prior, level in combos:
        S = _system(n_time, kernel, ratio, scale, K, prior)
        s, gamma = S["s"], S["gamma"]
        flux = c["flux"][level]
        f_d = _lib.dev(flux)
        y = flux[None, :] - c["g"][rows]
        ref, cref = _numerics.ss2_baseline_halfchi2(y, s, dtype=LD, return_coef=True)
        coef = torch.full((n, K), float("nan"), dtype=torch.float64, device=c["g_d"].device)
        got = _call(f_d, c["g_d"], S, coef_out=coef)
        h = got.cpu().numpy()
        r_h = float((np.abs(h[rows].astype(LD) - ref).astype(np.float64) / ss2_gls_bar(y, s, gamma)).max())
        r_c = float((np.abs(coef.cpu().numpy()[rows].astype(LD) - cref).astype(np.float64)
                     / ss2_coef_bar(y, s, gamma)[:, None]).max())
        if rows.size < n:
            for r0 in range(0, n, 2048):
                part_c = torch.empty((min(2048, n - r0), K), dtype=torch.float64, device=coef.device)
                part = _call(f_d, c["g_d"][r0:r0 + 2048], S, coef_out=part_c)
                assert torch.equal(part, got[r0:r0 + 2048]) and torch.equal(part_c, coef[r0:r0 + 2048])
        _worst["h"], _worst["coef"] = max(_worst["h"], r_h), max(_worst["coef"], r_c)
        print("K %d n_time %d n %d %s s %g sigma scale %g %s level %g sigma: Gamma %.4f lambda_min %.3g, |d h| / bar %.3g, "
              "|d coef| / bar %.3g (largest so far %.3g, %.3g)"
              % (K, n_time, n, kernel, ratio, scale, prior, level, gamma, s.lambda_min, r_h, r_c, _worst["h"], _worst["coef"]))
        assert r_h <= 1.0 and r_c <= 1.0
        assert (h >= 0.0).all()
        # without coef_out, one double off the 16-byte boundary, and again: the same bits
        assert torch.equal(_call(f_d, c["g_d"], S), got)
        coef2 = torch.empty_like(coef)
        assert torch.equal(_call(f_d, c["g_off"], S, coef_out=coef2), got) and torch.equal(coef2, coef)
        assert torch.equal(_call(f_d, c["g_d"], S, coef_out=coef2), got) and torch.equal(coef2, coef)


def _combos(K, salt):
    return [(kernel, ratio, scale, prior, LEVELS[(i + j + K + salt) % 3])
            for i, (kernel, ratio, scale) in enumerate(PARAMS) for j, prior in enumerate(PRIORS)]


@pytest.mark.parametrize("spec, n", [(t, n) for n in NS for t in N_TIMES])
def test_reduction_matches_longdouble(spec, n):
    for K in KS:
        _check(K, _n_time(spec, K), n, _combos(K, N_TIMES.index(spec) + n))


@pytest.mark.parametrize("K, n_time", CAPPED)
def test_reduction_past_the_capped_grid(K, n_time):
    n = _capped_n(K, n_time)
    waves = 4 * _lib.ss2_baseline_blocks(n, n_time, K)
    assert 2 * waves < n <= 2 * waves + 3
    # the long-double statement on rows of a wave's first slot, around the start of its second slot, and at the end (the
    # second pass: the last three rows); every row against launches that stay in the first slot
    rows = np.unique(np.concatenate([np.arange(64), np.arange(waves - 32, waves + 96), np.arange(n - 64, n)]))
    _check(K, n_time, n, [(kernel, ratio, scale, PRIORS[i % 2], 3.0) for i, (kernel, ratio, scale) in enumerate(PARAMS)],
           rows=rows)


@pytest.mark.parametrize("n_time, n", [(1, 3), (2, 257), (65, 257), (128, 3), (129, 257), (333, 2), (2049, 257)])
def test_minv_zero_gives_the_ss2_kernels_bits(n_time, n):
    c = _case(n_time, n)
    for K in KS:
        if K > n_time:
            continue
        for params in (PARAMS[0], PARAMS[2], PARAMS[-1]):
            S = _system(n_time, *params, K, "flat")
            for level in (0.0, 100.0):
                f_d = _lib.dev(c["flux"][level])
                want = _lib.chi2_grid_ss2(f_d, c["g_d"], *S["dev"][:3])
                coef = torch.full((n, K), float("nan"), dtype=torch.float64, device=c["g_d"].device)
                got = _lib.chi2_grid_ss2_baseline(f_d, c["g_d"], *S["dev"], np.zeros(K * (K + 1) // 2), coef_out=coef)
                assert torch.equal(got, want) and (got > 0).all()
                assert not coef.any()                                      # M = 0: the coefficients are 0
                off = _lib.chi2_grid_ss2_baseline(f_d, c["g_off"], *S["dev"], np.zeros(K * (K + 1) // 2))
                assert torch.equal(off, want)


def test_minv_zero_gives_the_ss2_kernels_bits_past_the_capped_grid():
    K, n_time = CAPPED[0]
    n = _capped_n(K, n_time)
    c = _case(n_time, n)
    S = _system(n_time, *PARAMS[0], K, "flat")
    f_d = _lib.dev(c["flux"][3.0])
    want = _lib.chi2_grid_ss2(f_d, c["g_d"], *S["dev"][:3])
    assert torch.equal(_lib.chi2_grid_ss2_baseline(f_d, c["g_d"], *S["dev"], np.zeros(K * (K + 1) // 2)), want)


@pytest.mark.parametrize("K, n_time, n", [(1, 65, 257), (3, 65, 257), (4, 2049, 257), (2, 129, 257), (4, 65, None),
                                          (2, 2048, None)])
def test_a_rows_bits_are_its_own(K, n_time, n):
    """row r of the grid against the same row alone, at position 0, 1 and n - 1 (behind the capped grid where n is the
    capped case's), in a view one double off, and on a second run"""
    n = _capped_n(K, n_time) if n is None else n
    c = _case(n_time, n)
    for params in (PARAMS[0], PARAMS[3]):
        S = _system(n_time, *params, K, "flat")
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


@pytest.mark.parametrize("ratio, tau", PAIRS)
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("n_time, n", [(5, 3), (65, 257), (128, 257), (129, 257), (2049, 257)])
def test_one_state_tables_are_the_ou_baseline_kernel(n_time, n, K, ratio, tau):
    c = _case(n_time, n)
    t, err = _tables(n_time)
    d = D.validate([{"time": t, "flux": np.ones(n_time), "flux_err": err, "red_sigma": ratio * SIGMA, "red_timescale": tau}])[0]
    u = _unit(d.time)
    B = np.stack([u ** p for p in range(K)])
    for sig in (INF, 30.0 * 1.2 * SIGMA):
        s = D.ou_baseline_system(d, B, sig)
        assert s.lambda_min >= D.MIN_BASELINE_EIGENVALUE
        A, g = np.zeros((n_time, 2, 2)), np.zeros((n_time, 2))
        A[:-1, 0, 0], g[:-1, 0] = s.alpha[1:], s.beta[1:]
        gamma = gain(A, g)
        assert gamma <= 1.0 + 1e-12                               # (alpha + beta <= 1: a convex predictor)
        ou_d = tuple(_lib.dev(v) for v in (s.alpha, s.beta, s.omega))
        ss_d = tuple(_lib.dev(v) for v in (A, g, s.omega))
        c_d = _lib.dev(s.c)
        for k in LEVELS:
            flux = c["flux"][k]
            f_d = _lib.dev(flux)
            y = flux[None, :] - c["g"]
            cg = torch.empty((n, K), dtype=torch.float64, device=f_d.device)
            cw = torch.empty_like(cg)
            got = _lib.chi2_grid_ss2_baseline(f_d, c["g_d"], *ss_d, c_d, s.minv, coef_out=cg).cpu().numpy()
            want = _lib.chi2_grid_ou_baseline(f_d, c["g_d"], *ou_d, c_d, s.minv, coef_out=cw).cpu().numpy()
            bar = gls_bar(y, s) + ss2_gls_bar(y, s, gamma)
            r = float((np.abs(got - want) / bar).max())
            _worst["ou"] = max(_worst["ou"], r)
            print("K %d n_time %d s_r %g sigma tau %g prior %g level %g: against chi2_grid_ou_baseline |d h| / bar %.3g, the "
                  "same bits in %d of %d rows" % (K, n_time, ratio, tau, sig, k, r, (got == want).sum(), n))
            assert r <= 1.0
            assert (np.abs((cg - cw).cpu().numpy()) <= (coef_bar(y, s) + ss2_coef_bar(y, s, gamma))[:, None]).all()


@pytest.mark.parametrize("K, n_time, n", [(1, 64, 257), (3, 333, 257), (4, 2049, 257), (4, 65, None)],
                         ids=["64", "333", "2049", "65-capped"])
def test_accumulates_onto_finite_inf_and_nan(K, n_time, n):
    n = _capped_n(K, n_time) if n is None else n
    c = _case(n_time, n)
    S = _system(n_time, *PARAMS[0], K, "flat")
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
    # an all-+inf target stays +inf
    acc = _call(f_d, c["g_d"], S, out=torch.full((n,), INF, dtype=torch.float64, device=f_d.device))
    assert np.isposinf(acc.cpu().numpy()).all()
    # with a rule of its own: +inf from either side
    sec = np.linspace(0.0, 1.0, n)
    acc = _call(f_d, c["g_d"], S, secdepth=_lib.dev(sec), sec_limit=0.5, out=_lib.dev(out0).clone()).cpu().numpy()
    assert np.array_equal(np.isposinf(acc), (np.isposinf(out0) | (sec >= 0.5)) & ~np.isnan(out0))


@pytest.mark.parametrize("K, n_time", [(2, 65), (4, 2049)])
def test_secondary_rule_is_the_weighted_kernels(K, n_time):
    c = _case(n_time, 257)
    S = _system(n_time, *PARAMS[-1], K, "plus_identity")
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
    for params in (PARAMS[0], PARAMS[2], PARAMS[-1]):
        S = _system(n_time, *params, K, "plus_identity")
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
    S = _system(63, *PARAMS[0], 2, "flat")
    f_d = _lib.dev(c["flux"][0.0])
    assert _call(f_d, c["g_d"][:0], S).shape == (0,)
    A, g, w, cols = S["dev"]
    with pytest.raises(AssertionError):
        _lib.chi2_grid_ss2_baseline(f_d, c["g_d"], A[:5], g, w, cols, S["s"].minv)
    with pytest.raises(AssertionError):
        _lib.chi2_grid_ss2_baseline(f_d, c["g_d"], A, w, w, cols, S["s"].minv)              # g of [n_time]: half the table
    with pytest.raises(AssertionError):
        _lib.chi2_grid_ss2_baseline(f_d, c["g_d"], A, g, w, cols[:, :5], S["s"].minv)
    with pytest.raises(AssertionError):
        _lib.chi2_grid_ss2_baseline(f_d, c["g_d"], A, g, w, cols, S["s"].minv[:2])
    with pytest.raises(AssertionError):
        _lib.chi2_grid_ss2_baseline(f_d, c["g_d"], A, g, w, torch.cat([cols, cols, cols]), np.zeros(21))
    with pytest.raises(AssertionError):
        _lib.chi2_grid_ss2_baseline(f_d, c["g_d"], A, g, w, cols, S["s"].minv,
                                    coef_out=torch.empty((3, 3), dtype=torch.float64, device=f_d.device))
    # through the ABI itself: a refusal enqueues nothing, n == 0 launches nothing
    call = _lib.lib().trxk_chi2_grid_ss2_baseline
    args = (f_d.data_ptr(), c["g_d"].data_ptr(), 63, 3, None, INF, 0, f_d.data_ptr(), A.data_ptr(), g.data_ptr(), w.data_ptr(),
            cols.data_ptr())
    assert call(*args, 5, S["s"].minv.ctypes.data, None, None) == 1
    bad = np.full(3, np.nan)
    assert call(*args, 2, bad.ctypes.data, None, None) == 1
    assert call(*args[:3], 0, *args[4:], 2, S["s"].minv.ctypes.data, None, None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(f_d.cpu().numpy(), c["flux"][0.0])       # (the `out` of the refused calls: untouched)


def test_zz_report_the_largest_ratios():
    """(runs last in the file: the figures DESIGN.md section 14 and the README quote)"""
    print("Ss2ColsFilter against np.longdouble: largest |d h| / bar over the file %.3g, largest |d coef| / bar %.3g (Gamma up "
          "to %.4g, lambda_min down to %.3g); one-state tables against chi2_grid_ou_baseline %.3g of the summed bars"
          % (_worst["h"], _worst["coef"], _worst["gamma"], _worst["lambda_min"], _worst["ou"]))
    assert max(_worst["h"], _worst["coef"], _worst["ou"]) <= 1.0
