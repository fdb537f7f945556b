"""Correlated (red) noise per dataset on the host: the `red_sigma` / `red_timescale` keys of a
dataset, their renormalisation, datasets.ou_system + _numerics.ou_halfchi2 against the dense statement
0.5 y^T solve(K, y), the two exact limits of the model, and the ABI entry of the reduction (include/trx_noise.h).  No GPU:
every check here ends before the first device call.

Bars, none of them chosen from results:
  dense solve: |d h| <= 1e-9 x 0.5 sum y^2 / sigma^2 + 1e-12 while cond(K) <= 1e5 (asserted): the solve's own error is
        cond(K) x eps ~ 2e-11 of y^T K^-1 y <= sum y^2 / sigma^2;
  tau -> 0: alpha = beta = 0 exactly (exp underflows), h = 0.5 sum y^2 / (sigma^2 + s_r^2) to 1e-13 relative (T <= 333
        terms of one rounding each, summed in two orders);
  tau = inf against _numerics.offset_halfchi2(s = s_r): the row bar of tests/test_gpu_chi2_ou.py,
        1e-12 (1 + 1 / (1 - max alpha)) 0.5 sum omega (|y| + max|y|)^2 + 1e-12;
  renorm: alpha and beta to 1e-15 relative (the roundings of red_sigma / fr and flux_err / fr), omega x fr^2 likewise.
"""
import os
import re
import subprocess

import numpy as np
import pytest

from triceratops_amd import _lib, _numerics
from triceratops_amd import datasets as D
from triceratops_amd import lightcurve as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
SIGMA = 1e-3
PAIRS = [(0.3, 2.0), (3.0, 10.0), (1.0, 0.1), (3.0, 1000.0)]          # (s_r / sigma, tau / cadence)
SIZES = [1, 2, 3, 17, 65, 129, 333]


def _ds(**extra):
    d = {"time": np.linspace(-0.1, 0.1, 7), "flux": np.full(7, 0.999), "flux_err": np.linspace(1e-3, 2e-3, 7)}
    d.update(extra)
    return d


def case(T, ratio, tau, seed=0, resid_sigmas=1.0):
    """a Dataset of T irregular sorted stamps (mean cadence 1), errors varying 3x around SIGMA, with the noise keys, and
    [4][T] residuals of `resid_sigmas` x the errors"""
    rng = np.random.default_rng(1000 * T + seed)
    t = np.cumsum(rng.uniform(0.3, 1.7, T))
    err = SIGMA * rng.uniform(0.6, 1.8, T)
    y = resid_sigmas * err * rng.normal(0.0, 1.0, (4, T))
    d = D.validate([{"time": t, "flux": np.ones(T), "flux_err": err, "red_sigma": ratio * SIGMA, "red_timescale": tau}])[0]
    return d, y


def row_bar(y, alpha, omega):
    """the bar of one row of trxn_chi2_grid_ou against the long-double recurrence (tests/test_gpu_chi2_ou.py)"""
    y = np.abs(np.asarray(y, dtype=np.float64))
    top = y.max(axis=-1, keepdims=True)
    return 1e-12 * (1.0 + 1.0 / (1.0 - alpha.max())) * 0.5 * np.sum(omega * (y + top) ** 2, axis=-1) + 1e-12


# ---------------------------------------------------------------------------------------
# validation
@pytest.mark.parametrize("err", [1e-3, np.linspace(1e-3, 2e-3, 7)])
@pytest.mark.parametrize("sigma, tau", [(2e-3, 0.05), (np.float64(1e-4), INF), (3, 1), (1e-9, np.float32(0.5))])
def test_validate_accepts_the_keys(sigma, tau, err):
    got = D.validate([_ds(), _ds(flux_err=err, red_sigma=sigma, red_timescale=tau)])
    assert got[0].red_sigma is None and got[0].red_timescale is None          # absent: white noise, as before
    assert isinstance(got[1].red_sigma, float) and got[1].red_sigma == float(sigma)
    assert isinstance(got[1].red_timescale, float) and got[1].red_timescale == float(tau)
    assert not D.Datasets(got[:1]).has_red_noise and D.Datasets(got).has_red_noise
    assert D.Dataset._fields[-2:] == ("red_sigma", "red_timescale")
    alpha, beta, omega = D.ou_system(got[1])
    assert alpha.shape == beta.shape == omega.shape == (7,) and alpha.dtype == np.float64
    assert alpha[0] == 0.0 and beta[0] == 0.0 and (alpha >= 0).all() and (alpha < 1).all() and (omega > 0).all()


def test_validate_without_the_keys_is_unchanged():
    a = D.validate([_ds(offset_sigma=1e-3)])[0]
    b = D.validate([_ds(offset_sigma=1e-3, red_sigma=None, red_timescale=None)])[0]
    assert a.red_sigma is None and b.red_sigma is None and b.red_timescale is None and b.offset_sigma == 1e-3


@pytest.mark.parametrize("extra", [
    {"red_sigma": 1e-3}, {"red_timescale": 0.1},                                          # one without the other
    {"red_sigma": 0.0, "red_timescale": 0.1}, {"red_sigma": -1e-3, "red_timescale": 0.1},
    {"red_sigma": float("nan"), "red_timescale": 0.1}, {"red_sigma": INF, "red_timescale": 0.1},
    {"red_sigma": "1e-3", "red_timescale": 0.1}, {"red_sigma": True, "red_timescale": 0.1},
    {"red_sigma": [1e-3], "red_timescale": 0.1},
    {"red_sigma": 1e-3, "red_timescale": 0.0}, {"red_sigma": 1e-3, "red_timescale": -1.0},
    {"red_sigma": 1e-3, "red_timescale": float("nan")}, {"red_sigma": 1e-3, "red_timescale": "x"},
    {"red_sigma": 1e-3, "red_timescale": -INF},
    {"red_sigma": 1e-3, "red_timescale": 0.1, "offset_sigma": 1e-3},                      # not built together
    {"red_sigma": 1e-3, "red_timescale": 0.1, "offset_sigma": INF},
    {"red_sigma": 1e-3, "red_timescale": 0.1, "baseline": np.linspace(-1, 1, 7)},
])
def test_validate_rejects(extra):
    with pytest.raises(ValueError, match="dataset 1.*red_"):
        D.validate([_ds(), _ds(**extra)])


def test_validate_wants_time_order_after_dropping_nan():
    t = np.linspace(-0.1, 0.1, 7)
    folded = t[[0, 2, 4, 6, 1, 3, 5]]
    with pytest.raises(ValueError, match="dataset 0.*non-decreasing"):
        D.validate([_ds(time=folded, red_sigma=1e-3, red_timescale=0.1)])
    assert D.validate([_ds(time=folded)])[0].time.size == 7                               # without the keys: any order
    # equal stamps are in order; a NaN point is dropped before the check, whatever its time
    same = np.array([0.0, 0.0, 0.1, 0.1, 0.2, 0.3, 0.3])
    assert D.validate([_ds(time=same, red_sigma=1e-3, red_timescale=0.1)])[0].time.size == 7
    flux = np.full(7, 0.999)
    flux[3] = np.nan
    out_of_order = t.copy()
    out_of_order[3] = -5.0
    got = D.validate([_ds(time=out_of_order, flux=flux, red_sigma=1e-3, red_timescale=0.1)])[0]
    assert got.time.size == 6 and np.all(np.diff(got.time) > 0)
    hole = t.copy()
    hole[2] = np.nan
    assert D.validate([_ds(time=hole, red_sigma=1e-3, red_timescale=0.1)])[0].time.size == 6


def test_prepare_dataset_passes_the_keys_through():
    t = np.linspace(-0.4, 0.4, 400)
    y = 1.0 + 1e-3 * np.sin(37.0 * t)
    assert "red_sigma" not in lc.prepare_dataset(t, y, n_bins=20, n_sigma=10)
    d = lc.prepare_dataset(t, y, n_bins=20, n_sigma=10, red_sigma=2e-4, red_timescale=0.05)
    assert d["red_sigma"] == 2e-4 and d["red_timescale"] == 0.05
    got = D.validate([d])[0]
    assert got.red_sigma == 2e-4 and got.red_timescale == 0.05


# ---------------------------------------------------------------------------------------
# the recurrence
@pytest.mark.parametrize("ratio, tau", PAIRS)
@pytest.mark.parametrize("T", SIZES)
def test_recurrence_is_the_dense_quadratic_form(T, ratio, tau):
    d, y = case(T, ratio, tau)
    alpha, beta, omega = D.ou_system(d)
    K = np.diag(d.flux_err ** 2) + d.red_sigma ** 2 * np.exp(-np.abs(d.time[:, None] - d.time[None, :]) / d.red_timescale)
    cond = np.linalg.cond(K)
    assert cond <= 1e5, cond
    want = 0.5 * np.einsum("rt,tr->r", y, np.linalg.solve(K, y.T))
    got = _numerics.ou_halfchi2(y, alpha, beta, omega)
    bar = 1e-9 * 0.5 * np.sum(y * y / d.flux_err ** 2, axis=1) + 1e-12
    print("T %d s_r %g sigma tau %g: cond(K) %.3g, max |d h| / bar %.3g" % (T, ratio, tau, cond, np.max(np.abs(got - want) / bar)))
    assert got.shape == (4,) and got.dtype == np.float64 and (np.abs(got - want) <= bar).all()
    # properties of the coefficients: 0 <= alpha < 1, alpha + beta = phi <= 1
    assert (alpha >= 0).all() and (alpha < 1).all() and (beta >= 0).all() and (alpha + beta <= 1.0 + 1e-15).all()
    # the long-double statement is the float64 one to the row bar
    ld = _numerics.ou_halfchi2(y, alpha, beta, omega, dtype=np.longdouble)
    assert ld.dtype == np.longdouble and (np.abs(np.asarray(ld - got, dtype=np.float64)) <= row_bar(y, alpha, omega)).all()


@pytest.mark.parametrize("T", SIZES)
def test_short_timescale_is_white_noise(T):
    d, y = case(T, 3.0, 1e-6)
    alpha, beta, omega = D.ou_system(d)
    assert not alpha.any() and not beta.any()
    assert np.array_equal(omega, 1.0 / (d.red_sigma ** 2 + d.flux_err ** 2))
    want = 0.5 * np.sum(y * y / (d.flux_err ** 2 + d.red_sigma ** 2), axis=1)
    got = _numerics.ou_halfchi2(y, alpha, beta, omega)
    assert (np.abs(got - want) <= 1e-13 * want).all()


@pytest.mark.parametrize("ratio", [0.3, 1.0, 3.0])
@pytest.mark.parametrize("T", SIZES)
def test_infinite_timescale_is_the_marginalised_offset(T, ratio):
    d, y = case(T, ratio, INF)
    y = y + 2.0 * SIGMA                                     # residuals carrying an offset
    alpha, beta, omega = D.ou_system(d)
    assert np.allclose(alpha[1:] + beta[1:], 1.0, rtol=0, atol=1e-15)
    got = _numerics.ou_halfchi2(y, alpha, beta, omega)
    want = _numerics.offset_halfchi2(y, 1.0 / d.flux_err ** 2, d.red_sigma)
    bar = row_bar(y, alpha, omega)
    print("T %d s_r %g sigma: max |d h| / bar %.3g" % (T, ratio, np.max(np.abs(got - want) / bar)))
    assert (np.abs(got - want) <= bar).all()


@pytest.mark.parametrize("fr", [1.0, 0.5, 0.37, 1.0 / 3.0, 0.0123])
def test_renorm_scales_red_sigma_with_the_errors(fr):
    d, _ = case(65, 3.0, 10.0)
    sets = D.Datasets([d, D.validate([_ds()])[0]])
    star = sets.renorm(fr)
    assert star.sets[0].red_sigma == d.red_sigma / fr and star.sets[0].red_timescale == d.red_timescale
    assert star.sets[1].red_sigma is None and star.has_red_noise
    a0, b0, w0 = D.ou_system(d)
    a1, b1, w1 = D.ou_system(star.sets[0])
    assert np.allclose(a1, a0, rtol=1e-15, atol=0) and np.allclose(b1, b0, rtol=1e-15, atol=0)
    assert np.allclose(w1, w0 * fr * fr, rtol=1e-15, atol=0)
    if fr in (1.0, 0.5):
        assert np.array_equal(a1, a0) and np.array_equal(b1, b0)          # a power of two: no rounding at all


# ---------------------------------------------------------------------------------------
# the ABI
def _declared():
    text = open(os.path.join(ROOT, "include", "trx_noise.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(trxn_[a-z0-9_]+)\s*\(", text)))


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(ln.split()[-1] for ln in out.splitlines() if " T " in ln)


def test_header_libraries_and_binding_list_the_same_symbols():
    assert _declared() == sorted(_lib.NOISE_SYMBOLS) == ["trxn_chi2_grid_ou"]
    assert not set(_lib.NOISE_SYMBOLS) & (set(_lib.ABI_SYMBOLS) | set(_lib.WARP_SYMBOLS))
    assert callable(_lib.chi2_grid_ou)
    for other in ("trx.h", "trx_warp.h", "trx_debug.h"):
        assert "trxn_" not in open(os.path.join(ROOT, "include", other)).read()
    if not (os.path.exists(_lib.LIB_PATH) and os.path.exists(_lib.TESTING_LIB_PATH)):
        pytest.skip("libtrx.so not built")
    for path in (_lib.LIB_PATH, _lib.TESTING_LIB_PATH):
        assert [s for s in _exports(path) if s.startswith("trxn_")] == _declared()


def test_argument_checks_need_no_gpu():
    """every refusal comes before anything touches a device: the pointers below are not device memory"""
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libtrx.so not built")
    L = _lib.lib()
    v = [np.zeros(4) for _ in range(7)]
    f, g, o, a, b, w, s = (x.ctypes.data for x in v)
    call = L.trxn_chi2_grid_ou
    ERR_ARG = 1
    assert call(None, g, 2, 2, s, INF, 0, o, a, b, w, None) == ERR_ARG              # NULL flux
    assert call(f, None, 2, 2, s, INF, 0, o, a, b, w, None) == ERR_ARG              # NULL grid
    assert call(f, g, 2, 2, s, INF, 0, None, a, b, w, None) == ERR_ARG              # NULL out
    assert call(f, g, 2, 2, s, INF, 0, o, None, b, w, None) == ERR_ARG              # NULL alpha
    assert call(f, g, 2, 2, s, INF, 0, o, a, None, w, None) == ERR_ARG              # NULL beta
    assert call(f, g, 2, 2, s, INF, 0, o, a, b, None, None) == ERR_ARG              # NULL omega
    assert call(f, g, 2, -1, s, INF, 0, o, a, b, w, None) == ERR_ARG                # n < 0
    assert call(f, g, 0, 2, s, INF, 0, o, a, b, w, None) == ERR_ARG                 # n_time < 1
    assert call(f, g, -3, 0, s, INF, 0, o, a, b, w, None) == ERR_ARG                # ... also with no rows
    assert b"null pointer" in L.trx_last_error() or b"n_time" in L.trx_last_error()
    assert call(f, g, 2, 0, None, INF, 0, o, a, b, w, None) == 0                    # n == 0: nothing to launch
    assert not any(x.any() for x in v)
