"""calc_probs_datasets on the host: input validation, the reference noise sigma_bar, prepare_dataset and the ABI
entry of the weighted reduction.  No GPU: every check here ends before the first device call."""
import os
import re

import numpy as np
import pandas as pd
import pytest

from triceratops_amd import _lib, datasets as D, lightcurve as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _target():
    from triceratops_amd.triceratops import target
    stars = pd.DataFrame({"ID": [1], "Tmag": [10.0], "Jmag": [9.5], "Hmag": [9.3], "Kmag": [9.2], "ra": [0.0],
                          "dec": [0.0], "mass": [1.0], "rad": [1.0], "Teff": [5777.0], "plx": [10.0],
                          "fluxratio": [1.0], "tdepth": [0.01]})
    return target(1, np.array([1]), stars=stars)


def _ds(n=5, **kw):
    d = {"time": np.linspace(-0.1, 0.1, n), "flux": np.ones(n), "flux_err": 1e-3}
    d.update(kw)
    return d


@pytest.mark.parametrize("bad", [
    [],                                                             # an empty list
    [_ds()] * 17,                                                   # more than 16 datasets
    [_ds(flux=np.ones(4))],                                         # mismatched lengths: flux
    [_ds(flux_err=np.full(4, 1e-3))],                               # mismatched lengths: flux_err
    [_ds(flux_err=0.0)], [_ds(flux_err=-1e-3)],                     # sigma <= 0
    [_ds(flux_err=np.array([1e-3, np.inf, 1e-3, 1e-3, 1e-3]))],     # sigma not finite
    [_ds(flux_err=np.array([1e-3, np.nan, 1e-3, 1e-3, 1e-3]))],
    [_ds(flux=np.full(5, np.nan))],                                 # no points left
    [_ds(), _ds(time=np.full(5, np.nan))],
], ids=["empty", "seventeen", "flux_len", "err_len", "zero", "negative", "inf", "nan", "all_nan_flux", "all_nan_time"])
def test_validation_errors(bad):
    with pytest.raises(ValueError):
        D.validate(bad)
    with pytest.raises(ValueError):
        _target().calc_probs_datasets(bad, 3.0, N=100)


@pytest.mark.parametrize("key", ["exptime", "nsamples"])
def test_cadence_keywords_are_refused(key):
    with pytest.raises(TypeError):
        _target().calc_probs_datasets([_ds()], 3.0, **{key: 1})


def test_sixteen_datasets_are_accepted():
    assert len(D.validate([_ds()] * 16)) == 16


def test_numpy_mode_is_refused():
    import triceratops_amd as ta
    from triceratops_amd import marginal_likelihoods as ml
    mode = ta.get_sampling()
    ml._sampling["mode"] = "numpy"
    try:
        with pytest.raises(NotImplementedError):
            _target().calc_probs_datasets([_ds()], 3.0, N=100)
        with pytest.raises(NotImplementedError):
            ml.lnZ_TTP(D.Datasets(D.validate([_ds()])), None, 1e-3, 3.0, 1.0, 1.0, 5777.0, 0.0, N=100)
    finally:
        ml._sampling["mode"] = mode


def test_nan_points_are_dropped_with_their_errors():
    t = np.array([0.0, 1.0, np.nan, 3.0, 4.0])
    f = np.array([1.0, np.nan, 1.2, 1.3, 1.4])
    e = np.array([0.1, 0.2, 0.3, 0.4, 0.5])
    (s,) = D.validate([{"time": t, "flux": f, "flux_err": e, "exptime": 0.02, "nsamples": 3}])
    assert np.array_equal(s.time, [0.0, 3.0, 4.0]) and np.array_equal(s.flux, [1.0, 1.3, 1.4])
    assert np.array_equal(s.flux_err, [0.1, 0.4, 0.5]) and s.exptime == 0.02 and s.nsamples == 3
    (s,) = D.validate([{"time": t, "flux": f, "flux_err": 0.25}])            # a scalar is broadcast; the defaults
    assert np.array_equal(s.flux_err, [0.25] * 3) and s.exptime == 0.00139 and s.nsamples == 20


def test_sigma_ref():
    # by hand: errors 1 and 2 -> mean of (1, 1/4) = 5/8 -> sqrt(8/5)
    s = D.validate([{"time": [0.0, 1.0], "flux": [1.0, 1.0], "flux_err": [1.0, 2.0]}])
    assert D.sigma_ref(s) == pytest.approx(np.sqrt(1.6), rel=1e-15)
    # equal errors: sigma itself, exactly -- also over several datasets and after a renormalisation
    s = D.validate([_ds(7, flux_err=5.27e-4), _ds(3, flux_err=np.full(3, 5.27e-4))])
    assert D.sigma_ref(s) == 5.27e-4
    assert D.Datasets(s).renorm(0.83).sigma_ref == 5.27e-4 / 0.83
    # a light curve split in two (even / odd points): the same number
    rng = np.random.default_rng(5)
    t, f, e = np.linspace(-0.2, 0.2, 41), np.ones(41), rng.uniform(2e-4, 9e-4, 41)
    whole = D.sigma_ref(D.validate([{"time": t, "flux": f, "flux_err": e}]))
    split = D.sigma_ref(D.validate([{"time": t[0::2], "flux": f[0::2], "flux_err": e[0::2]},
                                    {"time": t[1::2], "flux": f[1::2], "flux_err": e[1::2]}]))
    assert whole == split and whole == pytest.approx(np.mean(e ** -2.0) ** -0.5, rel=1e-14)
    # renormalisation acts on flux and on every error; sigma_bar is taken afterwards
    r = D.Datasets(D.validate([{"time": t, "flux": f, "flux_err": e}])).renorm(0.5)
    assert np.array_equal(r.sets[0].flux_err, e / 0.5) and np.array_equal(r.sets[0].flux, (f - 0.5) / 0.5)
    assert r.sigma_ref == pytest.approx(whole / 0.5, rel=1e-14)


def test_prepare_dataset_errors_follow_the_counts():
    # 4 bins over [-0.4, 0.4): 4, 2, 0 and 1 (+ the end point's own bin) points
    t = np.array([-0.4, -0.35, -0.3, -0.25, -0.15, -0.05, 0.25, 0.4])
    y = 1.0 + 1e-3 * np.array([1.0, -1.0, 2.0, -2.0, 0.5, 1.5, -0.5, 0.0])
    d = lc.prepare_dataset(t, y, half_width=0.41, n_bins=4, n_sigma=2, exptime=0.02, nsamples=7)
    tb, yb, count = lc.bin_lightcurve(t, y, time_bin_size=2 * 0.4 / 4)
    keep = count > 0
    assert np.array_equal(d["time"], tb[keep]) and np.array_equal(d["flux"], yb[keep])
    assert d["time"].size == keep.sum() < count.size                     # the empty bin is gone
    assert d["exptime"] == 0.02 and d["nsamples"] == 7
    # one per-point scatter, divided by the root of each bin's occupancy
    s = d["flux_err"] * np.sqrt(count[keep])
    assert np.allclose(s, s[0], rtol=1e-14) and np.all(d["flux_err"] > 0)
    head, c = yb[keep][:2], count[keep][:2]
    assert s[0] == pytest.approx(np.sqrt(np.mean(c * (head - head.mean()) ** 2)), rel=1e-14)
    D.validate([d])
    # equal occupancy: every error is prepare()'s sigma
    t = np.linspace(-0.4, 0.4, 401)[:-1] + 1e-9
    y = 1.0 + 1e-3 * np.sin(37.0 * t)
    d = lc.prepare_dataset(t, y, n_bins=20, n_sigma=10)
    if np.all(np.diff(lc.bin_lightcurve(*lc.trim(t, y, 0.4), time_bin_size=2 * np.max(t) / 20)[2][:10]) == 0):
        assert np.allclose(d["flux_err"][:10], lc.prepare(t, y, n_bins=20, n_sigma=10)[2], rtol=1e-12)


def test_weighted_reduction_is_declared_and_listed():
    assert "trx_chi2_grid_weighted" in _lib.ABI_SYMBOLS
    header = open(os.path.join(ROOT, "include", "trx.h")).read()
    assert re.search(r"\bint\s+trx_chi2_grid_weighted\s*\(", header)
    declared = set(re.findall(r"\b(trx_[a-z0-9_]+)\s*\(", header))
    assert declared == set(_lib.ABI_SYMBOLS)


def test_target_has_the_entry_point():
    from triceratops_amd.triceratops import target
    assert callable(getattr(target, "calc_probs_datasets"))
    from triceratops_amd import fused
    assert fused.DATASET_GRID_BYTES == 512 << 20
