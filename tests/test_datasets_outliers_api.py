"""The outlier-tolerant likelihood per dataset on the host: the `outlier_frac` / `outlier_scale` keys and
datasets.outliers, their way through Datasets and renorm, datasets.robust_constants, _numerics.robust_halfchi2 and
robust_responsibility, and the ABI entry of the reduction (include/trx_robust.h).  No GPU: every check here ends before the
first device call.

Bars, none of them chosen from results:
  robust_halfchi2 in float64 against the same function in np.longdouble, both on the same double constants:
        |d h| <= 1e-12 sum_t (1 + lo_t) + 1e-12, lo_t from the long-double pass -- the path's own bar for a sum of
        non-negative terms of this length (tests/test_gpu_chi2_offset.py::_bar); the 1 per point covers the log1p term,
        which is at most ln 2.  Measured here: the largest |d h| / bar over the inputs below is 3e-4;
  the two upper bounds, h >= 0 and the renormalised dataset: to the same bar.

robust_inputs() is also what tests/test_gpu_chi2_robust.py feeds the kernel.
"""
import math
import os
import re
import subprocess

import numpy as np
import pytest

from triceratops_amd import _lib, _numerics
from triceratops_amd import datasets as D
from triceratops_amd import lightcurve as lc
from triceratops_amd.funcs import renorm_flux

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
NAN = float("nan")
PAIRS = [(0.01, 5.0), (0.5, 1.5), (1e-6, 100.0), (0.05, 10.0)]
OFFS = (1.0, 5.0, 100.0)
LD = np.longdouble


def _ds(**keys):
    t = np.linspace(-0.1, 0.1, 7)
    return dict({"time": t, "flux": 1.0 - 1e-3 * (np.abs(t) < 0.04), "flux_err": 1e-3}, **keys)


def robust_inputs(n_time, n, off, seed=0):
    """(flux [T], inv_var [T], grid [n][T]): a grid near 1, errors of 1e-3 spanning sqrt(10) (weights spanning 10x), a light
    curve `off` sigma above 1.  Rows 0 .. n - 1 do not depend on n."""
    rng = np.random.default_rng(1000 * n_time + seed)
    sigma = 1e-3 * 10.0 ** rng.uniform(0.0, 0.5, n_time)
    flux = 1.0 + off * sigma
    grid = 1.0 + 3e-4 * np.random.default_rng(7 * n_time + seed + 1).normal(size=(257, n_time))
    assert n <= 257
    return flux, 1.0 / (sigma * sigma), np.ascontiguousarray(grid[:n])


def robust_reference(flux, inv_var, grid, consts):
    """(h in long double, the bar per row)"""
    d = flux.astype(LD) - grid.astype(LD)
    w = inv_var.astype(LD)
    h = _numerics.robust_halfchi2(d, w, *consts)
    a = LD(0.5) * w * d * d
    lo = np.minimum(a + LD(consts[0]), a * LD(consts[2]) + LD(consts[1]))
    return h, np.asarray(1e-12 * np.sum(1.0 + lo, axis=-1) + 1e-12, dtype=np.float64)


# ---------------------------------------------------------------------------------------
# the keys
@pytest.mark.parametrize("pair", [(0.01, 5.0), (0.5, 1.0000001), (np.float64(1e-6), 100), (0.05, np.float32(10))])
def test_validate_accepts(pair):
    dicts = [_ds(), _ds(outlier_frac=pair[0], outlier_scale=pair[1]), _ds(outlier_frac=None, outlier_scale=None)]
    sets = D.validate(dicts)
    got = D.outliers(dicts, sets)
    assert isinstance(got, list) and got[0] is None and got[2] is None
    assert isinstance(got[1], tuple) and all(type(v) is float for v in got[1])
    assert got[1] == (float(pair[0]), float(pair[1]))
    with pytest.raises(ValueError):
        D.outliers(dicts[:2], sets)


@pytest.mark.parametrize("keys", [
    {"outlier_frac": 0.1}, {"outlier_scale": 5.0}, {"outlier_frac": 0.1, "outlier_scale": None},
    {"outlier_frac": None, "outlier_scale": 5.0},
] + [{"outlier_frac": f, "outlier_scale": 5.0} for f in (0, 0.0, -0.1, 0.6, NAN, INF, "0.1", True, [0.1], np.array([0.1]))]
  + [{"outlier_frac": 0.1, "outlier_scale": s} for s in (1.0, 0.5, NAN, INF, "5", True, [5.0])])
def test_validate_rejects(keys):
    with pytest.raises(ValueError, match=r"dataset 1.*outlier_"):
        D.validate([_ds(), _ds(**keys)])


@pytest.mark.parametrize("extra", [{"offset_sigma": 1e-3}, {"baseline": np.linspace(-1, 1, 7), "baseline_sigma": 2.0},
                                   {"red_sigma": 1e-3, "red_timescale": 0.1},
                                   {"red_grid": [(1e-3, 0.1, 1.0), (2e-3, INF, 1.0)]}])
def test_the_keys_stand_alone_or_next_to_a_t0_grid(extra):
    D.validate([_ds(), _ds(**extra)])
    with pytest.raises(ValueError, match=r"dataset 1.*outlier_"):
        D.validate([_ds(), _ds(outlier_frac=0.05, outlier_scale=10.0, **extra)])
    with pytest.raises(ValueError, match=r"dataset 0.*outlier_"):
        D.validate([_ds(outlier_scale=10.0, outlier_frac=0.05, **extra)])
    dicts = [_ds(outlier_frac=0.05, outlier_scale=10.0, t0_grid=[(-0.01, 1.0), (0.01, 3.0)])]
    sets = D.validate(dicts)
    assert D.outliers(dicts, sets) == [(0.05, 10.0)] and D.t0_grids(dicts, sets)[0].shape == (2, 2)


def test_dataset_is_unchanged_and_datasets_carries_the_pairs():
    assert D.Dataset._fields == ("time", "flux", "flux_err", "exptime", "nsamples", "offset_sigma", "baseline",
                                 "baseline_sigma", "red_grid", "red_sigma", "red_timescale")
    dicts = [_ds(), _ds(outlier_frac=0.05, outlier_scale=10.0)]
    a, b = D.validate([_ds(), _ds()]), D.validate(dicts)
    for x, y in zip(a, b):
        for name, u, v in zip(x._fields, x, y):
            assert (np.array_equal(u, v) if isinstance(u, np.ndarray) else u == v), name
    with pytest.raises(ValueError, match="unknown key"):
        D.validate([_ds(outlier_fraction=0.1)])
    pairs = D.outliers(dicts, b)
    plain, ds = D.Datasets(b), D.Datasets(b, None, pairs)
    assert plain.outliers == (None, None) and not plain.has_outliers and not plain.has_t0_grids
    assert ds.has_outliers and ds.outliers == (None, (0.05, 10.0)) and not ds.has_t0_grids
    with pytest.raises(ValueError):
        D.Datasets(b, None, pairs[:1])
    with pytest.raises(ValueError):
        D.Datasets(b, None, pairs + [None])
    star = ds.renorm(0.83)
    assert star.has_outliers and star.outliers == ds.outliers
    assert not plain.renorm(0.83).has_outliers
    for x, y in zip(star.sets, plain.renorm(0.83).sets):
        assert np.array_equal(x.flux, y.flux) and np.array_equal(x.flux_err, y.flux_err)
    assert star.sigma_ref == plain.renorm(0.83).sigma_ref and ds.sigma_ref == plain.sigma_ref


def test_prepare_dataset_passes_the_keys_through():
    rng = np.random.default_rng(1)
    t = np.sort(rng.uniform(-0.5, 0.5, 4000))
    f = 1.0 + 1e-3 * rng.normal(size=t.size)
    plain = lc.prepare_dataset(t, f)
    assert "outlier_frac" not in plain and "outlier_scale" not in plain
    keyed = lc.prepare_dataset(t, f, outlier_frac=0.02, outlier_scale=8.0)
    assert set(keyed) == set(plain) | {"outlier_frac", "outlier_scale"}
    assert keyed["outlier_frac"] == 0.02 and keyed["outlier_scale"] == 8.0
    assert all(np.array_equal(np.asarray(plain[k], dtype=object), np.asarray(keyed[k], dtype=object)) for k in plain)
    keyed["offset_sigma"] = None
    assert D.outliers([keyed], D.validate([keyed])) == [(0.02, 8.0)]
    with pytest.raises(ValueError, match="outlier_"):
        D.validate([lc.prepare_dataset(t, f, outlier_frac=0.02)])


# ---------------------------------------------------------------------------------------
# the constants and the numpy statement
@pytest.mark.parametrize("frac,scale", PAIRS + [(0.5, 1.0000001)])
def test_robust_constants_against_their_definition(frac, scale):
    c0, c1, k2 = D.robust_constants(frac, scale)
    assert all(type(v) is float for v in (c0, c1, k2))
    assert c0 == -math.log1p(-frac) and c1 == math.log(scale) - math.log(frac) and k2 == 1.0 / (scale * scale)
    assert c0 >= 0 and c1 > 0 and 0 < k2 < 1
    # the mixture's weights: exp(-c0) = 1 - eps, exp(-c1) = eps / kappa
    assert abs(math.exp(-c0) - (1.0 - frac)) <= 4e-16 and abs(math.exp(-c1) - frac / scale) <= 4e-16 * frac / scale * (1 + c1)


@pytest.mark.parametrize("n_time", [1, 2, 63, 64, 65, 129, 333, 2048, 2049, 70001])
def test_statement_in_double_against_long_double_and_its_bounds(n_time):
    n = 3
    worst = 0.0
    for pair in PAIRS:
        consts = D.robust_constants(*pair)
        c0, c1, k2 = consts
        for off in OFFS:
            flux, w, grid = robust_inputs(n_time, n, off)
            want, bar = robust_reference(flux, w, grid, consts)
            got = _numerics.robust_halfchi2(flux - grid, w, *consts)
            assert got.dtype == np.float64 and got.shape == (n,) and want.dtype == LD
            err = np.abs((got.astype(LD) - want).astype(np.float64))
            worst = max(worst, float(np.max(err / bar)))
            assert (err <= bar).all(), (pair, off, err, bar)
            assert (got >= 0).all()
            half = 0.5 * np.sum(w * (flux - grid) ** 2, axis=1)
            assert (got <= half + n_time * c0 + bar).all()
            assert (got <= k2 * half + n_time * c1 + bar).all()
    print("n_time %d: max |d h| / bar %.3g" % (n_time, worst))


def test_one_point_is_the_closed_form_and_nan_stays_nan():
    for frac, scale in PAIRS:
        c = D.robust_constants(frac, scale)
        for z in (0.0, 0.3, 1.0, 5.0, 8.0, 100.0):
            a = LD(0.5) * LD(z) * LD(z)
            want = -np.log((LD(1) - LD(frac)) * np.exp(-a) + LD(frac) / LD(scale) * np.exp(-a / (LD(scale) * LD(scale))))
            got = _numerics.robust_halfchi2(np.array([z * 1e-3]), np.array([1e6]), *c)
            assert got.shape == () and abs(float(LD(got) - want)) <= 1e-12 * (1.0 + float(want)) + 1e-12, (frac, scale, z)
    c = D.robust_constants(0.05, 10.0)
    r = np.array([[1e-3, NAN, 2e-3], [1e-3, 0.0, 2e-3]])
    got = _numerics.robust_halfchi2(r, np.full(3, 1e6), *c)
    assert np.isnan(got[0]) and np.isfinite(got[1])
    assert _numerics.robust_halfchi2(r.astype(np.float32), np.full(3, 1e6), *c).dtype == np.float32


@pytest.mark.parametrize("frac,scale", PAIRS)
def test_responsibility(frac, scale):
    c = D.robust_constants(frac, scale)
    z = np.concatenate([[0.0], np.linspace(0.01, 12.0, 400)])
    p = _numerics.robust_responsibility(z * 1e-3, np.full(z.size, 1e6), *c)
    assert p.shape == z.shape and p.dtype == np.float64
    assert ((p >= 0) & (p <= 1)).all() and (np.diff(p) >= 0).all() and p[-1] > p[0]
    prior = (frac / scale) / ((1.0 - frac) + frac / scale)
    assert abs(p[0] - prior) <= 8e-16 * (1 + c[1])
    assert np.array_equal(p, _numerics.robust_responsibility(-z * 1e-3, np.full(z.size, 1e6), *c))
    assert _numerics.robust_responsibility((z * 1e-3).astype(LD), np.full(z.size, 1e6), *c).dtype == LD


@pytest.mark.parametrize("fr", [0.83, 0.37, 0.0123])
def test_a_renormalised_dataset_gives_the_same_term(fr):
    for pair in PAIRS:
        consts = D.robust_constants(*pair)
        for off in OFFS:
            flux, w, grid = robust_inputs(333, 3, off)
            err = 1.0 / np.sqrt(w)
            want, bar = robust_reference(flux, w, grid, consts)
            f2, e2 = renorm_flux(flux, err, fr)
            g2 = (grid - (1.0 - fr)) / fr
            assert np.allclose(f2, (flux - (1.0 - fr)) / fr, rtol=1e-15) and np.allclose(e2, err / fr, rtol=1e-15)
            got = _numerics.robust_halfchi2(f2 - g2, 1.0 / (e2 * e2), *consts)
            assert (np.abs((got.astype(LD) - want).astype(np.float64)) <= bar).all(), (pair, off, fr)


# ---------------------------------------------------------------------------------------
# the ABI
def _declared():
    text = open(os.path.join(ROOT, "include", "trx_robust.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(trxr_[a-z0-9_]+)\s*\(", text)))


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(ln.split()[-1] for ln in out.splitlines() if " T " in ln)


def test_header_libraries_and_binding_list_the_same_symbol():
    import ctypes
    assert _declared() == sorted(_lib.ROBUST_SYMBOLS) == ["trxr_chi2_grid_robust"]
    assert not set(_lib.ROBUST_SYMBOLS) & (set(_lib.ABI_SYMBOLS) | set(_lib.WARP_SYMBOLS) | set(_lib.NOISE_SYMBOLS)
                                           | set(_lib.MIX_SYMBOLS) | set(_lib.SHIFT_SYMBOLS) | set(_lib.DEBUG_SYMBOLS))
    assert callable(_lib.chi2_grid_robust)
    others = sorted(f for f in os.listdir(os.path.join(ROOT, "include")) if f != "trx_robust.h")
    assert {"trx.h", "trx_warp.h", "trx_noise.h", "trx_mix.h", "trx_shift.h", "trx_debug.h"} <= set(others)
    for other in others:
        assert "trxr_" not in open(os.path.join(ROOT, "include", other)).read().lower()
    import __graft_entry__ as g
    g.build()
    for path in (_lib.LIB_PATH, _lib.TESTING_LIB_PATH):
        assert [s for s in _exports(path) if s.startswith("trxr_")] == _declared()
    for name in ("trx_robust.hpp", "trx_robust.h"):
        assert any(os.path.basename(d) == name for d in g.DEPS), name
    vp, dbl = ctypes.c_void_p, ctypes.c_double
    for L in (_lib.lib(), _lib.testing_lib()):
        fn = L.trxr_chi2_grid_robust
        assert fn.restype is ctypes.c_int
        assert list(fn.argtypes) == [vp, vp, vp, ctypes.c_int, ctypes.c_long, vp, dbl, ctypes.c_int, vp, dbl, dbl, dbl, vp]


def test_argument_checks_need_no_gpu():
    """every refusal comes before anything touches a device: the pointers below are not device memory"""
    import __graft_entry__ as g
    g.build()
    L = _lib.lib()
    v = [np.zeros(64) for _ in range(4)]
    f, w, m, o = (x.ctypes.data for x in v)
    call = L.trxr_chi2_grid_robust
    ERR_ARG = 1
    c0, c1, k2 = D.robust_constants(0.05, 10.0)
    for n in (4, 0):                                                            # (... also with no rows)
        assert call(None, w, m, 8, n, None, INF, 0, o, c0, c1, k2, None) == ERR_ARG
        assert call(f, None, m, 8, n, None, INF, 0, o, c0, c1, k2, None) == ERR_ARG
        assert call(f, w, None, 8, n, None, INF, 0, o, c0, c1, k2, None) == ERR_ARG
        assert call(f, w, m, 8, n, None, INF, 0, None, c0, c1, k2, None) == ERR_ARG
        assert b"null pointer" in L.trx_last_error()
        for n_time in (0, -1):
            assert call(f, w, m, n_time, n, None, INF, 0, o, c0, c1, k2, None) == ERR_ARG
        assert b"n_time" in L.trx_last_error()
        for bad in (NAN, INF, -INF, -1e-300, -1.0):
            assert call(f, w, m, 8, n, None, INF, 0, o, bad, c1, k2, None) == ERR_ARG
        assert b"c0" in L.trx_last_error()
        for bad in (NAN, INF, -INF):
            assert call(f, w, m, 8, n, None, INF, 1, o, c0, bad, k2, None) == ERR_ARG
        assert b"c1" in L.trx_last_error()
        for bad in (NAN, INF, -INF, 0.0, -0.25, 1.0, 1.5):
            assert call(f, w, m, 8, n, None, INF, 0, o, c0, c1, bad, None) == ERR_ARG
        assert b"k2" in L.trx_last_error()
    assert call(f, w, m, 8, -1, None, INF, 0, o, c0, c1, k2, None) == ERR_ARG         # n < 0
    # n == 0: nothing to launch -- c0 = 0 and a negative c1 are allowed
    for accumulate in (0, 1):
        assert call(f, w, m, 8, 0, None, INF, accumulate, o, c0, c1, k2, None) == 0
        assert call(f, w, m, 1, 0, m, 1.0, accumulate, o, 0.0, -3.0, 0.5, None) == 0
    assert not any(x.any() for x in v)
