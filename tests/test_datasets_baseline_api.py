"""Per-dataset linear baseline models on the host: the `baseline` / `baseline_sigma` keys of a dataset,
their renormalisation, datasets.baseline_system, the float64 statement _numerics.baseline_halfchi2 against least squares
and against a direct numerical integral over the coefficients, lightcurve.polynomial_baseline and the ABI entry of the
reduction.  No GPU: every check here ends before the first device call.

Tolerances, none of them chosen from results:
  renormalisation: a finite sigma is sigma / fr exactly; the scaled system matrix moves by <= 1e-14 (only roundings differ);
  flat priors against np.linalg.lstsq on the sqrt(w)-scaled system: 1e-10 x 0.5 S2, on columns whose scaled system has
        lambda_min >= 0.01 (asserted);
  one column of ones against offset_halfchi2: 1e-12 x 0.5 S2;
  K = 2, finite priors against nested quadrature: ten times the quadrature's own error estimate, which is asserted below
        1e-11 of the integral for the outer and for every inner integral (so 2e-10 in the logarithm);
  the rounding bar of a flat-prior value: 1e-12 x 0.5 S2 x (1 + 4 sqrt(K / lambda_min)) + 1e-12 (tests/test_gpu_chi2_baseline.py)."""
import math
import os
import re

import numpy as np
import pytest

from triceratops_amd import _lib, _numerics
from triceratops_amd import datasets as D
from triceratops_amd import lightcurve as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
NAN = float("nan")
T7 = np.linspace(-0.1, 0.1, 7)
U7 = np.linspace(-1.0, 1.0, 7)


def _ds(**extra):
    d = {"time": T7.copy(), "flux": np.full(7, 0.999), "flux_err": np.linspace(1e-3, 2e-3, 7)}
    d.update(extra)
    return d


def _bar(S2, K, lam):
    return 1e-12 * 0.5 * S2 * (1.0 + 4.0 * math.sqrt(K / lam)) + 1e-12


# ---- 1. validation accepts ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("baseline, sigma, k", [
    (U7, "absent", 1), (U7.tolist(), 2e-3, 1), ([U7, U7 ** 2], "absent", 2), (np.stack([U7, U7 ** 2]), [1e-3, INF], 2),
    (np.stack([U7, U7 ** 2, U7 ** 3]), INF, 3), (np.stack([U7, U7 ** 2]), np.array([0.5, 3.0]), 2), (U7, None, 1),
])
def test_validate_accepts_baseline(baseline, sigma, k):
    extra = {"baseline": baseline}
    if not isinstance(sigma, str):
        extra["baseline_sigma"] = sigma
    got = D.validate([_ds(), _ds(**extra)])
    assert got[0].baseline is None and got[0].baseline_sigma is None
    b, s = got[1].baseline, got[1].baseline_sigma
    assert b.shape == (k, 7) and b.dtype == np.float64 and s.shape == (k,)
    assert np.array_equal(b, np.atleast_2d(np.asarray(baseline, dtype=np.float64)))
    want = np.full(k, INF) if (isinstance(sigma, str) or sigma is None) else np.broadcast_to(np.asarray(sigma, float), (k,))
    assert np.array_equal(s, want)
    sets = D.Datasets(got)
    assert sets.has_baselines and not sets.has_offsets
    assert D.baseline_system(got[0]) is None and len(D.baseline_system(got[1]).terms) == k


def test_validate_accepts_none_for_both_keys():
    got = D.validate([_ds(baseline=None, baseline_sigma=None), _ds(offset_sigma=INF, baseline=None)])
    assert all(g.baseline is None and g.baseline_sigma is None for g in got)
    assert not D.Datasets(got).has_baselines and D.Datasets(got).has_offsets
    assert D.Dataset(T7, T7, T7, 0.1, 1).baseline is None and D.Dataset(T7, T7, T7, 0.1, 1).baseline_sigma is None
    assert D.MAX_BASELINE_TERMS == 4


def test_offset_is_term_zero_of_the_system():
    d = D.validate([_ds(offset_sigma=2e-3, baseline=[U7, U7 ** 2], baseline_sigma=[INF, 1e-3])])[0]
    system = D.baseline_system(d)
    assert [t[0] for t in system.terms] == ["offset", "baseline", "baseline"]
    assert [t[2] for t in system.terms] == [2e-3, INF, 1e-3]
    w = 1.0 / d.flux_err ** 2
    B = np.stack([np.ones(7), U7, U7 ** 2])
    assert np.allclose(system.D, (w * B * B).sum(axis=1), rtol=1e-15)
    assert np.allclose(system.g, w * B / np.sqrt(system.D)[:, None], rtol=1e-15)
    A = (B * w) @ B.T + np.diag([1.0 / 2e-3 ** 2, 0.0, 1.0 / 1e-3 ** 2])
    A = A / np.sqrt(np.outer(system.D, system.D))
    assert np.abs(system.A - A).max() <= 1e-14 and np.abs(system.M @ system.A - np.eye(3)).max() <= 1e-12
    assert system.minv.shape == (6,) and np.array_equal(system.minv, system.M[np.triu_indices(3)])
    assert system.lambda_min >= 1e-6
    # an offset alone has a system too (one column of ones); no term, no system
    one = D.baseline_system(D.validate([_ds(offset_sigma=INF)])[0])
    assert one.terms == (("offset", None, INF),) and np.array_equal(one.A, [[1.0]]) and np.array_equal(one.M, [[1.0]])


# ---- 2. validation rejects ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extra", [
    {"baseline": U7[:6]},                                                     # a wrong length
    {"baseline": np.stack([U7, U7])[:, :5]},
    {"baseline": np.zeros((2, 2, 7))},
    {"baseline": np.where(np.arange(7) == 3, NAN, U7)},                       # NaN / inf in a kept entry
    {"baseline": np.where(np.arange(7) == 0, INF, U7)},
    {"baseline": U7, "baseline_sigma": 0.0},                                  # baseline_sigma <= 0, NaN, wrong length
    {"baseline": U7, "baseline_sigma": -1.0},
    {"baseline": U7, "baseline_sigma": NAN},
    {"baseline": U7, "baseline_sigma": [1.0, 2.0]},
    {"baseline": [U7, U7 ** 2], "baseline_sigma": [1.0, -2.0]},
    {"baseline": U7, "baseline_sigma": "x"},
    {"baseline_sigma": 1.0},                                                  # ... or without baseline
    {"baseline": None, "baseline_sigma": INF},
    {"baseline": [U7, U7 ** 2, U7 ** 3, U7 ** 4, U7 ** 5]},                   # more than 4 terms in total
    {"baseline": [U7, U7 ** 2, U7 ** 3, U7 ** 4], "offset_sigma": 1e-3},
    {"baseline": np.zeros(7)},                                                # an all-zero column
    {"baseline": [U7, np.zeros(7)]},
    {"baseline": np.full(7, 2.5), "offset_sigma": INF},                       # a constant column next to a flat offset
    {"baseline": [U7, 3.0 * U7]},                                             # two proportional columns
])
def test_validate_rejects_baseline(extra):
    with pytest.raises(ValueError, match="dataset 1.*baseline"):
        D.validate([_ds(), _ds(**extra)])


def test_validate_rejects_three_flat_terms_on_two_points():
    two = {"time": [0.0, 0.1], "flux": [1.0, 1.0], "flux_err": 1e-3}
    u = np.array([-1.0, 1.0])
    with pytest.raises(ValueError, match="dataset 1.*baseline"):
        D.validate([_ds(), dict(two, offset_sigma=INF, baseline=[u, u ** 2 + 0.5 * u])])
    # ... and finite priors make the same columns a proper system
    got = D.validate([dict(two, offset_sigma=1e-3, baseline=[u, u ** 2 + 0.5 * u], baseline_sigma=1e-3)])
    assert D.baseline_system(got[0]).lambda_min >= 1e-6


# ---- 3. NaN drops ---------------------------------------------------------------------------------------------------
def test_a_dropped_point_drops_its_baseline_entries():
    flux = np.full(7, 0.999)
    flux[2] = NAN
    time = T7.copy()
    time[5] = NAN
    cols = np.stack([U7, U7 ** 2])
    cols[:, 2] = NAN                      # (an entry of a dropped point may be anything)
    cols[1, 5] = INF
    got = D.validate([_ds(time=time, flux=flux, baseline=cols)])[0]
    keep = np.array([0, 1, 3, 4, 6])
    assert got.time.size == 5 and np.array_equal(got.baseline, np.stack([U7, U7 ** 2])[:, keep])


# ---- 4. renorm ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fr", [1.0, 0.37, 1.0 / 3.0, 0.0123])
def test_renorm_scales_finite_sigmas_and_leaves_the_scaled_system(fr):
    sets = D.Datasets(D.validate([_ds(offset_sigma=2.5e-3, baseline=[U7, U7 ** 2], baseline_sigma=[1.5e-3, INF]),
                                  _ds(baseline=U7, baseline_sigma=4e-3), _ds()]))
    star = sets.renorm(fr)
    assert np.array_equal(star.sets[0].baseline_sigma, [1.5e-3 / fr, INF]) and star.sets[0].offset_sigma == 2.5e-3 / fr
    assert np.array_equal(star.sets[1].baseline_sigma, [4e-3 / fr]) and star.sets[2].baseline_sigma is None
    assert np.array_equal(star.sets[0].baseline, sets.sets[0].baseline)          # the columns are left alone
    for a, b in zip(sets.sets[:2], star.sets[:2]):
        A0, A1 = D.baseline_system(a).A, D.baseline_system(b).A
        print("fr %g: max |d A~| %.3g" % (fr, np.abs(A1 - A0).max()))
        assert np.abs(A1 - A0).max() <= 1e-14
        assert abs(D.baseline_system(a).lambda_min - D.baseline_system(b).lambda_min) <= 1e-13


# ---- 5. flat priors: least squares -----------------------------------------------------------------------------------
def _poly_case(K, T, seed=0):
    rng = np.random.default_rng(1000 * K + T + seed)
    u = np.linspace(-1.0, 1.0, T) if T > 1 else np.zeros(1)
    B = np.stack([u ** p for p in range(K)])
    sigma = 1e-3
    w = 1.0 / (sigma * rng.uniform(0.6, 1.8, T)) ** 2
    r = rng.normal(0.0, sigma, (3, T)) + sigma * (2.0 + 1.5 * u)             # residuals carrying a trend
    return u, B, w, r


@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_flat_priors_are_weighted_least_squares(K):
    for T in sorted({K, K + 1, 5, 50}):
        if T < K:
            continue
        u, B, w, r = _poly_case(K, T)
        lam = D.linear_system(w, B, INF).lambda_min
        assert lam >= 0.01, (K, T, lam)
        h = _numerics.baseline_halfchi2(r, w, B)
        assert h.shape == (3,) and (h >= 0.0).all()
        sw = np.sqrt(w)
        for i in range(3):
            c = np.linalg.lstsq((B * sw).T, r[i] * sw, rcond=None)[0]
            want = 0.5 * np.sum(w * (r[i] - c @ B) ** 2)
            S2 = np.sum(w * r[i] ** 2)
            print("K %d T %d: h %.6g least squares %.6g, difference / (0.5 S2) %.3g" % (K, T, h[i], want, (h[i] - want) / (0.5 * S2)))
            assert abs(h[i] - want) <= 1e-10 * 0.5 * S2
        assert np.array_equal(_numerics.baseline_halfchi2(r, w, B, INF), h)
        assert np.array_equal(_numerics.baseline_halfchi2(r, w, B, [INF] * K), h)
        one = _numerics.baseline_halfchi2(r[1], w, B)                                       # [T] in, a scalar out
        assert np.ndim(one) == 0 and abs(one - h[1]) <= 1e-12 * 0.5 * np.sum(w * r[1] ** 2)
    assert np.array_equal(_numerics.baseline_halfchi2(r, w, None), 0.5 * np.sum(w * r * r, axis=-1))


# ---- 6. one column of ones: offset_halfchi2 -------------------------------------------------------------------------
@pytest.mark.parametrize("s", [1e-4, 1e-3, 0.1, INF])
@pytest.mark.parametrize("T", [1, 5, 50])
def test_a_column_of_ones_is_the_offset(T, s):
    _, _, w, r = _poly_case(1, T, seed=7)
    got = _numerics.baseline_halfchi2(r, w, np.ones(T), s)
    want = _numerics.offset_halfchi2(r, w, s)
    S2 = np.sum(w * r * r, axis=-1)
    assert (np.abs(got - want) <= 1e-12 * 0.5 * S2).all()


# ---- 7. K = 2, finite priors: the integral ----------------------------------------------------------------------------
def _neg_log_marginal2(r, w, B, s):
    """-ln int int exp(-0.5 sum w (r - c1 B1 - c2 B2)^2) N(c1; 0, s1^2) N(c2; 0, s2^2) dc2 dc1 by nested quadrature, in log
    space around the maximum; returns (value, relative error estimate of the integral)"""
    from scipy.integrate import quad

    def f(c1, c2):
        d = r - c1 * B[0] - c2 * B[1]
        return (0.5 * np.sum(w * d * d) + 0.5 * c1 * c1 / s[0] ** 2 + 0.5 * c2 * c2 / s[1] ** 2
                + 0.5 * math.log(2 * math.pi * s[0] ** 2) + 0.5 * math.log(2 * math.pi * s[1] ** 2))

    A = (B * w) @ B.T + np.diag(1.0 / np.asarray(s) ** 2)
    b = (B * w) @ r
    c_hat = np.linalg.solve(A, b)
    f0 = f(*c_hat)
    inner_rel = [0.0]

    def inner(c1):
        centre = (b[1] - A[0, 1] * c1) / A[1, 1]
        half = 12.0 / math.sqrt(A[1, 1])
        val, err = quad(lambda c2: math.exp(-(f(c1, c2) - f0)), centre - half, centre + half, epsabs=0.0, epsrel=1e-13,
                        points=[centre], limit=200)
        if val > 1e-30:                   # (the tails of the outer integral carry no weight)
            inner_rel[0] = max(inner_rel[0], err / val)
        return val

    half = 12.0 / math.sqrt(A[0, 0] - A[0, 1] ** 2 / A[1, 1])
    val, err = quad(inner, c_hat[0] - half, c_hat[0] + half, epsabs=0.0, epsrel=1e-13, points=[c_hat[0]], limit=200)
    assert err < 1e-11 * val and inner_rel[0] < 1e-11
    return f0 - math.log(val), err / val + inner_rel[0]


@pytest.mark.parametrize("scale", [(0.3, 0.3), (1.0, 3.0), (100.0, 0.5)])
@pytest.mark.parametrize("T", [2, 5, 50])
def test_baseline_halfchi2_is_the_marginal_over_two_coefficients(T, scale):
    u, _, w, r = _poly_case(2, T, seed=31)
    B = np.stack([np.ones(T), u])
    s = (scale[0] * 1e-3, scale[1] * 1e-3)
    h = float(_numerics.baseline_halfchi2(r[0], w, B, s))
    want, rel = _neg_log_marginal2(r[0], w, B, s)
    G = (B * w) @ B.T
    logdet = np.linalg.slogdet(np.eye(2) + np.diag(np.asarray(s) ** 2) @ G)[1]
    got = h + 0.5 * logdet
    print("T %d s %s sigma: h %.6g, -ln integral %.12g, difference %.3g, quadrature estimate %.3g"
          % (T, scale, h, want, got - want, rel))
    assert rel <= 2e-11
    assert abs(got - want) <= 10.0 * 2e-11
    assert 0.0 <= h <= 0.5 * np.sum(w * r[0] ** 2)


# ---- 8. limits --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_baseline_halfchi2_limits(K):
    u, B, w, r = _poly_case(K, 50, seed=3)
    S2 = np.sum(w * r * r, axis=-1)
    b = r @ (w * B).T                                                      # [3][K]
    # s -> 0: today's chi^2/2, continuously: b^T A^-1 b <= s^2 |b|^2 since A >= diag(1 / s^2)
    tiny = _numerics.baseline_halfchi2(r, w, B, 1e-12)
    assert (np.abs(tiny - 0.5 * S2) <= 0.5 * 1e-24 * np.sum(b * b, axis=-1) + 1e-15 * S2).all()
    # as many flat terms as points: the baseline absorbs the residuals
    uK, BK, wK, rK = _poly_case(K, K, seed=3)
    lam = D.linear_system(wK, BK, INF).lambda_min
    hK = _numerics.baseline_halfchi2(rK, wK, BK)
    assert (hK <= _bar(np.sum(wK * rK * rK, axis=-1), K, lam)).all() and (hK >= 0.0).all()
    # adding B c0 to the residuals does not move the flat-prior value
    lam = D.linear_system(w, B, INF).lambda_min
    flat = _numerics.baseline_halfchi2(r, w, B)
    c0 = 1e-3 * np.array([30.0, -7.0, 11.0, 5.0])[:K]
    moved = _numerics.baseline_halfchi2(r + c0 @ B, w, B)
    bar = _bar(np.sum(w * (r + c0 @ B) ** 2, axis=-1), K, lam)
    print("K %d: flat-prior value under r + B c0: max |d h| / bar %.3g" % (K, (np.abs(moved - flat) / bar).max()))
    assert (np.abs(moved - flat) <= bar).all()
    with pytest.raises(ValueError):
        _numerics.baseline_halfchi2(r, w, np.zeros(50))


# ---- 9. polynomial_baseline -------------------------------------------------------------------------------------------
def test_polynomial_baseline_and_prepare_dataset():
    t = np.array([3.0, 1.0, NAN, 2.5, 5.0])
    cols = lc.polynomial_baseline(t, 3)
    assert cols.shape == (3, 5)
    u = cols[0]
    assert np.nanmin(u) == -1.0 and np.nanmax(u) == 1.0 and np.isnan(u[2]) and u[0] == 0.0
    fin = ~np.isnan(t)
    assert np.array_equal(cols[1][fin], u[fin] ** 2) and np.array_equal(cols[2][fin], u[fin] ** 3)
    assert lc.polynomial_baseline(t, 1).shape == (1, 5)
    for bad in ((t, 0), (np.array([1.0, 1.0]), 1), (np.array([NAN]), 1)):
        with pytest.raises(ValueError):
            lc.polynomial_baseline(*bad)
    tt = np.linspace(-0.4, 0.4, 400)
    y = 1.0 + 1e-3 * np.sin(37.0 * tt)
    d0 = lc.prepare_dataset(tt, y, n_bins=20, n_sigma=10)
    assert d0["baseline"] is None and d0["baseline_sigma"] is None
    assert D.validate([d0])[0].baseline is None
    d2 = lc.prepare_dataset(tt, y, n_bins=20, n_sigma=10, offset_sigma=INF, baseline_order=2, baseline_sigma=[2e-3, INF])
    assert d2["baseline"].shape == (2, d2["time"].size)
    assert np.array_equal(d2["baseline"], lc.polynomial_baseline(d2["time"], 2))
    v = D.validate([d2])[0]
    assert v.baseline.shape == (2, v.time.size) and np.array_equal(v.baseline_sigma, [2e-3, INF])
    assert len(D.baseline_system(v).terms) == 3


# ---- 10. ABI ----------------------------------------------------------------------------------------------------------
def test_abi_declares_the_baseline_reduction():
    assert "trx_chi2_grid_baseline" in _lib.ABI_SYMBOLS and len(_lib.ABI_SYMBOLS) == 29
    header = open(os.path.join(ROOT, "include", "trx.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"\bint\s+trx_chi2_grid_baseline\s*\(([^)]*)\)", header)
    assert m is not None
    args = m.group(1)
    assert re.search(r"const\s+double\s*\*\s*wbasis\s*,\s*int\s+n_terms\s*,\s*const\s+double\s*\*\s*minv\s*,\s*"
                     r"double\s*\*\s*coef_out\s*,\s*void\s*\*\s*stream", args)
    assert callable(_lib.chi2_grid_baseline)
    # the argument checks need no device: nothing is enqueued
    L = _lib.lib()
    assert L.trx_chi2_grid_baseline(None, None, None, 5, 1, None, INF, 0, None, None, 1, None, None, None) == 1
    assert b"null pointer" in L.trx_last_error()
