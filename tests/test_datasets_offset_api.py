"""Per-dataset baseline offsets on the host: the `offset_sigma` key of a dataset, its
renormalisation, the float64 restatement _numerics.offset_halfchi2 against a direct numerical integral over the offset,
and the ABI entry of the reduction.  No GPU: every check here ends before the first device call.

Tolerances: 1e-15 relative for s^2 sum(w) under renormalisation (two roundings each side); 1e-10 absolute for the
closed form against scipy's quadrature (quad's own error estimate is asserted below 1e-11 of the integral)."""
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


def _ds(**extra):
    d = {"time": np.linspace(-0.1, 0.1, 7), "flux": np.full(7, 0.999), "flux_err": np.linspace(1e-3, 2e-3, 7)}
    d.update(extra)
    return d


@pytest.mark.parametrize("value", [0.5, 3, np.float64(2e-3), INF, None])
def test_validate_accepts_offset_sigma(value):
    got = D.validate([_ds(), _ds(offset_sigma=value)])
    assert got[0].offset_sigma is None                                   # absent: no offset, as before
    if value is None:
        assert got[1].offset_sigma is None
    else:
        assert isinstance(got[1].offset_sigma, float) and got[1].offset_sigma == float(value)
    assert D.Datasets(got).has_offsets == (value is not None)


@pytest.mark.parametrize("value", [0, 0.0, -1, -INF, float("nan"), "x", "1.0", True, [1.0]])
def test_validate_rejects_offset_sigma(value):
    with pytest.raises(ValueError, match="dataset 1.*offset_sigma"):
        D.validate([_ds(), _ds(offset_sigma=value)])


@pytest.mark.parametrize("fr", [1.0, 0.37, 1.0 / 3.0, 0.0123])
def test_renorm_scales_offset_sigma_with_the_errors(fr):
    sets = D.Datasets(D.validate([_ds(offset_sigma=2.5e-3), _ds(offset_sigma=INF), _ds()]))
    star = sets.renorm(fr)
    assert star.sets[0].offset_sigma == 2.5e-3 / fr
    assert star.sets[1].offset_sigma == INF and star.sets[2].offset_sigma is None
    # s^2 sum(w): the factor the evidence drops is the same for every star
    before = sets.sets[0].offset_sigma ** 2 * math.fsum(1.0 / sets.sets[0].flux_err ** 2)
    after = star.sets[0].offset_sigma ** 2 * math.fsum(1.0 / star.sets[0].flux_err ** 2)
    assert abs(after - before) <= 1e-15 * before
    assert np.array_equal(star.sets[0].flux_err, sets.sets[0].flux_err / fr)


def test_prepare_dataset_passes_the_key_through():
    t = np.linspace(-0.4, 0.4, 400)
    y = 1.0 + 1e-3 * np.sin(37.0 * t)
    assert lc.prepare_dataset(t, y, n_bins=20, n_sigma=10)["offset_sigma"] is None
    d = lc.prepare_dataset(t, y, n_bins=20, n_sigma=10, offset_sigma=INF)
    assert d["offset_sigma"] == INF
    assert D.validate([d])[0].offset_sigma == INF


def _neg_log_marginal(r, w, s):
    """-ln int exp(-0.5 sum w (r - c)^2) N(c; 0, s^2) dc by quadrature, in log space around the maximum"""
    from scipy.integrate import quad

    def f(c):
        return 0.5 * np.sum(w * (r - c) ** 2) + 0.5 * c * c / (s * s) + 0.5 * math.log(2 * math.pi * s * s)

    prec = np.sum(w) + 1.0 / (s * s)
    c_hat = np.sum(w * r) / prec
    f0 = f(c_hat)
    half = 12.0 / math.sqrt(prec)             # (exp(-72) of the peak at the ends)
    val, err = quad(lambda c: math.exp(-(f(c) - f0)), c_hat - half, c_hat + half, epsabs=0.0, epsrel=1e-13,
                    points=[c_hat], limit=200)
    assert err < 1e-11 * val
    return f0 - math.log(val)


@pytest.mark.parametrize("scale", [0.1, 1.0, 100.0])
@pytest.mark.parametrize("T", [1, 5, 50])
def test_offset_halfchi2_is_the_marginal_over_the_offset(T, scale):
    rng = np.random.default_rng(1000 * T + int(10 * scale))
    sigma = 1e-3
    err = sigma * rng.uniform(0.6, 1.8, T)
    w = 1.0 / err ** 2
    r = rng.normal(0.0, sigma, T) + 2.0 * sigma          # residuals carrying an offset of 2 sigma
    s = scale * sigma
    h = float(_numerics.offset_halfchi2(r, w, s))
    want = _neg_log_marginal(r, w, s)
    got = h + 0.5 * math.log1p(s * s * math.fsum(w))
    print("T %d s %g sigma: h %.6g, -ln integral %.12g, difference %.3g" % (T, scale, h, want, got - want))
    assert abs(got - want) <= 1e-10
    assert 0.0 <= h <= 0.5 * np.sum(w * r * r)


def test_offset_halfchi2_limits():
    rng = np.random.default_rng(7)
    w = rng.uniform(1.0, 10.0, 50) * 1e6
    r = rng.normal(3e-3, 1e-3, (4, 50))
    S0, S1, S2 = math.fsum(w), np.sum(w * r, axis=1), np.sum(w * r * r, axis=1)
    flat = _numerics.offset_halfchi2(r, w, INF)
    assert flat.shape == (4,) and np.array_equal(flat, 0.5 * (S2 - S1 * S1 / S0))
    assert np.array_equal(_numerics.offset_halfchi2(r, w, None), 0.5 * S2)
    # s -> 0: today's chi^2/2, continuously (the difference is at most 0.5 s^2 S1^2)
    tiny = _numerics.offset_halfchi2(r, w, 1e-12)
    assert np.all(np.abs(tiny - 0.5 * S2) <= 0.5 * 1e-24 * S1 * S1 + 1e-15 * S2)
    # one point and a flat prior: the offset absorbs the residual
    assert _numerics.offset_halfchi2([0.3], [4.0], INF) == 0.0
    assert _numerics.offset_halfchi2(np.array([[0.3], [-1.7]]), [4.0], INF).tolist() == [0.0, 0.0]
    # a shift of the residuals does not move the flat-prior value
    moved = _numerics.offset_halfchi2(r + 0.01, w, INF)
    assert np.all(np.abs(moved - flat) <= 1e-12 * 0.5 * np.sum(w * (r + 0.01) ** 2, axis=1))


def test_abi_declares_the_offset_reduction():
    assert "trx_chi2_grid_offset" in _lib.ABI_SYMBOLS
    header = open(os.path.join(ROOT, "include", "trx.h")).read()
    m = re.search(r"\bint\s+trx_chi2_grid_offset\s*\(([^)]*)\)", header)
    assert m is not None
    args = m.group(1)
    assert re.search(r"double\s+sum_w\s*,\s*double\s+prior_prec\s*,\s*double\s*\*\s*offset_out", args)
    assert callable(_lib.chi2_grid_offset)
