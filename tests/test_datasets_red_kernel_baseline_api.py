"""Baseline terms marginalised under Matern-3/2 or two-term noise, on the host: the
`red_kernel_baseline` / `red_kernel_baseline_sigma` keys of a dataset, how Datasets carries and renormalises them,
datasets.ss2_baseline_system + _numerics.ss2_baseline_halfchi2 against the dense statements, the limits of the model, and
the ABI entry of the reduction (trxk_chi2_grid_ss2_baseline, include/trx_ss.h).  No GPU: every check here ends before the
first device call.

Bars, none of them chosen from results:
  dense solves: |d h| <= 1e-9 x 0.5 sum y^2 / sigma^2 + 1e-12 while cond(K) <= 1e5 (asserted), the bar of
        tests/test_datasets_red_kernel_api.py -- against 0.5 [y^T K^-1 y - b^T A^-1 b] and, for finite priors, against
        0.5 y^T (K + B diag(s^2) B^T)^-1 y;
  ss2_gls_bar, the device bar of tests/test_gpu_chi2_ss2_baseline.py, also held between the float64 and the long-double
        statement here: ss2_bar of tests/test_gpu_chi2_ss2.py -- the recurrence's roundings through the predictor's l1
        gain Gamma -- times the projection factor 1 + 4 sqrt(K / lambda_min) of the baseline tests: |d b~_k| is bounded by
        the same innovation errors through Cauchy-Schwarz in the unit columns, and a perturbation d b~ moves the quadratic
        form by at most 2 sqrt(S2) |d b~| / sqrt(lambda_min);
  ss2_coef_bar: 1e-12 (1 + Gamma) sqrt(K sum omega (|y| + Gamma max|y|)^2) / lambda_min + 1e-15 per entry of M b~:
        coef_bar of tests/test_datasets_red_baseline_api.py with Gamma in place of 1 / (1 - max alpha);
  ou2 with tau_1 = tau_2 against ou_baseline_halfchi2 with red_sigma = hypot(s_1, s_2), both in long double: the sum of
        gls_bar and ss2_gls_bar (the two recurrences' tables agree to 1e-13 relative, tests/test_datasets_red_kernel_api.py);
  a flat-prior column combination added to y: ss2_gls_bar at the shifted level;
  renorm by a power of two rounds nothing: A~, M, A, g identical in bits, D and omega times fr^2 exactly.
Measured here (test_zz_report): the dense checks at most 4.9e-6 (projected form) and 1.2e-5 (K + B S B^T) of their bar,
float64 against long double 3.3e-4 of ss2_gls_bar and 1.6e-4 of ss2_coef_bar, lambda_min >= 0.013 (four columns on four
stamps).
"""
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

from test_datasets_red_baseline_api import gls_bar
from test_datasets_red_kernel_api import KERNELS, RATIOS, SCALES, SIZES, case, dense, keys, light_curve
from test_datasets_red_noise_api import SIGMA
from test_gpu_chi2_ss2 import PARAMS, gain, ss2_bar
from triceratops_amd import _lib, _numerics
from triceratops_amd import datasets as D
from triceratops_amd import lightcurve as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
LD = np.longdouble
KS = [1, 2, 3, 4]
PRIORS = ("flat", "plus_identity")
_worst = {"dense": 0.0, "dense_c": 0.0, "ld": 0.0, "coef": 0.0, "lambda_min": INF}


def _ds(**extra):
    d = {"time": np.linspace(-0.1, 0.1, 7), "flux": np.full(7, 0.999), "flux_err": np.linspace(1e-3, 2e-3, 7)}
    d.update(extra)
    return d


M32 = {"red_kernel": "matern32", "red_sigma": 2e-3, "red_timescale": 0.05}
OU2 = {"red_kernel": "ou2", "red_sigma": (2e-3, 1e-3), "red_timescale": (0.05, 0.5)}


def _m32(**extra):
    return _ds(**M32, **extra)


U = np.linspace(-1.0, 1.0, 7)
ONES = np.ones(7)


def unit_time(t):
    return (t - 0.5 * (t[0] + t[-1])) / (0.5 * (t[-1] - t[0])) if t.size > 1 else np.zeros(1)


def columns(d, k):
    """u^0 ... u^(k - 1) on a Dataset's stamps"""
    u = unit_time(d.time)
    return np.stack([u ** p for p in range(k)])


def system_of(d, B, prior):
    """the system of the columns under flat priors, or under the priors that add the identity to A~ (1 / (s_k^2 D_k) = 1)"""
    s = D.ss2_baseline_system(d, B, INF)
    if prior == "plus_identity":
        s = D.ss2_baseline_system(d, B, 1.0 / np.sqrt(s.D))
    return s


def ss2_gls_bar(y, system, gamma):
    """the bar of one row of trxk_chi2_grid_ss2_baseline against the long-double statement: ss2_bar times the projection
    factor 1 + 4 sqrt(K / lambda_min)"""
    k = system.c.shape[0]
    return (ss2_bar(y, gamma, system.omega) - 1e-12) * (1.0 + 4.0 * np.sqrt(k / system.lambda_min)) + 1e-12


def ss2_coef_bar(y, system, gamma):
    """the bar of one entry of coef_out (the scaled coefficients M b~) against the long-double statement"""
    y = np.abs(np.asarray(y, dtype=np.float64))
    top = y.max(axis=-1, keepdims=True)
    k = system.c.shape[0]
    e = np.sum(system.omega * (y + gamma * top) ** 2, axis=-1)
    return 1e-12 * (1.0 + gamma) * np.sqrt(k * e) / system.lambda_min + 1e-15


# ---------------------------------------------------------------------------------------
# validation
@pytest.mark.parametrize("base", [M32, OU2], ids=KERNELS)
@pytest.mark.parametrize("sigma", [None, 1e-2, INF, [1e-2, INF], np.array([3.0, 1e-9]), np.float32(0.5)])
def test_validate_accepts_the_keys(sigma, base):
    B = np.stack([ONES, U])
    dicts = [_ds(), _ds(red_kernel_baseline=B, red_kernel_baseline_sigma=sigma, **base),
             _ds(red_kernel_baseline=U, **base)]
    sets = D.validate(dicts)
    assert D.Dataset._fields == ("time", "flux", "flux_err", "exptime", "nsamples", "offset_sigma", "baseline",
                                 "baseline_sigma", "red_grid", "red_sigma", "red_timescale")
    assert sets[1].red_kernel == base["red_kernel"] and sets[1].baseline is None
    pairs = D.red_kernel_baselines(dicts, sets)
    assert pairs[0] is None
    cols, s = pairs[1]
    assert cols.shape == (2, 7) and cols.dtype == np.float64 and cols.flags.c_contiguous and np.array_equal(cols, B)
    want = np.full(2, INF) if sigma is None else np.broadcast_to(np.asarray(sigma, dtype=np.float64), (2,))
    assert s.shape == (2,) and s.dtype == np.float64 and np.array_equal(s, want)
    assert pairs[2][0].shape == (1, 7) and np.array_equal(pairs[2][1], [INF])       # [len(time)]: one column, flat
    ds = D.Datasets(sets, red_kernel_baselines=pairs)
    assert ds.has_red_kernel_baselines and ds.has_red_noise and not ds.has_baselines and not ds.has_red_baselines
    plain = D.Datasets(sets)
    assert not plain.has_red_kernel_baselines and plain.red_kernel_baselines == (None, None, None)
    assert D.red_baselines(dicts, sets) == [None, None, None]
    with pytest.raises(ValueError, match="red_kernel_baselines: 2 pairs for 3 datasets"):
        D.Datasets(sets, red_kernel_baselines=pairs[:2])
    with pytest.raises(ValueError, match="red_kernel_baselines: 2 dicts for 3 datasets"):
        D.red_kernel_baselines(dicts[:2], sets)


def test_keys_of_none_are_no_keys():
    a = D.validate([_m32()])
    dicts = [_m32(red_kernel_baseline=None, red_kernel_baseline_sigma=None)]
    b = D.validate(dicts)
    assert D.red_kernel_baselines(dicts, b) == [None]
    for x, y in zip(a[0], b[0]):
        assert np.array_equal(x, y)


def test_nan_points_are_dropped_with_their_entries():
    flux = np.full(7, 0.999)
    flux[2] = np.nan
    time = np.linspace(-0.1, 0.1, 7)
    time[5] = np.nan
    B = np.stack([ONES, U])
    B[:, 2] = np.nan                     # entries of dropped points may be anything
    B[1, 5] = INF
    dicts = [_m32(time=time, flux=flux, red_kernel_baseline=B)]
    sets = D.validate(dicts)
    cols, _ = D.red_kernel_baselines(dicts, sets)[0]
    assert sets[0].time.size == 5 and np.array_equal(cols, np.stack([ONES, U])[:, [0, 1, 3, 4, 6]])
    bad = np.stack([ONES, U])
    bad[1, 3] = np.nan                   # ... those of a kept point may not
    with pytest.raises(ValueError, match="dataset 0.*red_kernel_baseline.*finite"):
        D.validate([_m32(time=time, flux=flux, red_kernel_baseline=bad)])


@pytest.mark.parametrize("base", [M32, OU2], ids=KERNELS)
@pytest.mark.parametrize("extra", [
    {"red_kernel_baseline": np.ones(6)}, {"red_kernel_baseline": np.ones((2, 6))}, {"red_kernel_baseline": np.ones((7, 2))},
    {"red_kernel_baseline": np.ones((1, 1, 7))}, {"red_kernel_baseline": np.ones((0, 7))}, {"red_kernel_baseline": 1.0},
    {"red_kernel_baseline": "ones"}, {"red_kernel_baseline": True}, {"red_kernel_baseline": [[1.0] * 7, [1.0] * 6]},
    {"red_kernel_baseline": np.where(np.arange(7) == 3, np.nan, U)},                                       # not finite
    {"red_kernel_baseline": np.where(np.arange(7) == 0, INF, U)},
    {"red_kernel_baseline": np.stack([U ** p for p in range(5)])},                                         # five columns
    {"red_kernel_baseline_sigma": 1e-2}, {"red_kernel_baseline_sigma": [1e-2, INF]},                       # no columns
    {"red_kernel_baseline": U, "red_kernel_baseline_sigma": 0.0}, {"red_kernel_baseline": U, "red_kernel_baseline_sigma": -1.0},
    {"red_kernel_baseline": U, "red_kernel_baseline_sigma": float("nan")},
    {"red_kernel_baseline": U, "red_kernel_baseline_sigma": "1"}, {"red_kernel_baseline": U, "red_kernel_baseline_sigma": True},
    {"red_kernel_baseline": U, "red_kernel_baseline_sigma": [1e-2, 1e-2]},
    {"red_kernel_baseline": np.stack([ONES, U]), "red_kernel_baseline_sigma": [1e-2, 0.0]},
    {"red_kernel_baseline": np.zeros(7)}, {"red_kernel_baseline": np.stack([U, np.zeros(7)])},             # a zero column
    {"red_kernel_baseline": np.stack([U, U])}, {"red_kernel_baseline": np.stack([ONES, U, ONES])},         # collinear
    {"red_kernel_baseline": np.stack([ONES, U, 2.0 * ONES - 3.0 * U])},
])
def test_validate_rejects(extra, base):
    with pytest.raises(ValueError, match="dataset 1.*red_kernel_baseline"):
        D.validate([_ds(), _ds(**base, **extra)])


@pytest.mark.parametrize("base", [M32, OU2], ids=KERNELS)
@pytest.mark.parametrize("extra", [
    {"offset_sigma": 1e-3}, {"offset_sigma": INF}, {"baseline": U ** 2}, {"baseline": U ** 2, "baseline_sigma": 1.0},
    {"red_baseline": ONES}, {"red_baseline": ONES, "red_baseline_sigma": 1e-3}, {"red_grid": [(1e-3, 0.1, 1.0)]},
    {"white_grid": [(1.0, 0.0, 1.0), (2.0, 0.0, 1.0)]}, {"outlier_frac": 0.05, "outlier_scale": 10.0},
], ids=["offset", "flat-offset", "baseline", "baseline_sigma", "red_baseline", "red_baseline_sigma", "red_grid", "white_grid",
        "outliers"])
def test_the_keys_stand_next_to_the_kernel_and_a_t0_grid_alone(extra, base):
    with pytest.raises(ValueError, match="dataset 1.*not built"):
        D.validate([_ds(), _ds(red_kernel_baseline=U, **base, **extra)])
    with pytest.raises(ValueError, match="dataset 0.*red_kernel_baseline.*not built"):
        D.red_kernel_baselines([_ds(red_kernel_baseline=U, **base, **extra)], D.validate([_ds(**base)]))
    dicts = [_ds(red_kernel_baseline=np.stack([ONES, U]), t0_grid=[(-0.001, 1.0), (0.0, 2.0), (0.001, 1.0)], **base)]
    sets = D.validate(dicts)
    ds = D.Datasets(sets, D.t0_grids(dicts, sets), red_kernel_baselines=D.red_kernel_baselines(dicts, sets))
    assert ds.has_t0_grids and ds.has_red_kernel_baselines and not ds.has_outliers and ds.t0_grids[0].shape == (3, 2)


def test_red_baseline_next_to_the_kernels_names_the_new_keys():
    for base in (M32, OU2):
        with pytest.raises(ValueError, match="dataset 0.*red_kernel.*not built.*red_kernel_baseline / red_kernel_baseline_sigma"):
            D.validate([_ds(red_baseline=ONES, **base)])


@pytest.mark.parametrize("extra", [{}, {"red_sigma": 1e-3, "red_timescale": 0.1},
                                   {"red_sigma": 1e-3, "red_timescale": 0.1, "red_kernel": "ou"}, {"t0_grid": [(0.0, 1.0)]}],
                         ids=["white", "ou", "ou-named", "t0_grid"])
def test_the_keys_need_one_of_the_two_kernels(extra):
    with pytest.raises(ValueError, match="dataset 1.*red_kernel_baseline needs red_kernel"):
        D.validate([_ds(), _ds(red_kernel_baseline=np.stack([ONES, U]), red_kernel_baseline_sigma=1e-2, **extra)])


def test_collinear_message_is_the_baselines_style():
    with pytest.raises(ValueError, match=r"dataset 0: the red_kernel_baseline terms are collinear .*smallest eigenvalue of "
                                         r"the scaled system .* < 1e-06"):
        D.validate([_m32(red_kernel_baseline=np.stack([ONES, ONES]))])
    with pytest.raises(ValueError, match="dataset 0: red_kernel_baseline term column 1 is zero at every point"):
        D.validate([_m32(red_kernel_baseline=np.stack([ONES, np.zeros(7)]))])
    with pytest.raises(ValueError, match="dataset 0: at most 4 red_kernel_baseline columns"):
        D.validate([_m32(red_kernel_baseline=np.stack([U ** p for p in range(5)]))])
    # finite priors lift the degeneracy, as they do for `baseline`
    dicts = [_m32(red_kernel_baseline=np.stack([ONES, ONES]), red_kernel_baseline_sigma=1e-3)]
    assert D.red_kernel_baselines(dicts, D.validate(dicts))[0][0].shape == (2, 7)


def test_prepare_dataset_passes_the_keys_through():
    import inspect
    names = list(inspect.signature(lc.prepare_dataset).parameters)
    assert "red_kernel_baseline_order" in names and "red_kernel_baseline_sigma" in names
    t = np.linspace(-0.4, 0.4, 400)
    y = 1.0 + 1e-3 * np.sin(37.0 * t)
    noise = dict(red_sigma=2e-4, red_timescale=0.05, red_kernel="matern32")
    plain = lc.prepare_dataset(t, y, n_bins=20, n_sigma=10, **noise)
    assert "red_kernel_baseline" not in plain and "red_kernel_baseline_sigma" not in plain
    d = lc.prepare_dataset(t, y, n_bins=20, n_sigma=10, red_kernel_baseline_order=1, red_kernel_baseline_sigma=[INF, 1e-2],
                           **noise)
    assert np.array_equal(d["red_kernel_baseline"], lc.trend_columns(d["time"], 1)) and d["red_kernel_baseline"].shape[0] == 2
    assert d["red_kernel_baseline_sigma"] == [INF, 1e-2] and "red_baseline" not in d
    sets = D.validate([d])
    cols, s = D.red_kernel_baselines([d], sets)[0]
    assert np.array_equal(cols[0], np.ones(sets[0].time.size)) and np.array_equal(s, [INF, 1e-2])
    with pytest.raises(ValueError, match="dataset 0.*red_kernel_baseline needs red_kernel"):
        D.validate([lc.prepare_dataset(t, y, n_bins=20, n_sigma=10, red_kernel_baseline_order=1)])


def test_fused_evaluation_is_refused_before_any_device_call(monkeypatch):
    """target._datasets_pass refuses evaluation='fused' once the work units are prepared and before they run; the
    preparation (priors, TRILEGAL) is not what is under test and is stubbed"""
    from test_datasets_api import _target
    from triceratops_amd.triceratops import target
    tg = _target()
    monkeypatch.setattr(target, "_prepare", lambda self, *a, **k: ([], 0))
    for base in (M32, OU2):
        dicts = [_ds(), _ds(red_kernel_baseline=np.stack([ONES, U]), **base)]
        sets = D.validate(dicts)
        ds = D.Datasets(sets, red_kernel_baselines=D.red_kernel_baselines(dicts, sets))
        with pytest.raises(NotImplementedError, match="evaluation='fused' with a red_kernel_baseline"):
            tg._datasets_pass(ds, 3.0, {}, 0, "fused")


def test_the_switch_and_the_record():
    from triceratops_amd import fused
    assert fused.DATASET_RED_KERNEL_BASELINES is None and "DATASET_RED_KERNEL_BASELINES" in fused.switches.__doc__
    box = {}
    with fused.switches(DATASET_RED_KERNEL_BASELINES=box):
        assert fused.DATASET_RED_KERNEL_BASELINES is box
    assert fused.DATASET_RED_KERNEL_BASELINES is None
    assert fused._Ss2Lin._fields == ("tables", "c", "minv", "sqrt_d") and fused._Ss2._fields == ("A", "g", "omega")
    assert fused._Dataset._fields == ("time", "flux", "inv_var", "exptime", "nsamples", "term", "shift")
    assert fused._Dataset(None, None, None, 0.0, 1).term is None and fused._Dataset(None, None, None, 0.0, 1).shift is None
    alone = fused._Dataset(None, None, None, 0.0, 1, term=fused._Ss2(1, 2, 3))             # the kernel's tables alone
    rec = fused._Ss2Lin((1, 2, 3), None, None, None)
    cols = fused._Dataset(None, None, None, 0.0, 1, term=rec)
    assert cols.term is rec and type(alone.term) is fused._Ss2 and type(cols.term) is fused._Ss2Lin
    assert not isinstance(alone.term, fused._Ss2Lin) and not isinstance(cols.term, fused._Ss2)


# ---------------------------------------------------------------------------------------
# Datasets: carried and renormalised
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("fr", [1.0, 0.5, 0.37])
@pytest.mark.parametrize("flat", [True, False], ids=["flat", "finite"])
def test_renorm_scales_the_finite_sigmas_and_leaves_the_system_alone(fr, flat, kernel):
    d, _ = case(50, kernel, 3.0, 5.0)
    B = columns(d, 3)
    s = np.array([INF, INF, INF]) if flat else np.array([30.0 * SIGMA, INF, 5.0 * SIGMA])
    sets = D.Datasets([d, D.validate([_ds()])[0]], red_kernel_baselines=[(B, s), None])
    star = sets.renorm(fr)
    cols, s1 = star.red_kernel_baselines[0]
    assert star.red_kernel_baselines[1] is None and star.has_red_kernel_baselines and not star.has_red_baselines
    assert np.array_equal(cols, B)                                             # the columns are left alone
    assert np.array_equal(s1, np.where(np.isfinite(s), s / fr, s))
    assert star.sets[0].red_kernel == kernel and np.array_equal(star.sets[0].red_sigma, np.asarray(d.red_sigma) / fr)
    if fr in (1.0, 0.5):
        # a power of two: no rounding at all
        a, b = D.ss2_baseline_system(d, B, s), D.ss2_baseline_system(star.sets[0], cols, s1)
        for name in ("A", "g", "Atilde", "M"):
            assert getattr(a, name).tobytes() == getattr(b, name).tobytes(), name
        assert np.array_equal(b.D, a.D * fr * fr) and np.array_equal(b.omega, a.omega * fr * fr)
        assert np.array_equal(b.minv, a.minv) and b.lambda_min == a.lambda_min


def test_system_fields():
    d, _ = case(50, "matern32", 3.0, 5.0)
    B = columns(d, 2)
    system = D.ss2_baseline_system(d, B, [INF, 3e-2])
    assert system._fields == ("A", "g", "omega", "c", "D", "Atilde", "M", "lambda_min")
    A, g, omega = D.ss2_system(d)
    assert np.array_equal(system.A, A) and np.array_equal(system.g, g) and np.array_equal(system.omega, omega)
    Z = _numerics.ss2_innovations(B, A, g)
    assert Z.shape == B.shape and Z.dtype == np.float64 and np.array_equal(Z[:, 0], B[:, 0])
    assert _numerics.ss2_innovations(B, A, g, dtype=LD).dtype == LD
    # the innovations are what ss2_halfchi2 squares
    assert np.allclose(0.5 * np.sum(omega * Z * Z, axis=1), _numerics.ss2_halfchi2(B, A, g, omega), rtol=1e-14, atol=0)
    assert np.allclose(system.D, np.sum(omega * Z * Z, axis=1), rtol=1e-14, atol=0)
    assert np.array_equal(system.c, omega * Z / np.sqrt(system.D)[:, None]) and system.c.flags.c_contiguous
    assert np.allclose(np.diag(system.Atilde), [1.0, 1.0 + 1.0 / (3e-2 ** 2 * system.D[1])], rtol=1e-15, atol=0)
    assert np.array_equal(system.minv, system.M[np.triu_indices(2)]) and system.minv.shape == (3,)
    assert system.lambda_min == float(np.linalg.eigvalsh(system.Atilde)[0])
    assert np.allclose(system.M @ system.Atilde, np.eye(2), rtol=0, atol=1e-12)
    with pytest.raises(ValueError, match="red_kernel"):
        D.ss2_baseline_system(D.validate([_ds()])[0], np.stack([ONES, U]), INF)


# ---------------------------------------------------------------------------------------
# the statement against the dense forms
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("ratio", RATIOS)
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("T", SIZES)
def test_statement_is_the_dense_quadratic_form(T, kernel, ratio, scale):
    d, y0 = case(T, kernel, ratio, scale)
    K = dense(d)
    cond = np.linalg.cond(K)
    assert cond <= 1e5, cond
    for k in KS:
        if k > T:
            continue
        B = columns(d, k)
        y = y0 + 2.0 * SIGMA * B.sum(axis=0)                    # residuals that carry the trend
        bar = 1e-9 * 0.5 * np.sum(y * y / d.flux_err ** 2, axis=1) + 1e-12
        Ky, KB = np.linalg.solve(K, y.T), np.linalg.solve(K, B.T)
        for prior in PRIORS:
            system = system_of(d, B, prior)
            assert system.lambda_min >= D.MIN_BASELINE_EIGENVALUE
            s = np.full(k, INF) if prior == "flat" else 1.0 / np.sqrt(system.D)
            A = B @ KB + np.diag(1.0 / s ** 2)
            b = B @ Ky
            want = 0.5 * (np.einsum("rt,tr->r", y, Ky) - np.einsum("kr,kr->r", b, np.linalg.solve(A, b)))
            got, coef = _numerics.ss2_baseline_halfchi2(y, system, return_coef=True)
            r = float(np.max(np.abs(got - np.maximum(want, 0.0)) / bar))
            _worst["dense"] = max(_worst["dense"], r)
            _worst["lambda_min"] = min(_worst["lambda_min"], system.lambda_min)
            print("T %d %s s %g sigma scale %g K %d %s: cond(K) %.3g, lambda_min %.3g, max |d h| / bar %.3g"
                  % (T, kernel, ratio, scale, k, prior, cond, system.lambda_min, r))
            assert got.shape == (4,) and got.dtype == np.float64 and r <= 1.0 and (got >= 0).all()
            if prior != "flat":
                C = K + B.T @ np.diag(s ** 2) @ B
                full = 0.5 * np.einsum("rt,tr->r", y, np.linalg.solve(C, y.T))
                r = float(np.max(np.abs(got - full) / bar))
                _worst["dense_c"] = max(_worst["dense_c"], r)
                assert r <= 1.0, (r, np.linalg.cond(C))
            # the coefficients are those of the dense generalised least squares
            dense_c = np.linalg.solve(A, b).T
            scale_c = np.abs(dense_c).max(axis=1, keepdims=True)
            # (two solves at cond(K) <= 1e5 and one of the K x K system: 1e-7 of the largest coefficient is far above)
            assert (np.abs(coef / np.sqrt(system.D) - dense_c) <= 1e-7 * scale_c + 1e-18).all()


@pytest.mark.parametrize("prior", PRIORS)
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("T", [4, 5, 63, 129, 333, 2049])
def test_float64_is_the_long_double_statement_to_the_device_bars(T, K, prior):
    """the bars the GPU tests hold the kernel to, on the host's two arithmetics: PARAMS and the residual levels of
    tests/test_gpu_chi2_ss2.py"""
    t, err, y0 = light_curve(T, seed=K)
    for i, (kernel, ratio, scale) in enumerate(PARAMS):
        d = D.validate([dict(time=t, flux=np.ones(T), flux_err=err, **keys(kernel, ratio, scale))])[0]
        system = system_of(d, columns(d, K), prior)
        assert system.lambda_min >= D.MIN_BASELINE_EIGENVALUE
        gamma = gain(system.A, system.g)
        level = (0.0, 3.0, 100.0)[(i + K + T) % 3]
        y = y0 + level * 1.2 * SIGMA
        h64, c64 = _numerics.ss2_baseline_halfchi2(y, system, return_coef=True)
        hld, cld = _numerics.ss2_baseline_halfchi2(y, system, dtype=LD, return_coef=True)
        assert hld.dtype == LD and cld.dtype == LD and cld.shape == (4, K) and h64.dtype == np.float64
        r_h = float(np.max(np.abs(np.asarray(hld - h64, dtype=np.float64)) / ss2_gls_bar(y, system, gamma)))
        r_c = float(np.max(np.abs(np.asarray(cld - c64, dtype=np.float64)) / ss2_coef_bar(y, system, gamma)[:, None]))
        _worst["ld"], _worst["coef"] = max(_worst["ld"], r_h), max(_worst["coef"], r_c)
        _worst["lambda_min"] = min(_worst["lambda_min"], system.lambda_min)
        assert r_h <= 1.0 and r_c <= 1.0, (kernel, ratio, scale, r_h, r_c)


def test_zz_report():
    print("dense checks: largest |d h| / bar %.3g (projected form) and %.3g (K + B S B^T); float64 against long double: "
          "%.3g of ss2_gls_bar, %.3g of ss2_coef_bar; smallest lambda_min %.3g"
          % (_worst["dense"], _worst["dense_c"], _worst["ld"], _worst["coef"], _worst["lambda_min"]))
    assert max(_worst["dense"], _worst["dense_c"], _worst["ld"], _worst["coef"]) <= 1.0


# ---------------------------------------------------------------------------------------
# limits and invariances
@pytest.mark.parametrize("dtype", [np.float64, LD])
@pytest.mark.parametrize("kernel", KERNELS)
def test_m_zero_gives_the_red_kernel_bits(kernel, dtype):
    for T in SIZES[1:] + [333]:
        d, y = case(T, kernel, 3.0, 5.0)
        system = D.ss2_baseline_system(d, columns(d, 2), [INF, INF])
        zero = system._replace(M=np.zeros((2, 2)))
        got, coef = _numerics.ss2_baseline_halfchi2(y, zero, dtype=dtype, return_coef=True)
        want = _numerics.ss2_halfchi2(y, system.A, system.g, system.omega, dtype=dtype)
        assert got.dtype == want.dtype and np.array_equal(got, want) and (got > 0).all() and not coef.any()
        if dtype is np.float64:                                  # (a long double's padding bytes are not its value)
            assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("ratio", RATIOS)
@pytest.mark.parametrize("T", [5, 50, 200])
def test_two_equal_time_scales_are_the_ou_baseline(T, ratio, scale):
    t, err, y = light_curve(T)
    s1, s2 = ratio * SIGMA, 0.5 * ratio * SIGMA
    base = dict(time=t, flux=np.ones(T), flux_err=err)
    two = D.validate([dict(base, red_kernel="ou2", red_sigma=(s1, s2), red_timescale=(scale, scale))])[0]
    one = D.validate([dict(base, red_sigma=float(np.hypot(s1, s2)), red_timescale=scale)])[0]
    for k in KS:
        B = columns(two, k)
        y_k = y + 2.0 * SIGMA * B.sum(axis=0)
        for sig in (np.full(k, INF), np.full(k, 30.0 * err.mean())):
            a, b = D.ss2_baseline_system(two, B, sig), D.ou_baseline_system(one, B, sig)
            got, cg = _numerics.ss2_baseline_halfchi2(y_k, a, dtype=LD, return_coef=True)
            want, cw = _numerics.ou_baseline_halfchi2(y_k, b, dtype=LD, return_coef=True)
            bar = gls_bar(y_k, b) + ss2_gls_bar(y_k, a, gain(a.A, a.g))
            assert (np.abs(np.asarray(got - want, dtype=np.float64)) <= bar).all(), (k, sig[0])


@pytest.mark.parametrize("kernel, ratio, scale", PARAMS)
@pytest.mark.parametrize("T", [5, 50, 200])
def test_flat_columns_in_the_data_do_not_show(T, kernel, ratio, scale):
    d, y = case(T, kernel, ratio, scale)
    for k in KS:
        B = columns(d, k)
        system = D.ss2_baseline_system(d, B, np.full(k, INF))
        gamma = gain(system.A, system.g)
        h0 = _numerics.ss2_baseline_halfchi2(y, system)
        for signs in itertools.product((0.0, 1.0, -2.5), repeat=k):
            if not any(signs):
                continue
            shifted = y + 3.0 * SIGMA * (np.array(signs) @ B)
            h1 = _numerics.ss2_baseline_halfchi2(shifted, system)
            bar = ss2_gls_bar(shifted, system, gamma)           # (at the shifted level: the larger of the two)
            assert (np.abs(h1 - h0) <= bar).all(), (k, signs, np.max(np.abs(h1 - h0) / bar))


@pytest.mark.parametrize("kernel", KERNELS)
def test_a_nan_stays_a_nan_in_its_row_alone(kernel):
    d, y = case(50, kernel, 3.0, 5.0)
    system = D.ss2_baseline_system(d, columns(d, 2), [INF, 1e-2])
    clean, c0 = _numerics.ss2_baseline_halfchi2(y, system, return_coef=True)
    bad = y.copy()
    bad[1, 5] = np.nan
    got, c1 = _numerics.ss2_baseline_halfchi2(bad, system, return_coef=True)
    assert np.isnan(got[1]) and np.array_equal(got[[0, 2, 3]], clean[[0, 2, 3]])
    assert np.isnan(c1[1]).all() and np.array_equal(c1[[0, 2, 3]], c0[[0, 2, 3]])


# ---------------------------------------------------------------------------------------
# the ABI
def _declared():
    text = open(os.path.join(ROOT, "include", "trx_ss.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(trxk_[a-z0-9_]+)\s*\(", text)))


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(ln.split()[-1] for ln in out.splitlines() if " T " in ln)


def test_header_libraries_and_binding_list_the_same_symbol():
    assert _declared() == sorted(_lib.SSGLS_SYMBOLS) == ["trxk_chi2_grid_ss2_baseline"]
    assert not set(_lib.SSGLS_SYMBOLS) & (set(_lib.ABI_SYMBOLS) | set(_lib.WARP_SYMBOLS) | set(_lib.NOISE_SYMBOLS)
                                          | set(_lib.MIX_SYMBOLS) | set(_lib.SHIFT_SYMBOLS) | set(_lib.ROBUST_SYMBOLS)
                                          | set(_lib.GLS_SYMBOLS) | set(_lib.SS_SYMBOLS) | set(_lib.WHITE_SYMBOLS)
                                          | set(_lib.WLIN_SYMBOLS) | set(_lib.DEBUG_SYMBOLS))
    assert len(_lib.ABI_SYMBOLS) == 29
    assert callable(_lib.chi2_grid_ss2_baseline) and callable(_lib.ss2_baseline_blocks)
    others = sorted(f for f in os.listdir(os.path.join(ROOT, "include")) if f != "trx_ss.h")
    assert len(others) == 8
    for other in others:
        assert "trxk_" not in open(os.path.join(ROOT, "include", other)).read().lower()
    if not (os.path.exists(_lib.LIB_PATH) and os.path.exists(_lib.TESTING_LIB_PATH)):
        pytest.skip("libtrx.so not built")
    for path in (_lib.LIB_PATH, _lib.TESTING_LIB_PATH):
        assert [s for s in _exports(path) if s.startswith("trxk_")] == _declared()


def test_argument_checks_need_no_gpu():
    """every refusal comes before anything touches a device: the pointers below are not device memory"""
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libtrx.so not built")
    L = _lib.lib()
    v = [np.zeros(16) for _ in range(10)]
    f, g, o, a, b, w, s, c, m, q = (x.ctypes.data for x in v)
    call = L.trxk_chi2_grid_ss2_baseline
    ERR_ARG = 1
    assert call(None, g, 2, 2, s, INF, 0, o, a, b, w, c, 2, m, q, None) == ERR_ARG            # NULL flux
    assert call(f, None, 2, 2, s, INF, 0, o, a, b, w, c, 2, m, q, None) == ERR_ARG            # NULL grid
    assert call(f, g, 2, 2, s, INF, 0, None, a, b, w, c, 2, m, q, None) == ERR_ARG            # NULL out
    assert call(f, g, 2, 2, s, INF, 0, o, None, b, w, c, 2, m, q, None) == ERR_ARG            # NULL A
    assert call(f, g, 2, 2, s, INF, 0, o, a, None, w, c, 2, m, q, None) == ERR_ARG            # NULL g
    assert call(f, g, 2, 2, s, INF, 0, o, a, b, None, c, 2, m, q, None) == ERR_ARG            # NULL omega
    assert call(f, g, 2, 2, s, INF, 0, o, a, b, w, None, 2, m, q, None) == ERR_ARG            # NULL columns
    assert call(f, g, 2, 2, s, INF, 0, o, a, b, w, c, 2, None, q, None) == ERR_ARG            # NULL minv
    assert b"null pointer" in L.trx_last_error()
    assert call(f, g, 2, -1, s, INF, 0, o, a, b, w, c, 2, m, q, None) == ERR_ARG              # n < 0
    assert call(f, g, 0, 2, s, INF, 0, o, a, b, w, c, 2, m, q, None) == ERR_ARG               # n_time < 1
    assert call(f, g, -3, 0, s, INF, 0, o, a, b, w, c, 2, m, q, None) == ERR_ARG              # ... also with no rows
    assert b"n_time" in L.trx_last_error()
    for k in (0, -1, 5, 1 << 20):
        assert call(f, g, 2, 2, s, INF, 0, o, a, b, w, c, k, m, q, None) == ERR_ARG           # n_terms outside 1 .. 4
        assert call(f, g, 2, 0, s, INF, 0, o, a, b, w, c, k, m, q, None) == ERR_ARG           # ... also with no rows
    assert b"n_terms" in L.trx_last_error()
    for value in (np.nan, INF, -INF):
        bad = np.zeros(16)
        bad[2] = value
        assert call(f, g, 2, 2, s, INF, 0, o, a, b, w, c, 2, bad.ctypes.data, q, None) == ERR_ARG      # minv not finite
    for k in (1, 2, 3, 4):
        assert call(f, g, 2, 0, None, INF, 0, o, a, b, w, c, k, m, None, None) == 0           # n == 0: nothing to launch
    assert not any(x.any() for x in v)
