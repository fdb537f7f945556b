"""Baseline terms marginalised next to a grid of white-noise candidates, on the host: the keys
`white_baseline` / `white_baseline_sigma`, their renormalisation, datasets.white_baseline_system +
_numerics.white_baseline_halfchi2 against the dense statement of the marginal (determinants included), and the ABI entry of
the reduction (include/trx_gls.h, prefix trxb_).  No GPU: every check here ends before the first device call.

Bars, none of them chosen from results:
  dense marginal: the spread over rows of T - dense <= 1e-11 (1 + |T|) (the dataset's dropped constant cancels in the
        spread; the statement's own spread measured 6e-14 at |T| = 50);
  flat priors: adding a combination of the columns to y moves T by at most 1e-10;
  large finite priors: s_k = 1e3 adds delta = 1 / (s_k^2 D_jk) to a unit diagonal: the lnc move by at most K delta /
        lambda_min, a quadratic form by at most S2 delta / lambda_min^2, and T agrees with the flat priors' to these plus
        1e-11 (1 + |T|);
  s_k = 1e-9: A_j >= diag(1 / s^2), so 0 <= 0.5 S2_j - h_j <= 0.5 s^2 |b_j|^2 and the soft minimum, 1-Lipschitz, moves by
        at most the largest of these; ln det A_j - K ln(1 / s^2) <= s^2 sum_k D_jk, half of which may reach a lnc;
  one candidate (1, 0, 1): baseline_halfchi2 within tests/test_gpu_chi2_baseline.py's bar for h,
        1e-12 x 0.5 S2 x (1 + 4 sqrt(K / lambda_min)) + 1e-12;
  renorm: lnc to 1e-13 (tests/test_datasets_white_grid_api.py) + 16 eps K^2 / lambda_min (the rounding of the scaled
        system's entries through its determinant)."""
import math
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
NAN = float("nan")
EPS = np.finfo(np.float64).eps
LD = np.longdouble
GRID = [(1.0, 0.0, 1.0), (1.5, 5e-4, 3.0)]
U = np.linspace(-1.0, 1.0, 7)
COLS = np.stack([np.ones(7), U])
# the issue's inputs: eight candidates with jitters
CANDS8 = lc.white_noise_grid([1.0, 1.5, 2.0, 3.0], [0.0, 5e-4])


def _ds(**extra):
    d = {"time": np.linspace(-0.1, 0.1, 7), "flux": np.full(7, 0.999), "flux_err": np.linspace(1e-3, 2e-3, 7)}
    d.update(extra)
    return d


def lin_case(T, K, sigmas="finite", seed=0, grid=CANDS8):
    """(Dataset, grid, B [K][T], sigmas [K], y [6][T]): errors from 5e-4 to 2e-3, priors from 1e-3 to 5e-3 (or flat), columns
    u^p, residuals of the errors' size plus a trend of 3e-3"""
    rng = np.random.default_rng(1000 * T + 10 * K + seed)
    t = rng.uniform(-0.2, 0.2, T)
    err = rng.uniform(5e-4, 2e-3, T)
    u = np.linspace(-1.0, 1.0, T)
    B = np.stack([u ** p for p in range(K)])
    sig = rng.uniform(1e-3, 5e-3, K) if sigmas == "finite" else np.full(K, float(sigmas))
    y = err * rng.normal(0.0, 1.0, (6, T)) + 3e-3 * rng.normal(0.0, 1.0, (6, 1)) * B[-1]
    dicts = [{"time": t, "flux": np.ones(T), "flux_err": err, "white_grid": grid, "white_baseline": B,
              "white_baseline_sigma": sig}]
    sets = D.validate(dicts)
    B2, s2 = D.white_baselines(dicts, sets)[0]
    return sets[0], D.white_grids(dicts, sets)[0], B2, s2, y


# ---------------------------------------------------------------------------------------
# validation
@pytest.mark.parametrize("cols, sigma", [(COLS, None), (COLS, 5e-3), (COLS, [INF, 5e-3]), (U, None), (U, 2.0),
                                         (np.stack([np.ones(7), U, U ** 2, U ** 3]), [INF, 1.0, 1.0, 1.0])])
def test_validate_accepts_the_keys(cols, sigma):
    extra = {"white_grid": GRID, "white_baseline": cols}
    if sigma is not None:
        extra["white_baseline_sigma"] = sigma
    dicts = [_ds(), _ds(**extra)]
    sets = D.validate(dicts)
    got = D.white_baselines(dicts, sets)
    assert got[0] is None
    B, s = got[1]
    want = np.atleast_2d(np.asarray(cols, dtype=np.float64))
    assert B.dtype == np.float64 and B.flags["C_CONTIGUOUS"] and np.array_equal(B, want)
    assert s.shape == (want.shape[0],) and np.array_equal(s, np.broadcast_to(INF if sigma is None else sigma, s.shape))
    assert type(sets[1]) is D.Dataset and sets[1].baseline is None and sets[1].offset_sigma is None
    ds = D.Datasets(sets, white_grids=D.white_grids(dicts, sets), white_baselines=got)
    assert ds.has_white_baselines and ds.has_white_grids and not ds.has_baselines and not ds.has_red_baselines
    assert not D.Datasets(sets).has_white_baselines and D.Datasets(sets).white_baselines == (None, None)
    import inspect
    assert list(inspect.signature(D.Datasets.__init__).parameters)[-1] == "white_baselines"


def test_dataset_gets_no_new_field_and_none_is_no_key():
    assert D.Dataset._fields == ("time", "flux", "flux_err", "exptime", "nsamples", "offset_sigma", "baseline",
                                 "baseline_sigma", "red_grid", "red_sigma", "red_timescale")
    dicts = [_ds(white_grid=GRID), _ds(white_grid=GRID, white_baseline=None, white_baseline_sigma=None)]
    a, b = D.validate(dicts)
    for name, x, y in zip(a._fields, a, b):
        assert (np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y), name
    assert D.white_baselines(dicts, [a, b]) == [None, None]
    with pytest.raises(ValueError, match="white_baselines: 1 dicts for 2 datasets"):
        D.white_baselines([_ds()], D.validate([_ds(), _ds()]))
    with pytest.raises(ValueError, match="white_baselines: 1 pairs for 2 datasets"):
        D.Datasets(D.validate([_ds(), _ds()]), white_baselines=[None])


def test_nan_dropped_points_take_their_entries_along():
    t = np.linspace(-0.1, 0.1, 7)
    t[2] = np.nan
    cols = COLS.copy()
    cols[1, 2] = np.nan                                                  # (the dropped point's entry need not be finite)
    dicts = [_ds(time=t, white_grid=GRID, white_baseline=cols)]
    sets = D.validate(dicts)
    B, _ = D.white_baselines(dicts, sets)[0]
    assert sets[0].time.size == 6 and B.shape == (2, 6) and np.array_equal(B, np.delete(COLS, 2, axis=1))
    cols[1, 3] = np.inf                                                  # ... a kept point's must
    with pytest.raises(ValueError, match="dataset 0.*white_baseline.*finite"):
        D.validate([_ds(time=t, white_grid=GRID, white_baseline=cols)])


@pytest.mark.parametrize("extra", [
    {"white_baseline_sigma": 1e-3},                                                          # a sigma without columns
    {"white_baseline": np.ones(6)}, {"white_baseline": np.ones((2, 6))}, {"white_baseline": np.ones((2, 2, 7))},
    {"white_baseline": 3.0}, {"white_baseline": np.ones((0, 7))},                            # a wrong shape
    {"white_baseline": np.stack([np.ones(7), U, U ** 2, U ** 3, U ** 4])},                   # more than four columns
    {"white_baseline": np.where(np.arange(7) == 3, NAN, 1.0)}, {"white_baseline": np.where(np.arange(7) == 3, INF, 1.0)},
    {"white_baseline": np.stack([np.ones(7), np.zeros(7)])},                                 # a zero column
    {"white_baseline": True}, {"white_baseline": "trend"},                                   # a bool or a string
    {"white_baseline": COLS, "white_baseline_sigma": True}, {"white_baseline": COLS, "white_baseline_sigma": "wide"},
    {"white_baseline": COLS, "white_baseline_sigma": 0.0}, {"white_baseline": COLS, "white_baseline_sigma": -1.0},
    {"white_baseline": COLS, "white_baseline_sigma": NAN}, {"white_baseline": COLS, "white_baseline_sigma": [1.0, 1.0, 1.0]},
    {"white_baseline": np.stack([np.ones(7), np.ones(7)])},                                  # collinear, flat priors
    {"white_baseline": np.stack([U, 2.0 * U])},
])
def test_validate_rejects(extra):
    with pytest.raises(ValueError, match="dataset 1.*white_baseline"):
        D.validate([_ds(), _ds(white_grid=GRID, **extra)])
    with pytest.raises(ValueError, match="dataset 1.*white_baseline"):
        D.white_baselines([_ds(), _ds(white_grid=GRID, **extra)], D.validate([_ds(), _ds()]))


def test_collinear_columns_are_found_per_candidate_and_finite_priors_mend_them():
    two = np.stack([np.ones(7), np.ones(7)])
    with pytest.raises(ValueError, match="collinear.*smallest eigenvalue"):
        D.validate([_ds(white_grid=GRID, white_baseline=two)])
    assert D.validate([_ds(white_grid=GRID, white_baseline=two, white_baseline_sigma=1e-3)])
    # every candidate's system is looked at: lambda_min is per candidate, and a singular one leaves no inverse
    dicts = [_ds(white_grid=GRID)]
    sets = D.validate(dicts)
    system = D.white_baseline_system(sets[0], D.white_grids(dicts, sets)[0], two, np.full(2, INF))
    assert system.lambda_min.shape == (2,) and (system.lambda_min < D.MIN_BASELINE_EIGENVALUE).all()
    assert all(M is None for M in system.M) or np.isnan(system.lnc).all() or (system.lambda_min > 0).all()


def test_the_keys_need_white_grid():
    for extra in ({}, {"offset_sigma": 1e-3}, {"red_sigma": 1e-3, "red_timescale": 0.1}, {"t0_grid": [(0.0, 1.0)]}):
        with pytest.raises(ValueError, match="dataset 0.*white_baseline"):
            D.validate([_ds(white_baseline=COLS, **extra)])
    with pytest.raises(ValueError, match="dataset 0.*white_baseline needs white_grid"):
        D.validate([_ds(white_baseline=COLS)])


@pytest.mark.parametrize("extra", [
    {"offset_sigma": 1e-3}, {"offset_sigma": INF}, {"baseline": np.linspace(-1, 1, 7)},
    {"baseline": np.linspace(-1, 1, 7), "baseline_sigma": 2.0},
    {"red_sigma": 1e-3, "red_timescale": 0.1}, {"red_grid": [(1e-3, 0.1, 1.0)]},
    {"red_kernel": "matern32", "red_sigma": 1e-3, "red_timescale": 0.1},
    {"red_kernel": "ou2", "red_sigma": (1e-3, 2e-3), "red_timescale": (0.1, 1.0)},
    {"red_sigma": 1e-3, "red_timescale": 0.1, "red_baseline": np.ones(7)},
    {"outlier_frac": 0.05, "outlier_scale": 10.0},
], ids=["offset", "flat-offset", "baseline", "baseline_sigma", "red_sigma", "red_grid", "matern32", "ou2", "red_baseline",
        "outliers"])
def test_the_keys_stand_next_to_white_grid_and_t0_grid_alone(extra):
    assert D.validate([_ds(**extra)])                                    # (the neighbour alone is a valid dataset)
    with pytest.raises(ValueError, match="dataset 0.*not built"):
        D.validate([_ds(white_grid=GRID, white_baseline=COLS, **extra)])
    with pytest.raises(ValueError, match="dataset 0.*white_baseline.*not built"):
        D.white_baselines([_ds(white_grid=GRID, white_baseline=COLS, **extra)], D.validate([_ds()]))
    with pytest.raises(ValueError, match="dataset 0"):
        D.validate([_ds(white_baseline=COLS, **extra)])                  # ... nor without white_grid
    dicts = [_ds(white_grid=GRID, white_baseline=COLS, t0_grid=[(0.0, 1.0), (0.01, 2.0)])]
    sets = D.validate(dicts)
    assert D.white_baselines(dicts, sets)[0][0].shape == (2, 7) and D.t0_grids(dicts, sets)[0].shape == (2, 2)


def test_the_plain_keys_next_to_white_grid_stay_refused():
    for extra in ({"offset_sigma": INF}, {"baseline": U, "baseline_sigma": 1e-3}):
        with pytest.raises(ValueError, match="dataset 0.*white_grid.*not built"):
            D.validate([_ds(white_grid=GRID, **extra)])


def test_prepare_dataset_builds_the_columns_on_the_kept_bins():
    import inspect
    assert list(inspect.signature(lc.prepare_dataset).parameters)[-2:] == ["white_baseline_order", "white_baseline_sigma"]
    t = np.linspace(-0.4, 0.4, 400)
    y = 1.0 + 1e-3 * np.sin(37.0 * t)
    plain = lc.prepare_dataset(t, y, n_bins=20, n_sigma=10, white_grid=CANDS8)
    assert "white_baseline" not in plain and "white_baseline_sigma" not in plain
    d = lc.prepare_dataset(t, y, n_bins=20, n_sigma=10, white_grid=CANDS8, white_baseline_order=1,
                           white_baseline_sigma=[INF, 5e-3])
    assert np.array_equal(d["white_baseline"], lc.trend_columns(d["time"], 1)) and d["white_baseline"].shape[0] == 2
    assert d["white_baseline_sigma"] == [INF, 5e-3]
    sets = D.validate([d])
    B, s = D.white_baselines([d], sets)[0]
    assert B.shape == (2, sets[0].time.size) and np.array_equal(s, [INF, 5e-3])
    with pytest.raises(ValueError, match="dataset 0.*white_baseline needs white_grid"):
        D.validate([lc.prepare_dataset(t, y, n_bins=20, n_sigma=10, white_baseline_order=1)])


def test_fused_evaluation_is_refused_before_any_device_call(monkeypatch):
    from test_datasets_api import _target
    from triceratops_amd.triceratops import target
    tg = _target()
    monkeypatch.setattr(target, "_prepare", lambda self, *a, **k: ([], 0))
    dicts = [_ds(), _ds(white_grid=GRID, white_baseline=COLS)]
    sets = D.validate(dicts)
    ds = D.Datasets(sets, white_grids=D.white_grids(dicts, sets), white_baselines=D.white_baselines(dicts, sets))
    with pytest.raises(NotImplementedError, match="evaluation='fused' with a white"):
        tg._datasets_pass(ds, 3.0, {}, 0, "fused")


def test_the_switch_is_listed_with_the_others():
    from triceratops_amd import fused
    assert fused.DATASET_WHITE_BASELINES is None and "DATASET_WHITE_BASELINES" in fused.switches.__doc__
    box = {}
    with fused.switches(DATASET_WHITE_BASELINES=box):
        assert fused.DATASET_WHITE_BASELINES is box
    assert fused.DATASET_WHITE_BASELINES is None
    assert fused._Dataset._fields == ("time", "flux", "inv_var", "exptime", "nsamples", "term", "shift")
    assert fused._Dataset._field_defaults == {"term": None, "shift": None}
    assert fused._WhiteLin._fields == ("w", "lnc", "basis", "minv")
    assert fused._WhiteLin._fields[:2] == fused._WhiteMix._fields        # (a type of its own, not a white_grid's pair grown)
    assert not issubclass(fused._WhiteLin, fused._WhiteMix) and not issubclass(fused._WhiteMix, fused._WhiteLin)


# ---------------------------------------------------------------------------------------
# the system and the statement
@pytest.mark.parametrize("K", [1, 2, 4])
@pytest.mark.parametrize("T", [5, 50])
def test_system_shapes_units_and_normalisation(T, K):
    d, grid, B, sig, y = lin_case(T, K)
    s = D.white_baseline_system(d, grid, B, sig)
    J = grid.shape[0]
    w, lnc0 = D.white_mix_system(d, grid)
    assert np.array_equal(s.w, w) and np.array_equal(s.B, B)
    assert s.minv.shape == (J, K * (K + 1) // 2) and s.minv.flags["C_CONTIGUOUS"] and np.isfinite(s.minv).all()
    assert s.lnc.shape == (J,) and s.lambda_min.shape == (J,) and s.D.shape == (J, K) and len(s.M) == J
    assert (s.lambda_min >= D.MIN_BASELINE_EIGENVALUE).all()
    total = math.fsum(math.exp(v) for v in s.lnc.tolist())
    assert abs(total - 1.0) <= 8 * EPS * J
    iu = np.triu_indices(K)
    for j in range(J):
        one = D.linear_system(w[j], B, sig)
        assert np.array_equal(s.D[j], one.D) and s.lambda_min[j] == one.lambda_min
        # minv is A_j^-1 in the units of the raw sums: its product with A_j is the unit matrix
        A = (B * w[j]) @ B.T + np.diag(1.0 / sig ** 2)
        Ainv = np.zeros((K, K))
        Ainv[iu] = s.minv[j]
        Ainv = Ainv + np.triu(Ainv, 1).T
        assert np.abs(Ainv @ A - np.eye(K)).max() <= 64 * EPS * K / one.lambda_min
        # lnc_j - ln pi_j - 0.5 sum ln w_j + 0.5 ln det A_j is one constant
    c = [s.lnc[j] - math.log(grid[j, 2]) - 0.5 * math.fsum(np.log(w[j]).tolist())
         + 0.5 * np.linalg.slogdet((B * w[j]) @ B.T + np.diag(1.0 / sig ** 2))[1] for j in range(J)]
    assert max(c) - min(c) <= 64 * EPS * max(abs(x) for x in c)


@pytest.mark.parametrize("K", [1, 2, 4])
@pytest.mark.parametrize("T", [5, 50])
def test_statement_is_the_dense_marginal_with_determinants(T, K):
    d, grid, B, sig, y = lin_case(T, K)
    s = D.white_baseline_system(d, grid, B, sig)
    got, cand, coef = _numerics.white_baseline_halfchi2(y, s, return_candidates=True, return_coef=True)
    assert got.dtype == np.float64 and got.shape == (6,) and cand.shape == (6, 8) and coef.shape == (6, 8, K)
    err = d.flux_err
    dense = []
    for row in y:
        terms = []
        for k, jit, pi_j in grid:
            C = np.diag(k * k * err * err + jit * jit) + B.T @ np.diag(sig ** 2) @ B
            terms.append(math.log(pi_j) - 0.5 * np.linalg.slogdet(C)[1] - 0.5 * row @ np.linalg.solve(C, row))
        top = max(terms)
        dense.append(-(top + math.log(math.fsum(math.exp(v - top) for v in terms))))
    diff = got - np.array(dense)
    print("T %d K %d: spread of T - dense %.3g at |T| <= %.3g" % (T, K, np.ptp(diff), np.abs(got).max()))
    assert np.ptp(diff) <= 1e-11 * (1.0 + np.abs(got).max())
    assert (got >= 0).all()
    # the coefficients are the posterior means: the generalised least-squares solution under candidate j's weights
    for j in (0, 7):
        A = (B * s.w[j]) @ B.T + np.diag(1.0 / sig ** 2)
        want = np.linalg.solve(A, (B * s.w[j]) @ y.T).T
        assert np.allclose(coef[:, j], want, rtol=1e-9, atol=1e-12)
    # the long-double statement and the float64 one
    ld = _numerics.white_baseline_halfchi2(y, s, dtype=LD)
    assert ld.dtype == LD and (np.abs(ld.astype(np.float64) - got) <= 1e-11 * (1.0 + np.abs(got))).all()


@pytest.mark.parametrize("K", [1, 2, 4])
@pytest.mark.parametrize("T", [5, 50])
def test_flat_priors_ignore_any_combination_of_the_columns(T, K):
    d, grid, B, sig, y = lin_case(T, K, sigmas=INF)
    s = D.white_baseline_system(d, grid, B, sig)
    base = _numerics.white_baseline_halfchi2(y, s)
    rng = np.random.default_rng(T + K)
    for _ in range(4):
        a = 3e-3 * rng.normal(0.0, 1.0, (6, K))
        moved = _numerics.white_baseline_halfchi2(y + a @ B, s)
        print("T %d K %d: max |d T| %.3g" % (T, K, np.abs(moved - base).max()))
        assert (np.abs(moved - base) <= 1e-10).all()
    # large finite priors are the flat ones
    wide = D.white_baseline_system(d, grid, B, np.full(K, 1e3))
    delta = float(np.max(1.0 / (1e6 * s.D)))                             # what 1 / (s_k^2 D_jk) adds to a unit diagonal
    lam = float(s.lambda_min.min())
    bar_lnc = K * delta / lam + 1e-13                                    # (0.5 d ln det <= 0.5 K delta / lam, twice: normalised)
    assert (np.abs(wide.lnc - s.lnc) <= bar_lnc).all()
    S2 = max(float(np.sum(s.w[j] * y * y, axis=-1).max()) for j in range(8))
    bar = bar_lnc + 0.5 * S2 * delta / lam ** 2 + 1e-11 * (1.0 + np.abs(base))
    assert (np.abs(_numerics.white_baseline_halfchi2(y, wide) - base) <= bar).all()


@pytest.mark.parametrize("K", [1, 2, 4])
@pytest.mark.parametrize("T", [5, 50])
def test_vanishing_priors_are_the_white_mix(T, K):
    d, grid, B, _, y = lin_case(T, K)
    tiny = 1e-9
    s = D.white_baseline_system(d, grid, B, np.full(K, tiny))
    w, lnc = D.white_mix_system(d, grid)
    assert (np.abs(s.lnc - lnc) <= 0.5 * tiny ** 2 * s.D.sum(axis=1).max() + 1e-13).all()
    got, cand = _numerics.white_baseline_halfchi2(y, s, return_candidates=True)
    want, h = _numerics.white_mix_halfchi2(y, w, lnc, return_candidates=True)
    b2 = np.stack([np.sum(((w[j] * y) @ B.T) ** 2, axis=-1) for j in range(8)], axis=-1)       # [6][J] |b_j|^2
    bar = 0.5 * tiny ** 2 * b2
    assert (cand <= h * (1 + 8 * EPS)).all() and (h - cand <= bar + 64 * EPS * (1 + h)).all()
    assert (np.abs(got - want) <= bar.max(axis=-1) + np.abs(s.lnc - lnc).max() + 64 * EPS * (1 + np.abs(want))).all()
    # minv = 0: the white mix itself
    zero = _numerics.white_baseline_halfchi2(y, s._replace(minv=np.zeros_like(s.minv), lnc=lnc))
    assert (np.abs(zero - want) <= 64 * EPS * (1 + np.abs(want))).all()


@pytest.mark.parametrize("sigmas", ["finite", INF])
@pytest.mark.parametrize("K", [1, 2, 4])
@pytest.mark.parametrize("T", [5, 50])
def test_one_unit_candidate_is_the_plain_baseline(T, K, sigmas):
    d, grid, B, sig, y = lin_case(T, K, sigmas=sigmas, grid=[(1.0, 0.0, 1.0)])
    s = D.white_baseline_system(d, grid, B, sig)
    assert s.lnc.tolist() == [0.0]
    w = 1.0 / (d.flux_err * d.flux_err)
    assert s.w[0].tobytes() == w.tobytes()
    got = _numerics.white_baseline_halfchi2(y, s)
    want = _numerics.baseline_halfchi2(y, w, B, sig)
    S2 = np.sum(w * y * y, axis=-1)
    bar = 1e-12 * 0.5 * S2 * (1.0 + 4.0 * math.sqrt(K / s.lambda_min[0])) + 1e-12
    assert (np.abs(got - want) <= bar).all()


@pytest.mark.parametrize("fr", [0.3, 0.9])
@pytest.mark.parametrize("K", [1, 2, 4])
@pytest.mark.parametrize("T", [5, 50])
def test_renorm_scales_the_sigmas_and_keeps_the_weights(T, K, fr):
    d, grid, B, sig, _ = lin_case(T, K)
    sig = sig.copy()
    sig[0] = INF                                                         # (a flat prior stays flat)
    sets = D.Datasets([d, D.validate([_ds()])[0]], white_grids=[grid, None], white_baselines=[(B, sig), None])
    star = sets.renorm(fr)
    B1, s1 = star.white_baselines[0]
    assert star.white_baselines[1] is None and star.has_white_baselines
    assert np.array_equal(B1, B) and s1[0] == INF and np.array_equal(s1[1:], sig[1:] / fr)
    assert np.array_equal(sets.white_baselines[0][1], sig)               # (the caller's pair is left alone)
    a = D.white_baseline_system(d, grid, B, sig)
    b = D.white_baseline_system(star.sets[0], star.white_grids[0], B1, s1)
    print("T %d K %d fr %g: max |d lnc| %.3g" % (T, K, fr, np.abs(a.lnc - b.lnc).max()))
    assert (np.abs(a.lnc - b.lnc) <= 1e-13 + 16 * EPS * K * K / a.lambda_min.min()).all()
    assert np.allclose(b.minv, a.minv / (fr * fr), rtol=64 * EPS * K * K / a.lambda_min.min(), atol=0)


def test_statement_edge_values():
    d, grid, B, sig, y = lin_case(17, 2)
    s = D.white_baseline_system(d, grid, B, sig)
    y = y.copy()
    y[1, 5] = np.nan
    got, cand = _numerics.white_baseline_halfchi2(y, s, return_candidates=True)
    assert np.isnan(got[1]) and np.isfinite(got[[0, 2, 3]]).all()
    for low in (-800.0, -INF):
        off = np.full(8, low)
        off[2] = 0.0
        t0, c0 = _numerics.white_baseline_halfchi2(y[0], s._replace(lnc=off), return_candidates=True)
        assert t0 == c0[2] and abs(c0[2] - cand[0, 2]) <= 64 * EPS * cand[0, 2]     # (one row and six sum in other orders)
    assert _numerics.white_baseline_halfchi2(np.zeros(17), s._replace(lnc=np.log(np.full(8, 0.125)))) >= 0.0
    only_coef = _numerics.white_baseline_halfchi2(y[0], s, return_coef=True)
    assert len(only_coef) == 2 and only_coef[1].shape == (8, 2)


# ---------------------------------------------------------------------------------------
# the ABI
def _declared():
    text = open(os.path.join(ROOT, "include", "trx_gls.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(trxb_[a-z0-9_]+)\s*\(", text)))


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(ln.split()[-1] for ln in out.splitlines() if " T " in ln)


def test_header_libraries_and_binding_list_the_same_symbols():
    assert _declared() == sorted(_lib.WLIN_SYMBOLS) == ["trxb_chi2_grid_white_baseline"]
    assert not set(_lib.WLIN_SYMBOLS) & (set(_lib.ABI_SYMBOLS) | set(_lib.WARP_SYMBOLS) | set(_lib.NOISE_SYMBOLS)
                                         | set(_lib.MIX_SYMBOLS) | set(_lib.SHIFT_SYMBOLS) | set(_lib.ROBUST_SYMBOLS)
                                         | set(_lib.GLS_SYMBOLS) | set(_lib.SS_SYMBOLS) | set(_lib.WHITE_SYMBOLS)
                                         | set(_lib.DEBUG_SYMBOLS))
    assert len(_lib.ABI_SYMBOLS) == 29
    assert callable(_lib.chi2_grid_white_baseline) and callable(_lib.white_lin_blocks)
    others = sorted(f for f in os.listdir(os.path.join(ROOT, "include")) if f != "trx_gls.h")
    assert len(others) == 8
    for other in others:
        assert "trxb_" not in open(os.path.join(ROOT, "include", other)).read().lower()
    # the header names no prefix but the core's, the OU filter's and its own two
    text = open(os.path.join(ROOT, "include", "trx_gls.h")).read().lower()
    assert set(re.findall(r"\btrx[a-z]?_", text)) == {"trx_", "trxn_", "trxg_", "trxb_"}
    if not (os.path.exists(_lib.LIB_PATH) and os.path.exists(_lib.TESTING_LIB_PATH)):
        pytest.skip("libtrx.so not built")
    for path in (_lib.LIB_PATH, _lib.TESTING_LIB_PATH):
        assert [s for s in _exports(path) if s.startswith("trxb_")] == _declared()


def test_white_lin_blocks_mirrors_the_launcher():
    # 4 rows a block below the cap
    assert _lib.white_lin_blocks(1, 100, 1, 1) == 1 and _lib.white_lin_blocks(5, 100, 8, 4) == 2
    # up to 24 sums a row: 128 VGPRs, four blocks a CU; up to 35: 168, three; 40: 256, two
    assert _lib.white_lin_blocks(10 ** 6, 100, 2, 1) == 1024 and _lib.white_lin_blocks(10 ** 6, 100, 8, 2) == 1024
    assert _lib.white_lin_blocks(10 ** 6, 100, 5, 4) == 768 and _lib.white_lin_blocks(10 ** 6, 100, 7, 4) == 768
    assert _lib.white_lin_blocks(10 ** 6, 100, 8, 3) == 768 and _lib.white_lin_blocks(10 ** 6, 100, 8, 4) == 512
    # the staged vectors and the 80 doubles of inverses never take more than 33 KB a block, four of which fit 160 KB: the
    # registers decide
    assert _lib.white_lin_blocks(10 ** 6, 1364, 1, 1) == 1024           # 3 x 1364 x 8 B = 32736 B
    assert _lib.white_lin_blocks(10 ** 6, 1365, 1, 1) == 1024           # past the stage limit: no LDS
    assert _lib.white_lin_blocks(10 ** 6, 314, 8, 4) == 512 and _lib.white_lin_blocks(10 ** 6, 315, 8, 4) == 512


def test_argument_checks_need_no_gpu():
    """every refusal comes before anything touches a device: the pointers below are not device memory"""
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libtrx.so not built")
    L = _lib.lib()
    v = [np.zeros(96) for _ in range(10)]
    f, g, o, w, b, s, m, c, k, q = (x.ctypes.data for x in v)
    call = L.trxb_chi2_grid_white_baseline
    ERR_ARG = 1
    assert call(None, g, 2, 2, s, INF, 0, o, w, b, 2, 2, m, c, k, q, None) == ERR_ARG          # NULL flux
    assert call(f, None, 2, 2, s, INF, 0, o, w, b, 2, 2, m, c, k, q, None) == ERR_ARG          # NULL grid
    assert call(f, g, 2, 2, s, INF, 0, None, w, b, 2, 2, m, c, k, q, None) == ERR_ARG          # NULL out
    assert call(f, g, 2, 2, s, INF, 0, o, None, b, 2, 2, m, c, k, q, None) == ERR_ARG          # NULL weights
    assert call(f, g, 2, 2, s, INF, 0, o, w, None, 2, 2, m, c, k, q, None) == ERR_ARG          # NULL basis
    assert call(f, g, 2, 2, s, INF, 0, o, w, b, 2, 2, None, c, k, q, None) == ERR_ARG          # NULL minv
    assert call(f, g, 2, 2, s, INF, 0, o, w, b, 2, 2, m, None, k, q, None) == ERR_ARG          # NULL lnc
    assert b"null pointer" in L.trx_last_error()
    assert call(f, g, 2, -1, s, INF, 0, o, w, b, 2, 2, m, c, k, q, None) == ERR_ARG            # n < 0
    assert call(f, g, 0, 2, s, INF, 0, o, w, b, 2, 2, m, c, k, q, None) == ERR_ARG             # n_time < 1
    assert call(f, g, -3, 0, s, INF, 0, o, w, b, 2, 2, m, c, k, q, None) == ERR_ARG            # ... also with no rows
    assert b"n_time" in L.trx_last_error()
    for n_cand in (0, -1, 9, 64):
        assert call(f, g, 2, 2, s, INF, 0, o, w, b, n_cand, 2, m, c, k, q, None) == ERR_ARG    # n_cand outside 1 ... 8
        assert call(f, g, 2, 0, s, INF, 0, o, w, b, n_cand, 2, m, c, k, q, None) == ERR_ARG    # ... also with no rows
    assert b"n_cand" in L.trx_last_error()
    for n_terms in (0, -1, 5, 1 << 20):
        assert call(f, g, 2, 2, s, INF, 0, o, w, b, 2, n_terms, m, c, k, q, None) == ERR_ARG   # n_terms outside 1 ... 4
        assert call(f, g, 2, 0, s, INF, 0, o, w, b, 2, n_terms, m, c, k, q, None) == ERR_ARG
    assert b"n_terms" in L.trx_last_error()
    for bad in (NAN, INF):
        for at in (0, 2):
            lnc = np.zeros(3)
            lnc[at] = bad
            assert call(f, g, 2, 2, s, INF, 0, o, w, b, 3, 2, m, lnc.ctypes.data, k, q, None) == ERR_ARG
            assert call(f, g, 2, 0, s, INF, 0, o, w, b, 3, 2, m, lnc.ctypes.data, None, None, None) == ERR_ARG
    assert b"lnc" in L.trx_last_error()
    for bad in (NAN, INF, -INF):
        for at in (0, 8):                                              # (the last entry of the third candidate's triangle)
            minv = np.zeros(9)
            minv[at] = bad
            assert call(f, g, 2, 2, s, INF, 0, o, w, b, 3, 2, minv.ctypes.data, c, k, q, None) == ERR_ARG
            assert call(f, g, 2, 0, s, INF, 0, o, w, b, 3, 2, minv.ctypes.data, c, None, None, None) == ERR_ARG
    assert b"minv" in L.trx_last_error()
    # n == 0: nothing to launch -- for every n_cand and n_terms, without secdepth and the outputs, -inf in lnc allowed
    lnc = np.array([0.0, -INF, -3.0, 0.0, 0.0, 0.0, 0.0, 0.0])
    for n_cand in range(1, 9):
        for n_terms in range(1, 5):
            assert call(f, g, 2, 0, None, INF, 0, o, w, b, n_cand, n_terms, m, lnc.ctypes.data, None, None, None) == 0
