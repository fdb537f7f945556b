"""A grid of white-noise candidates per dataset on the host: the `white_grid` key -- error scale k and
jitter s, per-point variance k^2 sigma_t^2 + s^2 --, its renormalisation, datasets.white_mix_system +
_numerics.white_mix_halfchi2 against the dense statement of the marginal over the candidates (determinants included), and
the ABI entry of the reduction (include/trx_mix.h, prefix trxv_).  No GPU: every check here ends before the first device
call.

Bars, none of them chosen from results:
  sum_j exp(lnc_j) = 1: to 8 eps J (J roundings of exp, one of the sum's log, one subtraction each);
  the (1, 0) candidate and a power-of-two k: bits;
  renorm: lnc to 1e-13 (every ln w_j[t] moves by 2 ln fr, the same for every candidate; what is left is the rounding of
        T <= 200 logs of size <= 16, half an ulp of 16 each: a random walk of sqrt(200) x 0.9e-15 = 1.3e-14 per sum, halved
        and differenced), w to 8 eps relative (the roundings of err / fr, s / fr, their squares, the sum and the
        reciprocal);
  dense statement: 64 eps (1 + |value| + max |lnc|), value = -ln sum_j pi_j N(y; 0, diag v_j) - (T / 2) ln 2 pi in long
        double from the candidates themselves: w = 1 / v and the logs of w are rounded once each (relative eps in every h_j,
        eps / 2 in each of the T terms of a log-determinant, which is what |value| is made of).
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
NAN = float("nan")
EPS = np.finfo(np.float64).eps
LD = np.longdouble
SIGMA = 1e-3
GRID = [(1.0, 0.0, 1.0), (1.5, 5e-4, 3.0)]
SIZES = [1, 2, 3, 50, 200]
# (k, s / SIGMA, prior weight): scales 0.5 ... 3, jitters 0 ... 3 sigma
CANDS = [(1.0, 0.0, 0.1), (0.5, 0.0, 0.3), (2.0, 1.0, 0.05), (3.0, 0.0, 0.35), (1.5, 3.0, 0.2)]


def _ds(**extra):
    d = {"time": np.linspace(-0.1, 0.1, 7), "flux": np.full(7, 0.999), "flux_err": np.linspace(1e-3, 2e-3, 7)}
    d.update(extra)
    return d


def mix_case(T, level=1.0, seed=0):
    """(Dataset, grid [5][3], y [4][T]): T folded stamps (not in time order), errors varying 3x around SIGMA, residuals of
    `level` times the errors' size (row 0: exactly level sigma each, alternating in sign)"""
    rng = np.random.default_rng(1000 * T + seed)
    t = rng.uniform(-0.2, 0.2, T)
    err = SIGMA * rng.uniform(0.6, 1.8, T)
    y = level * err * rng.normal(0.0, 1.0, (4, T))
    y[0] = level * err * np.where(np.arange(T) % 2, -1.0, 1.0)
    dicts = [{"time": t, "flux": np.ones(T), "flux_err": err, "white_grid": [(k, s * SIGMA, w) for k, s, w in CANDS]}]
    sets = D.validate(dicts)
    return sets[0], D.white_grids(dicts, sets)[0], y


def _logsumexp(v):
    top = max(v)
    return top + math.log(math.fsum(math.exp(x - top) for x in v))


# ---------------------------------------------------------------------------------------
# validation
@pytest.mark.parametrize("grid", [GRID, np.array(GRID), [(1, 0, 5)], [GRID[1]] * 8, [GRID[1], GRID[1]], [(2.0, 0.0, 1.0)],
                                  [(np.float32(1.5), 0, 1e-300), (0.5, 2e-3, 1e-300)]])
def test_validate_accepts_a_grid(grid):
    dicts = [_ds(), _ds(white_grid=grid)]
    sets = D.validate(dicts)
    got = D.white_grids(dicts, sets)
    assert got[0] is None
    g = got[1]
    want = np.array(grid, dtype=np.float64)
    assert g.dtype == np.float64 and g.shape == want.shape and g.flags["C_CONTIGUOUS"]
    assert np.array_equal(g[:, :2], want[:, :2])
    assert abs(math.fsum(g[:, 2]) - 1.0) <= 4 * EPS and np.allclose(g[:, 2], want[:, 2] / want[:, 2].sum(), rtol=4 * EPS)
    assert type(sets[1]) is D.Dataset and sets[1].red_grid is None and sets[1].red_sigma is None
    ds = D.Datasets(sets, white_grids=got)
    assert ds.has_white_grids and not D.Datasets(sets).has_white_grids and not ds.has_red_noise
    assert D.Datasets(sets).white_grids == (None, None)
    assert D.MAX_WHITE_CANDIDATES == 8


def test_dataset_gets_no_new_field_and_none_is_no_key():
    assert D.Dataset._fields == ("time", "flux", "flux_err", "exptime", "nsamples", "offset_sigma", "baseline",
                                 "baseline_sigma", "red_grid", "red_sigma", "red_timescale")
    for extra in ({}, {"offset_sigma": 1e-3}, {"red_sigma": 1e-3, "red_timescale": 0.1}, {"outlier_frac": 0.1, "outlier_scale": 5.0}):
        dicts = [_ds(**extra), _ds(white_grid=None, **extra)]
        a, b = D.validate(dicts)
        for name, x, y in zip(a._fields, a, b):
            assert (np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y), name
        assert D.white_grids(dicts, [a, b]) == [None, None]
    with pytest.raises(ValueError, match="white_grids: 1 dicts for 2 datasets"):
        D.white_grids([_ds()], D.validate([_ds(), _ds()]))
    with pytest.raises(ValueError, match="white_grids: 1 grids for 2 datasets"):
        D.Datasets(D.validate([_ds(), _ds()]), white_grids=[None])


@pytest.mark.parametrize("extra", [
    {"white_grid": []}, {"white_grid": [GRID[0]] * 9},                                       # 1 ... 8 candidates
    {"white_grid": [(1.0, 0.0)]}, {"white_grid": [(1.0, 0.0, 1.0, 1.0)]}, {"white_grid": (1.0, 0.0, 1.0)},
    {"white_grid": "grid"}, {"white_grid": True}, {"white_grid": 3.0}, {"white_grid": [("a", 0.0, 1.0)]},
    {"white_grid": [(True, 0.0, 1.0)]},
    {"white_grid": [(0.0, 0.0, 1.0)]}, {"white_grid": [(-1.0, 0.0, 1.0)]}, {"white_grid": [(INF, 0.0, 1.0)]},
    {"white_grid": [(NAN, 0.0, 1.0)]},
    {"white_grid": [(1.0, -1e-9, 1.0)]}, {"white_grid": [(1.0, INF, 1.0)]}, {"white_grid": [(1.0, NAN, 1.0)]},
    {"white_grid": [(1.0, 0.0, 0.0)]}, {"white_grid": [(1.0, 0.0, -1.0)]}, {"white_grid": [(1.0, 0.0, INF)]},
    {"white_grid": [(1.0, 0.0, NAN)]}, {"white_grid": [GRID[0], (1.0, 0.0, 0.0)]},
])
def test_validate_rejects(extra):
    with pytest.raises(ValueError, match="dataset 1.*white_grid"):
        D.validate([_ds(), _ds(**extra)])
    with pytest.raises(ValueError, match="dataset 1.*white_grid"):
        D.white_grids([_ds(), _ds(**extra)], D.validate([_ds(), _ds()]))


@pytest.mark.parametrize("extra", [
    {"offset_sigma": 1e-3}, {"offset_sigma": INF}, {"baseline": np.linspace(-1, 1, 7)},
    {"baseline": np.linspace(-1, 1, 7), "baseline_sigma": 2.0},
    {"red_sigma": 1e-3, "red_timescale": 0.1}, {"red_grid": [(1e-3, 0.1, 1.0)]},
    {"red_kernel": "matern32", "red_sigma": 1e-3, "red_timescale": 0.1},
    {"red_kernel": "ou2", "red_sigma": (1e-3, 2e-3), "red_timescale": (0.1, 1.0)},
    {"red_sigma": 1e-3, "red_timescale": 0.1, "red_baseline": np.ones(7)},
    {"red_sigma": 1e-3, "red_timescale": 0.1, "red_baseline": np.ones(7), "red_baseline_sigma": 1e-3},
    {"outlier_frac": 0.05, "outlier_scale": 10.0},
], ids=["offset", "flat-offset", "baseline", "baseline_sigma", "red_sigma", "red_grid", "matern32", "ou2", "red_baseline",
        "red_baseline_sigma", "outliers"])
def test_the_key_stands_alone_or_next_to_a_t0_grid(extra):
    assert D.validate([_ds(**extra)])                                    # (the neighbour alone is a valid dataset)
    with pytest.raises(ValueError, match="dataset 0.*white_grid.*not built"):
        D.validate([_ds(white_grid=GRID, **extra)])
    dicts = [_ds(white_grid=GRID, t0_grid=[(0.0, 1.0), (0.01, 2.0)])]
    sets = D.validate(dicts)
    assert D.white_grids(dicts, sets)[0].shape == (2, 3) and D.t0_grids(dicts, sets)[0].shape == (2, 2)
    assert D.outliers(dicts, sets) == [None] and D.red_baselines(dicts, sets) == [None]


def test_a_folded_light_curve_is_accepted_where_red_grid_refuses_it():
    t = np.linspace(-0.1, 0.1, 7)
    folded = t[[0, 2, 4, 6, 1, 3, 5]]
    dicts = [_ds(time=folded, white_grid=GRID)]
    sets = D.validate(dicts)
    assert np.array_equal(sets[0].time, folded) and D.white_grids(dicts, sets)[0].shape == (2, 3)
    w, lnc = D.white_mix_system(sets[0], D.white_grids(dicts, sets)[0])
    assert w.shape == (2, 7) and np.isfinite(lnc).all()
    with pytest.raises(ValueError, match="dataset 0.*red_grid.*non-decreasing"):
        D.validate([_ds(time=folded, red_grid=[(1e-3, 1e-9, 1.0)])])
    hole = folded.copy()
    hole[2] = np.nan
    assert D.validate([_ds(time=hole, white_grid=GRID)])[0].time.size == 6


def test_white_noise_grid_and_prepare_dataset():
    g = lc.white_noise_grid([1.0, 1.5, 2.0, 3.0], [0.0, 5e-4])
    assert g.shape == (8, 3) and g.dtype == np.float64 and g.flags["C_CONTIGUOUS"]
    assert np.array_equal(g[:, 0], [1.0, 1.0, 1.5, 1.5, 2.0, 2.0, 3.0, 3.0]) and np.array_equal(g[:, 1], [0.0, 5e-4] * 4)
    assert np.allclose(g[:, 2], 1.0 / 8.0, rtol=4 * EPS, atol=0)
    one = lc.white_noise_grid([1.0, 2.0, 4.0])
    assert one.shape == (3, 3) and not one[:, 1].any() and np.array_equal(one[:, 0], [1.0, 2.0, 4.0])
    w = np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]])
    g2 = lc.white_noise_grid([1.0, 2.0], [0.0, 1e-4, 1e-3], w)
    assert np.allclose(g2[:, 2], w.ravel() / 21.0, rtol=4 * EPS, atol=0)
    assert lc.white_noise_grid(1.5, 1e-4).shape == (1, 3)
    for bad in (dict(weights=np.ones((3, 2))), dict(weights=-w), dict(weights=w * np.nan)):
        with pytest.raises(ValueError):
            lc.white_noise_grid([1.0, 2.0], [0.0, 1e-4, 1e-3], **bad)
    with pytest.raises(ValueError):
        lc.white_noise_grid([], [0.0])
    t = np.linspace(-0.4, 0.4, 400)
    y = 1.0 + 1e-3 * np.sin(37.0 * t)
    assert "white_grid" not in lc.prepare_dataset(t, y, n_bins=20, n_sigma=10)
    d = lc.prepare_dataset(t, y, n_bins=20, n_sigma=10, white_grid=g)
    assert d["white_grid"] is g
    sets = D.validate([d])
    assert np.array_equal(D.white_grids([d], sets)[0][:, :2], g[:, :2])
    with pytest.raises(ValueError, match="dataset 0.*white_grid"):
        D.validate([lc.prepare_dataset(t, y, n_bins=20, n_sigma=10, white_grid=lc.white_noise_grid(np.ones(3), np.zeros(3)))])


def test_fused_evaluation_is_refused_before_any_device_call(monkeypatch):
    """target._datasets_pass refuses evaluation='fused' for a dataset with the key once the work units are prepared and
    before they run; the preparation (priors, TRILEGAL) is not what is under test and is stubbed"""
    from test_datasets_api import _target
    from triceratops_amd.triceratops import target
    tg = _target()
    monkeypatch.setattr(target, "_prepare", lambda self, *a, **k: ([], 0))
    dicts = [_ds(), _ds(white_grid=GRID)]
    sets = D.validate(dicts)
    ds = D.Datasets(sets, white_grids=D.white_grids(dicts, sets))
    with pytest.raises(NotImplementedError, match="evaluation='fused' with a white_grid"):
        tg._datasets_pass(ds, 3.0, {}, 0, "fused")


def test_the_switch_is_listed_with_the_others():
    from triceratops_amd import fused
    assert fused.DATASET_WHITE_NOISE is None and "DATASET_WHITE_NOISE" in fused.switches.__doc__
    box = {}
    with fused.switches(DATASET_WHITE_NOISE=box):
        assert fused.DATASET_WHITE_NOISE is box
    assert fused.DATASET_WHITE_NOISE is None
    assert fused._Dataset._fields == ("time", "flux", "inv_var", "exptime", "nsamples", "term", "shift")
    assert fused._Dataset._field_defaults == {"term": None, "shift": None}
    assert fused._WhiteMix._fields == ("w", "lnc")


# ---------------------------------------------------------------------------------------
# the system and the statement
@pytest.mark.parametrize("T", SIZES)
def test_mix_system_shapes_and_normalisation(T):
    d, grid, _ = mix_case(T)
    w, lnc = D.white_mix_system(d, grid)
    J = len(CANDS)
    assert w.shape == (J, T) and w.dtype == np.float64 and w.flags["C_CONTIGUOUS"] and (w > 0).all()
    assert lnc.shape == (J,) and lnc.dtype == np.float64 and np.isfinite(lnc).all() and (lnc <= 0).all()
    total = math.fsum(math.exp(v) for v in lnc.tolist())
    print("T %d: lnc %s, sum exp(lnc) - 1 = %.3g" % (T, lnc, total - 1.0))
    assert abs(total - 1.0) <= 8 * EPS * J
    # the weights enter as their logs: lnc_j - ln pi_j - 0.5 sum ln w_j is one constant
    c = [lnc[j] - math.log(grid[j, 2]) - 0.5 * math.fsum(np.log(w[j]).tolist()) for j in range(J)]
    assert max(c) - min(c) <= 8 * EPS * max(abs(x) for x in c) + 1e-15


@pytest.mark.parametrize("T", SIZES)
def test_the_unit_candidate_and_a_power_of_two_scale_in_bits(T):
    d, _, y = mix_case(T)
    err = d.flux_err
    w, lnc = D.white_mix_system(d, np.array([(1.0, 0.0, 1.0)]))
    assert lnc.tolist() == [0.0]
    assert w[0].tobytes() == (1.0 / (err * err)).tobytes()              # what fused._Dataset.upload forms
    w2, _ = D.white_mix_system(d, np.array([(2.0, 0.0, 0.5), (1.0, 0.0, 0.5), (0.5, 0.0, 0.5)]))
    assert w2[0].tobytes() == (1.0 / ((2.0 * err) * (2.0 * err))).tobytes()
    assert w2[1].tobytes() == w[0].tobytes()
    assert w2[2].tobytes() == (1.0 / ((0.5 * err) * (0.5 * err))).tobytes()
    # J = 1 with lnc = 0: the plain weighted chi^2/2 in float64
    want = 0.5 * np.sum(w[0] * y * y, axis=-1)
    got, cand = _numerics.white_mix_halfchi2(y, w, lnc, return_candidates=True)
    assert got.dtype == np.float64 and got.shape == (4,) and cand.shape == (4, 1)
    assert got.tobytes() == want.tobytes() and cand[:, 0].tobytes() == want.tobytes()
    ld = _numerics.white_mix_halfchi2(y, w, lnc, dtype=LD)
    assert ld.dtype == LD and np.array_equal(ld, LD(0.5) * np.sum(w[0].astype(LD) * y.astype(LD) * y.astype(LD), axis=-1))


@pytest.mark.parametrize("fr", [1.0, 0.5, 0.37, 1.0 / 3.0, 0.0123])
@pytest.mark.parametrize("T", [1, 50, 200])
def test_renorm_scales_the_jitters_and_keeps_the_weights(T, fr):
    d, grid, _ = mix_case(T)
    sets = D.Datasets([d, D.validate([_ds()])[0]], white_grids=[grid, None])
    star = sets.renorm(fr)
    g = star.white_grids[0]
    assert star.white_grids[1] is None and star.has_white_grids and g is not grid
    assert np.array_equal(g[:, 1], grid[:, 1] / fr) and np.array_equal(g[:, [0, 2]], grid[:, [0, 2]])
    assert np.array_equal(sets.white_grids[0], grid)                     # (the caller's grid is left alone)
    w0, c0 = D.white_mix_system(d, grid)
    w1, c1 = D.white_mix_system(star.sets[0], g)
    assert np.allclose(w1, w0 * fr * fr, rtol=8 * EPS, atol=0)
    print("T %d fr %g: max |d lnc| %.3g" % (T, fr, np.max(np.abs(c1 - c0))))
    assert (np.abs(c1 - c0) <= 1e-13).all()
    if fr in (1.0, 0.5):
        assert np.array_equal(w1, w0 * fr * fr)                          # a power of two: no rounding at all
    if fr == 1.0:
        assert np.array_equal(c1, c0)


@pytest.mark.parametrize("level", [0.0, 3.0, 100.0])
@pytest.mark.parametrize("T", SIZES)
def test_statement_is_the_dense_marginal_with_determinants(T, level):
    d, grid, y = mix_case(T, level)
    w, lnc = D.white_mix_system(d, grid)
    got, cand = _numerics.white_mix_halfchi2(y, w, lnc, dtype=LD, return_candidates=True)
    assert got.dtype == LD and got.shape == (4,) and cand.shape == (4, len(CANDS))
    # the dense form from the candidates themselves: -ln sum_j pi_j N(y; 0, diag v_j), less the (T / 2) ln 2 pi the path drops
    err, yl = d.flux_err.astype(LD), y.astype(LD)
    lnn = []
    for k, s, pi_j in grid:
        v = (LD(k) * LD(k)) * (err * err) + LD(s) * LD(s)
        lnn.append(np.log(LD(pi_j)) - LD(0.5) * np.sum(np.log(v)) - LD(0.5) * np.sum(yl * yl / v, axis=-1))
    lnn = np.stack(lnn)                                                # [J][4]
    top = lnn.max(axis=0)
    want = -(top + np.log(np.exp(lnn - top).sum(axis=0)))
    # ln of the normaliser sum_j pi_j prod_t w_j[t]^(1/2), from the same candidates
    raw = np.array([np.log(LD(pi_j)) - LD(0.5) * np.sum(np.log((LD(k) * LD(k)) * (err * err) + LD(s) * LD(s)))
                    for k, s, pi_j in grid])
    lnz = raw.max() + np.log(np.exp(raw - raw.max()).sum())
    value = got - lnz
    bar = 64 * EPS * (1.0 + np.abs(want).astype(np.float64) + float(np.max(np.abs(lnc))))
    diff = np.abs(np.asarray(value - want, dtype=np.float64))
    print("T %d level %g: max |d| %.3g, max |d| / bar %.3g" % (T, level, diff.max(), (diff / bar).max()))
    assert (diff <= bar).all()
    # T >= min_j (h_j - lnc_j) - ln J >= 0 needs no clamp here; the candidates are the plain weighted sums
    assert (got >= 0).all()
    for j in range(len(CANDS)):
        assert np.array_equal(cand[:, j], LD(0.5) * np.sum(w[j].astype(LD) * yl * yl, axis=-1))
    # the float64 statement against the long-double one: the soft minimum is 1-Lipschitz in the h_j
    f64 = _numerics.white_mix_halfchi2(y, w, lnc)
    assert f64.dtype == np.float64
    assert (np.abs(f64 - got.astype(np.float64)) <= 4 * T * EPS * cand.max(axis=1).astype(np.float64)
            + 16 * EPS * (1 + np.abs(f64) + np.abs(lnc).max())).all()


def test_statement_edge_values():
    d, grid, y = mix_case(17, 3.0)
    w, lnc = D.white_mix_system(d, grid)
    y = y.copy()
    y[1, 5] = np.nan
    got = _numerics.white_mix_halfchi2(y, w, lnc)
    assert np.isnan(got[1]) and np.isfinite(got[[0, 2, 3]]).all()
    # a candidate at -800 does not reach the sum, one at -inf is switched off: the other's value, less its lnc
    h = 0.5 * np.sum(w[2] * y[0] * y[0])
    for low in (-800.0, -INF):
        off = np.full(5, low)
        off[2] = 0.0
        assert _numerics.white_mix_halfchi2(y[0], w, off) == h
    # rounding cannot drive the result below 0
    assert _numerics.white_mix_halfchi2(np.zeros(17), w, np.log(np.full(5, 0.2))) >= 0.0
    # permuted candidates: the same value to the rounding of the sum
    p = [3, 0, 4, 1, 2]
    a, b = _numerics.white_mix_halfchi2(y[0], w, lnc), _numerics.white_mix_halfchi2(y[0], w[p], lnc[p])
    assert abs(a - b) <= 16 * EPS * (1 + abs(a) + np.abs(lnc).max())


# ---------------------------------------------------------------------------------------
# the ABI
def _declared():
    text = open(os.path.join(ROOT, "include", "trx_mix.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(trxv_[a-z0-9_]+)\s*\(", text)))


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(ln.split()[-1] for ln in out.splitlines() if " T " in ln)


def test_header_libraries_and_binding_list_the_same_symbols():
    assert _declared() == sorted(_lib.WHITE_SYMBOLS) == ["trxv_chi2_grid_white_mix"]
    assert not set(_lib.WHITE_SYMBOLS) & (set(_lib.ABI_SYMBOLS) | set(_lib.WARP_SYMBOLS) | set(_lib.NOISE_SYMBOLS)
                                          | set(_lib.MIX_SYMBOLS) | set(_lib.SHIFT_SYMBOLS) | set(_lib.ROBUST_SYMBOLS)
                                          | set(_lib.GLS_SYMBOLS) | set(_lib.SS_SYMBOLS) | set(_lib.DEBUG_SYMBOLS))
    assert len(_lib.ABI_SYMBOLS) == 29
    assert callable(_lib.chi2_grid_white_mix) and callable(_lib.white_mix_blocks)
    others = sorted(f for f in os.listdir(os.path.join(ROOT, "include")) if f != "trx_mix.h")
    assert len(others) == 8
    for other in others:
        assert "trxv_" not in open(os.path.join(ROOT, "include", other)).read().lower()
    # the header names no prefix but the core's, the OU filter's and its own two
    text = open(os.path.join(ROOT, "include", "trx_mix.h")).read().lower()
    assert set(re.findall(r"\btrx[a-z]?_", text)) == {"trx_", "trxn_", "trxm_", "trxv_"}
    if not (os.path.exists(_lib.LIB_PATH) and os.path.exists(_lib.TESTING_LIB_PATH)):
        pytest.skip("libtrx.so not built")
    for path in (_lib.LIB_PATH, _lib.TESTING_LIB_PATH):
        assert [s for s in _exports(path) if s.startswith("trxv_")] == _declared()


def test_white_mix_blocks_mirrors_the_launcher():
    # 4 rows a block below the cap; 8 blocks a CU while the staged vectors leave room, fewer where they fill the LDS
    assert _lib.white_mix_blocks(1, 100, 1) == 1 and _lib.white_mix_blocks(5, 100, 8) == 2
    assert _lib.white_mix_blocks(10 ** 6, 100, 8) == 2048                 # 9 x 100 x 8 B: eight blocks a CU
    assert _lib.white_mix_blocks(10 ** 6, 2048, 1) == 256 * 5             # 32 KB a block: five fit 160 KB
    assert _lib.white_mix_blocks(10 ** 6, 454, 8) == 256 * 5              # 9 x 454 x 8 B = 32688 B
    assert _lib.white_mix_blocks(10 ** 6, 455, 8) == 2048                 # past the stage limit: no LDS
    assert _lib.white_mix_blocks(10 ** 6, 1364, 2) == 256 * 5 and _lib.white_mix_blocks(10 ** 6, 1365, 2) == 2048
    assert _lib.white_mix_blocks(10 ** 6, 2049, 1) == 2048


def test_argument_checks_need_no_gpu():
    """every refusal comes before anything touches a device: the pointers below are not device memory"""
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libtrx.so not built")
    L = _lib.lib()
    v = [np.zeros(16) for _ in range(7)]
    f, g, o, w, s, c, k = (x.ctypes.data for x in v)
    call = L.trxv_chi2_grid_white_mix
    ERR_ARG = 1
    assert call(None, g, 2, 2, s, INF, 0, o, w, 2, c, k, None) == ERR_ARG             # NULL flux
    assert call(f, None, 2, 2, s, INF, 0, o, w, 2, c, k, None) == ERR_ARG             # NULL grid
    assert call(f, g, 2, 2, s, INF, 0, None, w, 2, c, k, None) == ERR_ARG             # NULL out
    assert call(f, g, 2, 2, s, INF, 0, o, None, 2, c, k, None) == ERR_ARG             # NULL weights
    assert call(f, g, 2, 2, s, INF, 0, o, w, 2, None, k, None) == ERR_ARG             # NULL lnc
    assert b"null pointer" in L.trx_last_error()
    assert call(f, g, 2, -1, s, INF, 0, o, w, 2, c, k, None) == ERR_ARG               # n < 0
    assert call(f, g, 0, 2, s, INF, 0, o, w, 2, c, k, None) == ERR_ARG                # n_time < 1
    assert call(f, g, -3, 0, s, INF, 0, o, w, 2, c, k, None) == ERR_ARG               # ... also with no rows
    assert b"n_time" in L.trx_last_error()
    for n_cand in (0, -1, 9, 64):
        assert call(f, g, 2, 2, s, INF, 0, o, w, n_cand, c, k, None) == ERR_ARG       # n_cand outside 1 ... 8
        assert call(f, g, 2, 0, s, INF, 0, o, w, n_cand, c, k, None) == ERR_ARG       # ... also with no rows
    assert b"n_cand" in L.trx_last_error()
    for bad in (NAN, INF):
        for at in (0, 2):
            lnc = np.zeros(3)
            lnc[at] = bad
            assert call(f, g, 2, 2, s, INF, 0, o, w, 3, lnc.ctypes.data, k, None) == ERR_ARG
            assert call(f, g, 2, 0, s, INF, 0, o, w, 3, lnc.ctypes.data, None, None) == ERR_ARG
    assert b"lnc" in L.trx_last_error()
    # n == 0: nothing to launch -- for every n_cand, without secdepth and cand_out, -inf in lnc allowed
    lnc = np.array([0.0, -INF, -3.0, 0.0, 0.0, 0.0, 0.0, 0.0])
    for n_cand in range(1, 9):
        assert call(f, g, 2, 0, None, INF, 0, o, w, n_cand, lnc.ctypes.data, None, None) == 0
    assert not any(x.any() for x in v)
