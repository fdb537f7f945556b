"""A grid of red-noise candidates per dataset on the host: the `red_grid` key, its renormalisation,
datasets.ou_mix_system + _numerics.ou_mix_halfchi2 against the dense statement of the marginal over the candidates
(determinants included), and the ABI entry of the reduction (include/trx_mix.h).  No GPU: every check here ends before
the first device call.

Bars, none of them chosen from results:
  dense statement: |d T| <= 1e-9 x 0.5 sum y^2 / sigma^2 + 1e-12 + 1e-11 T while cond(K_j) <= 1e5 (asserted): the dense
        bar of tests/test_datasets_red_noise_api.py for the quadratic forms (the soft minimum is 1-Lipschitz in them), plus
        the error of slogdet, T x cond x eps;
  sum_j exp(lnc_j) = 1: |logsumexp(lnc)| <= 1e-15 J (math.fsum of J terms of one rounding each);
  renorm: lnc to 2e-15 T + 4 eps max_j sum_n |ln omega_j[n]| (every ln omega_n moves by 2 ln fr, the same for every
        candidate; what is left is the rounding of the logs and of omega itself), alpha and beta to 1e-15 relative.
"""
import math
import os
import re
import subprocess

import numpy as np
import pytest

from test_datasets_red_noise_api import PAIRS, SIGMA, SIZES, _ds, case
from triceratops_amd import _lib, _numerics
from triceratops_amd import datasets as D
from triceratops_amd import lightcurve as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
EPS = np.finfo(np.float64).eps
GRID = [(2e-3, 0.05, 1.0), (1e-3, INF, 3.0)]
CANDS = PAIRS + [(1.0, INF)]                               # (s_r / sigma, tau / cadence): five candidates
WEIGHTS = [0.1, 0.3, 0.05, 0.35, 0.2]


def mix_case(T, seed=0):
    """case() of tests/test_datasets_red_noise_api.py with the five candidates as its red_grid: (Dataset, y [4][T])"""
    d, y = case(T, 1.0, 1.0, seed)
    grid = [(r * SIGMA, tau, w) for (r, tau), w in zip(CANDS, WEIGHTS)]
    d = D.validate([{"time": d.time, "flux": d.flux, "flux_err": d.flux_err, "red_grid": grid}])[0]
    return d, y


def _logsumexp(v):
    top = max(v)
    return top + math.log(math.fsum(math.exp(x - top) for x in v))


# ---------------------------------------------------------------------------------------
# validation
@pytest.mark.parametrize("grid", [GRID, np.array(GRID), [(1e-3, 0.1, 5)], [GRID[0]] * 8, [GRID[0], GRID[0]],
                                  [(np.float32(1e-3), 1, 1e-300), (2e-3, 2, 1e-300)]])
def test_validate_accepts_a_grid(grid):
    got = D.validate([_ds(), _ds(red_grid=grid)])
    assert got[0].red_grid is None
    g = got[1].red_grid
    want = np.array(grid, dtype=np.float64)
    assert g.dtype == np.float64 and g.shape == want.shape and g.flags["C_CONTIGUOUS"]
    assert np.array_equal(g[:, :2], want[:, :2])
    assert abs(math.fsum(g[:, 2]) - 1.0) <= 4 * EPS and np.allclose(g[:, 2], want[:, 2] / want[:, 2].sum(), rtol=4 * EPS)
    assert got[1].red_sigma is None and got[1].red_timescale is None
    assert not D.Datasets(got[:1]).has_red_noise and D.Datasets(got).has_red_noise
    assert D.MAX_RED_CANDIDATES == 8


def test_the_last_fields_stay_and_the_five_argument_construction_works():
    assert D.Dataset._fields[-2:] == ("red_sigma", "red_timescale")
    assert D.Dataset._fields[-3] == "red_grid"
    t = np.arange(3.0)
    d = D.Dataset(t, t, t, 0.1, 2)
    assert d.red_grid is None and d.red_sigma is None and d.offset_sigma is None and d.nsamples == 2


def test_validate_without_the_key_is_unchanged():
    for extra in ({}, {"offset_sigma": 1e-3}, {"red_sigma": 1e-3, "red_timescale": 0.1},
                  {"baseline": np.linspace(-1, 1, 7), "baseline_sigma": 2.0}):
        a = D.validate([_ds(**extra)])[0]
        b = D.validate([_ds(red_grid=None, **extra)])[0]
        assert a.red_grid is None and b.red_grid is None
        for name, x, y in zip(a._fields, a, b):
            assert (np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y), name
        # what the fields were before the key, in their order
        assert [n for n in a._fields if n != "red_grid"] == [
            "time", "flux", "flux_err", "exptime", "nsamples", "offset_sigma", "baseline", "baseline_sigma", "red_sigma",
            "red_timescale"]
        assert a.red_sigma == extra.get("red_sigma") and a.offset_sigma == extra.get("offset_sigma")


@pytest.mark.parametrize("extra", [
    {"red_grid": []}, {"red_grid": [GRID[0]] * 9},                                          # 1 ... 8 candidates
    {"red_grid": [(1e-3, 0.1)]}, {"red_grid": [(1e-3, 0.1, 1.0, 1.0)]}, {"red_grid": (1e-3, 0.1, 1.0)},
    {"red_grid": "grid"}, {"red_grid": True}, {"red_grid": 3.0}, {"red_grid": [("a", 0.1, 1.0)]},
    {"red_grid": [(0.0, 0.1, 1.0)]}, {"red_grid": [(-1e-3, 0.1, 1.0)]}, {"red_grid": [(INF, 0.1, 1.0)]},
    {"red_grid": [(float("nan"), 0.1, 1.0)]},
    {"red_grid": [(1e-3, 0.0, 1.0)]}, {"red_grid": [(1e-3, -1.0, 1.0)]}, {"red_grid": [(1e-3, float("nan"), 1.0)]},
    {"red_grid": [(1e-3, -INF, 1.0)]},
    {"red_grid": [(1e-3, 0.1, 0.0)]}, {"red_grid": [(1e-3, 0.1, -1.0)]}, {"red_grid": [(1e-3, 0.1, INF)]},
    {"red_grid": [(1e-3, 0.1, float("nan"))]}, {"red_grid": [GRID[0], (1e-3, 0.1, 0.0)]},
    {"red_grid": GRID, "red_sigma": 1e-3, "red_timescale": 0.1},                            # not built together
    {"red_grid": GRID, "offset_sigma": 1e-3}, {"red_grid": GRID, "offset_sigma": INF},
    {"red_grid": GRID, "baseline": np.linspace(-1, 1, 7)},
])
def test_validate_rejects(extra):
    with pytest.raises(ValueError, match="dataset 1.*red_grid"):
        D.validate([_ds(), _ds(**extra)])


def test_validate_wants_time_order():
    t = np.linspace(-0.1, 0.1, 7)
    folded = t[[0, 2, 4, 6, 1, 3, 5]]
    with pytest.raises(ValueError, match="dataset 0.*red_grid.*non-decreasing"):
        D.validate([_ds(time=folded, red_grid=GRID)])
    same = np.array([0.0, 0.0, 0.1, 0.1, 0.2, 0.3, 0.3])
    assert D.validate([_ds(time=same, red_grid=GRID)])[0].time.size == 7
    hole = t.copy()
    hole[2] = np.nan
    assert D.validate([_ds(time=hole, red_grid=GRID)])[0].time.size == 6


def test_red_noise_grid_and_prepare_dataset():
    g = lc.red_noise_grid([1e-3, 2e-3], [0.01, 0.1, INF])
    assert g.shape == (6, 3) and g.dtype == np.float64
    assert np.array_equal(g[:, 0], [1e-3] * 3 + [2e-3] * 3) and np.array_equal(g[:, 1], [0.01, 0.1, INF] * 2)
    assert np.allclose(g[:, 2], 1.0 / 6.0, rtol=4 * EPS, atol=0)
    w = np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]])
    g = lc.red_noise_grid([1e-3, 2e-3], [0.01, 0.1, INF], w)
    assert np.allclose(g[:, 2], w.ravel() / 21.0, rtol=4 * EPS, atol=0)
    assert lc.red_noise_grid(1e-3, 0.1).shape == (1, 3)
    for bad in (dict(weights=np.ones((3, 2))), dict(weights=-w), dict(weights=w * np.nan)):
        with pytest.raises(ValueError):
            lc.red_noise_grid([1e-3, 2e-3], [0.01, 0.1, INF], **bad)
    with pytest.raises(ValueError):
        lc.red_noise_grid([], [0.1])
    t = np.linspace(-0.4, 0.4, 400)
    y = 1.0 + 1e-3 * np.sin(37.0 * t)
    assert "red_grid" not in lc.prepare_dataset(t, y, n_bins=20, n_sigma=10)
    d = lc.prepare_dataset(t, y, n_bins=20, n_sigma=10, red_grid=g)
    assert d["red_grid"] is g and "red_sigma" not in d
    assert np.array_equal(D.validate([d])[0].red_grid[:, :2], g[:, :2])
    with pytest.raises(ValueError, match="dataset 0.*red_grid"):
        D.validate([lc.prepare_dataset(t, y, n_bins=20, n_sigma=10, red_grid=lc.red_noise_grid(np.full(3, 1e-3), np.ones(3)))])


# ---------------------------------------------------------------------------------------
# the system and the statement
@pytest.mark.parametrize("T", SIZES)
def test_mix_system_shapes_and_normalisation(T):
    d, _ = mix_case(T)
    alpha, beta, omega, lnc = D.ou_mix_system(d)
    J = len(CANDS)
    for v in (alpha, beta, omega):
        assert v.shape == (J, T) and v.dtype == np.float64 and v.flags["C_CONTIGUOUS"]
    assert lnc.shape == (J,) and lnc.dtype == np.float64 and np.isfinite(lnc).all() and (lnc <= 0).all()
    print("T %d: lnc %s, logsumexp %.3g" % (T, lnc, _logsumexp(lnc.tolist())))
    assert abs(_logsumexp(lnc.tolist())) <= 1e-15 * J
    for j, (s_r, tau, weight) in enumerate(d.red_grid):
        one = D.ou_system(d._replace(red_grid=None, red_sigma=s_r, red_timescale=tau))
        assert all(np.array_equal(a[j], b) for a, b in zip((alpha, beta, omega), one))
    # the weights enter as their logs: lnc_j - ln pi_j - 0.5 sum ln omega_j is one constant
    c = [lnc[j] - math.log(d.red_grid[j, 2]) - 0.5 * math.fsum(np.log(omega[j])) for j in range(J)]
    assert max(c) - min(c) <= 8 * EPS * max(abs(x) for x in c) + 1e-15


@pytest.mark.parametrize("T", SIZES)
def test_one_candidate_is_ou_halfchi2_in_bits(T):
    d, y = case(T, *PAIRS[1])
    one = D.validate([{"time": d.time, "flux": d.flux, "flux_err": d.flux_err,
                       "red_grid": [(d.red_sigma, d.red_timescale, 7.0)]}])[0]
    alpha, beta, omega, lnc = D.ou_mix_system(one)
    assert lnc.tolist() == [0.0] and one.red_grid[0, 2] == 1.0
    abw = D.ou_system(d)
    assert all(np.array_equal(a[0], b) for a, b in zip((alpha, beta, omega), abw))
    for dtype in (np.float64, np.longdouble):
        want = _numerics.ou_halfchi2(y, *abw, dtype=dtype)
        got, cand = _numerics.ou_mix_halfchi2(y, alpha, beta, omega, lnc, dtype=dtype, return_candidates=True)
        assert got.dtype == dtype and got.shape == (4,) and cand.shape == (4, 1)
        # (equal values of one dtype and sign: the same bits; a long double's padding bytes are not its value)
        assert np.array_equal(got, want) and np.array_equal(cand[:, 0], want) and not np.signbit(got).any()
        assert np.array_equal(_numerics.ou_mix_halfchi2(y, alpha, beta, omega, lnc, dtype=dtype), want)
        if dtype is np.float64:
            assert got.tobytes() == want.tobytes() and cand[:, 0].tobytes() == want.tobytes()


@pytest.mark.parametrize("T", SIZES)
def test_statement_is_the_dense_marginal_with_determinants(T):
    d, y = mix_case(T)
    alpha, beta, omega, lnc = D.ou_mix_system(d)
    dt = np.abs(d.time[:, None] - d.time[None, :])
    lnw, quad = [], []
    for j, (s_r, tau, weight) in enumerate(d.red_grid):
        K = np.diag(d.flux_err ** 2) + s_r ** 2 * np.exp(-dt / tau)
        cond = np.linalg.cond(K)
        assert cond <= 1e5, (j, cond)
        sign, logdet = np.linalg.slogdet(K)
        assert sign == 1.0
        # ln det K_j = -sum ln omega_j
        assert abs(logdet + math.fsum(np.log(omega[j]))) <= 1e-11 * T + 1e-12
        lnw.append(math.log(weight) - 0.5 * logdet)
        quad.append(0.5 * np.einsum("rt,tr->r", y, np.linalg.solve(K, y.T)))
    lnw, quad = np.array(lnw), np.array(quad)                       # [J], [J][4]
    x = lnw[:, None] - quad
    top = x.max(axis=0)
    want = -(top + np.log(np.exp(x - top).sum(axis=0))) + _logsumexp(lnw.tolist())
    got = _numerics.ou_mix_halfchi2(y, alpha, beta, omega, lnc)
    bar = 1e-9 * 0.5 * np.sum(y * y / d.flux_err ** 2, axis=1) + 1e-12 + 1e-11 * T
    print("T %d: max |d T| %.3g, max |d T| / bar %.3g" % (T, np.max(np.abs(got - want)), np.max(np.abs(got - want) / bar)))
    assert got.shape == (4,) and got.dtype == np.float64 and (np.abs(got - want) <= bar).all()
    # T >= min_j h_j - max lnc >= 0, and the candidates come back as ou_halfchi2 gives them
    got2, cand = _numerics.ou_mix_halfchi2(y, alpha, beta, omega, lnc, return_candidates=True)
    assert np.array_equal(got2, got) and (got >= 0).all() and (got >= cand.min(axis=1) - 4 * EPS * got).all()
    for j in range(len(CANDS)):
        assert np.array_equal(cand[:, j], _numerics.ou_halfchi2(y, alpha[j], beta[j], omega[j]))
    # the float64 statement against the long-double one: the rounding of exp / log and of the recurrences
    ld = _numerics.ou_mix_halfchi2(y, alpha, beta, omega, lnc, dtype=np.longdouble)
    assert ld.dtype == np.longdouble
    print("    float64 against long double: max |d T| %.3g" % float(np.max(np.abs(ld - got))))


def test_statement_edge_values():
    d, y = mix_case(17)
    alpha, beta, omega, lnc = D.ou_mix_system(d)
    y = y.copy()
    y[1, 5] = np.nan
    got = _numerics.ou_mix_halfchi2(y, alpha, beta, omega, lnc)
    assert np.isnan(got[1]) and np.isfinite(got[[0, 2, 3]]).all()
    # a candidate at -800 does not reach the sum: the other's value, less its lnc
    h = _numerics.ou_halfchi2(y[0], alpha[2], beta[2], omega[2])
    off = np.full(5, -800.0)
    off[2] = 0.0
    assert _numerics.ou_mix_halfchi2(y[0], alpha, beta, omega, off) == h


@pytest.mark.parametrize("fr", [1.0, 0.5, 0.37, 1.0 / 3.0, 0.0123])
def test_renorm_scales_the_amplitudes_and_keeps_the_weights(fr):
    T = 65
    d, _ = mix_case(T)
    sets = D.Datasets([d, D.validate([_ds()])[0]])
    star = sets.renorm(fr)
    g = star.sets[0].red_grid
    assert np.array_equal(g[:, 0], d.red_grid[:, 0] / fr) and np.array_equal(g[:, 1:], d.red_grid[:, 1:])
    assert star.sets[1].red_grid is None and star.has_red_noise and g is not d.red_grid
    a0, b0, w0, c0 = D.ou_mix_system(d)
    a1, b1, w1, c1 = D.ou_mix_system(star.sets[0])
    assert np.allclose(a1, a0, rtol=1e-15, atol=0) and np.allclose(b1, b0, rtol=1e-15, atol=0)
    assert np.allclose(w1, w0 * fr * fr, rtol=1e-15, atol=0)
    bar = 2e-15 * T + 4 * EPS * max(np.abs(np.log(w)).sum(axis=1).max() for w in (w0, w1))
    print("fr %g: max |d lnc| %.3g (bar %.3g)" % (fr, np.max(np.abs(c1 - c0)), bar))
    assert (np.abs(c1 - c0) <= bar).all()
    if fr == 1.0:
        assert np.array_equal(c1, c0)


# ---------------------------------------------------------------------------------------
# the ABI
def _declared():
    text = open(os.path.join(ROOT, "include", "trx_mix.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(trxm_[a-z0-9_]+)\s*\(", text)))


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(ln.split()[-1] for ln in out.splitlines() if " T " in ln)


def test_header_libraries_and_binding_list_the_same_symbols():
    assert _declared() == sorted(_lib.MIX_SYMBOLS) == ["trxm_chi2_grid_ou_mix"]
    assert not set(_lib.MIX_SYMBOLS) & (set(_lib.ABI_SYMBOLS) | set(_lib.WARP_SYMBOLS) | set(_lib.NOISE_SYMBOLS)
                                        | set(_lib.DEBUG_SYMBOLS))
    assert callable(_lib.chi2_grid_ou_mix)
    for other in ("trx.h", "trx_warp.h", "trx_noise.h", "trx_debug.h"):
        assert "trxm_" not in open(os.path.join(ROOT, "include", other)).read()
    if not (os.path.exists(_lib.LIB_PATH) and os.path.exists(_lib.TESTING_LIB_PATH)):
        pytest.skip("libtrx.so not built")
    for path in (_lib.LIB_PATH, _lib.TESTING_LIB_PATH):
        assert [s for s in _exports(path) if s.startswith("trxm_")] == _declared()


def test_argument_checks_need_no_gpu():
    """every refusal comes before anything touches a device: the pointers below are not device memory"""
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libtrx.so not built")
    L = _lib.lib()
    v = [np.zeros(16) for _ in range(9)]
    f, g, o, a, b, w, s, c, k = (x.ctypes.data for x in v)
    call = L.trxm_chi2_grid_ou_mix
    ERR_ARG = 1
    assert call(None, g, 2, 2, s, INF, 0, o, a, b, w, 2, c, k, None) == ERR_ARG             # NULL flux
    assert call(f, None, 2, 2, s, INF, 0, o, a, b, w, 2, c, k, None) == ERR_ARG             # NULL grid
    assert call(f, g, 2, 2, s, INF, 0, None, a, b, w, 2, c, k, None) == ERR_ARG             # NULL out
    assert call(f, g, 2, 2, s, INF, 0, o, None, b, w, 2, c, k, None) == ERR_ARG             # NULL alpha
    assert call(f, g, 2, 2, s, INF, 0, o, a, None, w, 2, c, k, None) == ERR_ARG             # NULL beta
    assert call(f, g, 2, 2, s, INF, 0, o, a, b, None, 2, c, k, None) == ERR_ARG             # NULL omega
    assert call(f, g, 2, 2, s, INF, 0, o, a, b, w, 2, None, k, None) == ERR_ARG             # NULL lnc
    assert b"null pointer" in L.trx_last_error()
    assert call(f, g, 2, -1, s, INF, 0, o, a, b, w, 2, c, k, None) == ERR_ARG               # n < 0
    assert call(f, g, 0, 2, s, INF, 0, o, a, b, w, 2, c, k, None) == ERR_ARG                # n_time < 1
    assert call(f, g, -3, 0, s, INF, 0, o, a, b, w, 2, c, k, None) == ERR_ARG               # ... also with no rows
    for n_cand in (0, -1, 9, 64):
        assert call(f, g, 2, 2, s, INF, 0, o, a, b, w, n_cand, c, k, None) == ERR_ARG       # n_cand outside 1 ... 8
        assert call(f, g, 2, 0, s, INF, 0, o, a, b, w, n_cand, c, k, None) == ERR_ARG       # ... also with no rows
    assert b"n_cand" in L.trx_last_error()
    for bad in (float("nan"), INF):
        for at in (0, 2):
            lnc = np.zeros(3)
            lnc[at] = bad
            assert call(f, g, 2, 2, s, INF, 0, o, a, b, w, 3, lnc.ctypes.data, k, None) == ERR_ARG
            assert call(f, g, 2, 0, s, INF, 0, o, a, b, w, 3, lnc.ctypes.data, None, None) == ERR_ARG
    assert b"lnc" in L.trx_last_error()
    # n == 0: nothing to launch -- for every n_cand, without secdepth and cand_out, -inf in lnc allowed
    lnc = np.array([0.0, -INF, -3.0, 0.0, 0.0, 0.0, 0.0, 0.0])
    for n_cand in range(1, 9):
        assert call(f, g, 2, 0, None, INF, 0, o, a, b, w, n_cand, lnc.ctypes.data, None, None) == 0
    assert not any(x.any() for x in v)
