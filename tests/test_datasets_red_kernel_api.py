"""The kernel of a dataset's correlated noise on the host: the `red_kernel` key next to `red_sigma` /
`red_timescale` -- "matern32": one Matern-3/2 term, "ou2": two exponential terms --, its renormalisation,
datasets.ss2_system + _numerics.ss2_halfchi2 against the dense statement 0.5 y^T solve(K, y) and ln det K, the limits of
the two models, and the ABI entry of the reduction (include/trx_ss.h).  No GPU: every check here ends before the first
device call.

Bars, none of them chosen from results:
  dense solve: |d h| <= 1e-9 x 0.5 sum y^2 / sigma^2 + 1e-12 while cond(K) <= 1e5 (asserted), the bar of
        tests/test_datasets_red_noise_api.py: the solve's own error is cond(K) x eps ~ 2e-11 of y^T K^-1 y <= sum y^2 / sigma^2;
  ln det K = sum_n ln S_n (math.fsum): 4 T cond(K) eps + 2 (log2 T + 1) eps sum_n |ln S_n| + 1e-12 -- a backward-stable
        factorisation moves each of the T eigenvalues by at most cond(K) eps relative, and slogdet adds up T logarithms of
        the size of ln S_n (about 13 each here, all of one sign: the sum's own spacing is the second term's size);
  ou2 with tau_1 = tau_2 against ou_system with s = hypot(s_1, s_2), both statements in long double: the row bar of
        tests/test_gpu_chi2_ou.py (row_bar); the tables themselves to 1e-13 relative (A[0][1] = 0 exactly: the second
        state does not enter);
  ou2 with s_2 = 1e-9 sigma against ou_system(s_1, tau_1): 0 <= h(K) - h(K + s_2^2 E) = 0.5 s_2^2 v^T E v', v = K^-1 y,
        |.| <= 0.5 s_2^2 lambda_max(E) |K^-1 y|^2 <= 0.5 s_2^2 T sum y^2 / sigma^2 / min sigma^2 (E has unit diagonal;
        K >= diag(sigma^2)) -- Cauchy-Schwarz, the form of the vanishing term in tests/test_gpu_datasets_red_noise.py with
        T / min sigma^2 >= S0 in place of S0 because K^-1 is not diagonal here -- plus row_bar for the two recurrences;
  matern32 with l = 1e-6 cadence: A = g = 0 and omega = 1 / (sigma^2 + s^2) exactly (exp underflows), h to 1e-13 relative;
  renorm: A and g to 1e-13 relative to the largest entry (the roundings of red_sigma / fr and flux_err / fr through the
        T-step recursion), omega x fr^2 likewise.
"""
import math
import os
import re
import subprocess

import numpy as np
import pytest

from test_datasets_red_noise_api import SIGMA, row_bar
from triceratops_amd import _lib, _numerics
from triceratops_amd import datasets as D
from triceratops_amd import lightcurve as lc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
LD = np.longdouble
SIZES = [1, 2, 50, 200]
RATIOS = [0.3, 3.0, 10.0]                    # s / sigma
SCALES = [0.5, 5.0, 50.0]                    # time scale / cadence
KERNELS = ["matern32", "ou2"]


def _ds(**extra):
    d = {"time": np.linspace(-0.1, 0.1, 7), "flux": np.full(7, 0.999), "flux_err": np.linspace(1e-3, 2e-3, 7)}
    d.update(extra)
    return d


def keys(kernel, ratio, scale):
    """the noise keys of a case: ou2 takes a second term of half the amplitude and seven times the time scale"""
    if kernel == "matern32":
        return {"red_kernel": kernel, "red_sigma": ratio * SIGMA, "red_timescale": scale}
    return {"red_kernel": kernel, "red_sigma": (ratio * SIGMA, 0.5 * ratio * SIGMA), "red_timescale": (scale, 7.0 * scale)}


def light_curve(T, seed=0):
    """T irregular sorted stamps (mean cadence 1), errors varying 3x around SIGMA, [4][T] residuals of the errors' size"""
    rng = np.random.default_rng(1000 * T + seed)
    t = np.cumsum(rng.uniform(0.3, 1.7, T))
    err = SIGMA * rng.uniform(0.6, 1.8, T)
    return t, err, err * rng.normal(0.0, 1.0, (4, T))


def case(T, kernel, ratio, scale):
    t, err, y = light_curve(T)
    d = D.validate([dict(time=t, flux=np.ones(T), flux_err=err, **keys(kernel, ratio, scale))])[0]
    return d, y


def dense(d):
    dt = np.abs(d.time[:, None] - d.time[None, :])
    K = np.diag(d.flux_err ** 2)
    if d.red_kernel == "matern32":
        x = np.sqrt(3.0) * dt / d.red_timescale
        return K + d.red_sigma ** 2 * (1.0 + x) * np.exp(-x)
    for s, tau in zip(d.red_sigma, d.red_timescale):
        K = K + s ** 2 * np.exp(-dt / tau)
    return K


# ---------------------------------------------------------------------------------------
# validation
def test_validate_accepts_the_kernels():
    got = D.validate([_ds(), _ds(red_kernel="matern32", red_sigma=2e-3, red_timescale=np.float32(0.5)),
                      _ds(red_kernel="ou2", red_sigma=[2e-3, 1e-3], red_timescale=np.array([0.05, 0.5]))])
    assert got[0].red_kernel is None and type(got[0]) is D.Dataset
    assert got[1].red_kernel == "matern32" and isinstance(got[1], D.Dataset)
    assert isinstance(got[1].red_sigma, float) and got[1].red_sigma == 2e-3 and got[1].red_timescale == 0.5
    assert got[2].red_kernel == "ou2" and isinstance(got[2], D.Dataset)
    for v, want in ((got[2].red_sigma, [2e-3, 1e-3]), (got[2].red_timescale, [0.05, 0.5])):
        assert v.dtype == np.float64 and v.shape == (2,) and v.flags.c_contiguous and v.tolist() == want
    assert D.Datasets(got).has_red_noise and not D.Datasets(got[:1]).has_red_noise
    for d in got[1:]:
        A, g, omega = D.ss2_system(d)
        assert A.shape == (7, 2, 2) and g.shape == (7, 2) and omega.shape == (7,)
        assert A.dtype == g.dtype == omega.dtype == np.float64 and (omega > 0).all()
        assert not A[-1].any() and not g[-1].any()                      # the last stamp predicts nothing
    with pytest.raises(ValueError, match="red_kernel"):
        D.ss2_system(got[0])


@pytest.mark.parametrize("kernel", [None, "ou"])
def test_the_ou_kernel_is_the_dataset_of_no_key(kernel):
    for extra in ({}, {"red_sigma": 2e-3, "red_timescale": INF}):
        a = D.validate([_ds(**extra)])[0]
        b = D.validate([_ds(red_kernel=kernel, **extra)])[0]
        assert type(a) is type(b) is D.Dataset and b.red_kernel is None and a._fields == b._fields
        for name, u, v in zip(a._fields, a, b):
            assert type(u) is type(v) and np.array_equal(u, v), name
        if extra:
            for u, v in zip(D.ou_system(a), D.ou_system(b)):
                assert u.tobytes() == v.tobytes()


M32 = {"red_kernel": "matern32", "red_sigma": 1e-3, "red_timescale": 0.1}
OU2 = {"red_kernel": "ou2", "red_sigma": (1e-3, 2e-3), "red_timescale": (0.1, 1.0)}


@pytest.mark.parametrize("extra", [
    {"red_kernel": "matern52", "red_sigma": 1e-3, "red_timescale": 0.1},                     # not a kernel
    {"red_kernel": "OU", "red_sigma": 1e-3, "red_timescale": 0.1}, {"red_kernel": "", "red_sigma": 1e-3, "red_timescale": 0.1},
    {"red_kernel": 2, "red_sigma": 1e-3, "red_timescale": 0.1}, {"red_kernel": True, "red_sigma": 1e-3, "red_timescale": 0.1},
    {"red_kernel": ["ou2"], "red_sigma": 1e-3, "red_timescale": 0.1},
    {"red_kernel": "matern32"}, {"red_kernel": "ou2"},                                       # no terms
    {"red_kernel": "matern32", "red_sigma": 1e-3}, {"red_kernel": "ou2", "red_timescale": (0.1, 1.0)},
    dict(M32, red_sigma=(1e-3, 2e-3)), dict(M32, red_timescale=(0.1, 1.0)), dict(M32, red_sigma=[1e-3]),   # shapes
    dict(OU2, red_sigma=1e-3), dict(OU2, red_timescale=0.1), dict(OU2, red_sigma=(1e-3, 2e-3, 3e-3)),
    dict(OU2, red_timescale=[[0.1, 1.0]]), dict(OU2, red_sigma=(1e-3,)),
    dict(M32, red_sigma=0.0), dict(M32, red_sigma=-1e-3), dict(M32, red_sigma=float("nan")), dict(M32, red_sigma=INF),
    dict(M32, red_sigma="1e-3"), dict(M32, red_sigma=True),
    dict(M32, red_timescale=0.0), dict(M32, red_timescale=-1.0), dict(M32, red_timescale=float("nan")),
    dict(M32, red_timescale=INF),                                                            # inf: the OU key's business
    dict(OU2, red_sigma=(1e-3, 0.0)), dict(OU2, red_sigma=(float("nan"), 1e-3)), dict(OU2, red_sigma=(1e-3, INF)),
    dict(OU2, red_sigma=(1e-3, "x")), dict(OU2, red_sigma=(True, 1e-3)),
    dict(OU2, red_timescale=(0.1, INF)), dict(OU2, red_timescale=(0.0, 1.0)), dict(OU2, red_timescale=(0.1, float("nan"))),
    dict(OU2, red_timescale=(-0.1, 1.0)),
])
def test_validate_rejects(extra):
    with pytest.raises(ValueError, match="dataset 1.*red_"):
        D.validate([_ds(), _ds(**extra)])


@pytest.mark.parametrize("base", [M32, OU2], ids=KERNELS)
@pytest.mark.parametrize("extra", [
    {"offset_sigma": 1e-3}, {"offset_sigma": INF}, {"baseline": np.linspace(-1, 1, 7)},
    {"red_grid": [(1e-3, 0.1, 1.0)]}, {"red_baseline": np.ones(7)}, {"red_baseline": np.ones(7), "red_baseline_sigma": 1e-3},
    {"outlier_frac": 0.05, "outlier_scale": 10.0},
], ids=["offset", "flat-offset", "baseline", "red_grid", "red_baseline", "red_baseline_sigma", "outliers"])
def test_the_new_kernels_stand_next_to_a_t0_grid_only(base, extra):
    with pytest.raises(ValueError, match="dataset 0.*red_kernel.*not built"):
        D.validate([_ds(**base, **extra)])
    dicts = [_ds(t0_grid=[(0.0, 1.0), (0.01, 2.0)], **base)]
    sets = D.validate(dicts)
    assert sets[0].red_kernel == base["red_kernel"] and D.t0_grids(dicts, sets)[0].shape == (2, 2)
    assert D.outliers(dicts, sets) == [None] and D.red_baselines(dicts, sets) == [None]


@pytest.mark.parametrize("base", [M32, OU2], ids=KERNELS)
def test_validate_wants_time_order(base):
    t = np.linspace(-0.1, 0.1, 7)
    with pytest.raises(ValueError, match="dataset 0.*non-decreasing"):
        D.validate([_ds(time=t[[0, 2, 4, 6, 1, 3, 5]], **base)])
    same = np.array([0.0, 0.0, 0.1, 0.1, 0.2, 0.3, 0.3])                                      # equal stamps are in order
    d = D.validate([_ds(time=same, **base)])[0]
    A, g, omega = D.ss2_system(d)
    assert np.isfinite(A).all() and np.isfinite(g).all() and (omega > 0).all()


def test_prepare_dataset_passes_the_key_through():
    t = np.linspace(-0.4, 0.4, 400)
    y = 1.0 + 1e-3 * np.sin(37.0 * t)
    assert "red_kernel" not in lc.prepare_dataset(t, y, n_bins=20, n_sigma=10, red_sigma=2e-4, red_timescale=0.05)
    d = lc.prepare_dataset(t, y, n_bins=20, n_sigma=10, red_sigma=2e-4, red_timescale=0.05, red_kernel="matern32")
    assert d["red_kernel"] == "matern32" and D.validate([d])[0].red_kernel == "matern32"
    d = lc.prepare_dataset(t, y, n_bins=20, n_sigma=10, red_sigma=(2e-4, 1e-4), red_timescale=(0.05, 0.5), red_kernel="ou2")
    got = D.validate([d])[0]
    assert got.red_kernel == "ou2" and got.red_sigma.tolist() == [2e-4, 1e-4] and got.red_timescale.tolist() == [0.05, 0.5]
    d = lc.prepare_dataset(t, y, n_bins=20, n_sigma=10, red_sigma=2e-4, red_timescale=0.05, red_kernel="ou")
    assert d["red_kernel"] == "ou" and type(D.validate([d])[0]) is D.Dataset


def test_fused_evaluation_is_refused_before_any_device_call(monkeypatch):
    """target._datasets_pass refuses evaluation='fused' for a dataset with correlated noise of any kernel once the work
    units are prepared and before they run; the preparation (priors, TRILEGAL) is not what is under test and is stubbed"""
    from test_datasets_api import _target
    from triceratops_amd.triceratops import target
    tg = _target()
    monkeypatch.setattr(target, "_prepare", lambda self, *a, **k: ([], 0))
    for base in (M32, OU2):
        ds = D.Datasets(D.validate([_ds(), _ds(**base)]))
        with pytest.raises(NotImplementedError, match="evaluation='fused' with a red_sigma"):
            tg._datasets_pass(ds, 3.0, {}, 0, "fused")


# ---------------------------------------------------------------------------------------
# the recurrence
@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("ratio", RATIOS)
@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("T", SIZES)
def test_recurrence_is_the_dense_quadratic_form_and_determinant(T, kernel, ratio, scale):
    d, y = case(T, kernel, ratio, scale)
    A, g, omega = D.ss2_system(d)
    K = dense(d)
    cond = np.linalg.cond(K)
    assert cond <= 1e5, cond
    want = 0.5 * np.einsum("rt,tr->r", y, np.linalg.solve(K, y.T))
    got = _numerics.ss2_halfchi2(y, A, g, omega)
    bar = 1e-9 * 0.5 * np.sum(y * y / d.flux_err ** 2, axis=1) + 1e-12
    lndet, want_lndet = -math.fsum(np.log(omega).tolist()), float(np.linalg.slogdet(K)[1])
    eps = np.finfo(np.float64).eps
    bar_det = 4.0 * T * cond * eps + 2.0 * (np.log2(T) + 1.0) * eps * float(np.sum(np.abs(np.log(omega)))) + 1e-12
    print("T %d %s s %g sigma scale %g: cond(K) %.3g, max |d h| / bar %.3g (relative %.3g), |d ln det| / bar %.3g"
          % (T, kernel, ratio, scale, cond, np.max(np.abs(got - want) / bar), np.max(np.abs(got - want) / want),
             abs(lndet - want_lndet) / bar_det))
    assert got.shape == (4,) and got.dtype == np.float64 and (np.abs(got - want) <= bar).all()
    assert abs(lndet - want_lndet) <= bar_det
    ld = _numerics.ss2_halfchi2(y, A, g, omega, dtype=LD)
    assert ld.dtype == LD and (np.abs(np.asarray(ld - got, dtype=np.float64)) <= bar).all()
    # a NaN stays a NaN, in its row alone
    bad = y.copy()
    bad[1, T // 2] = np.nan
    h = _numerics.ss2_halfchi2(bad, A, g, omega)
    assert np.isnan(h[1]) and np.array_equal(h[[0, 2, 3]], got[[0, 2, 3]])


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("ratio", RATIOS)
@pytest.mark.parametrize("T", SIZES)
def test_two_equal_time_scales_are_one_ou_term(T, ratio, scale):
    t, err, y = light_curve(T)
    s1, s2 = ratio * SIGMA, 0.5 * ratio * SIGMA
    base = dict(time=t, flux=np.ones(T), flux_err=err)
    two = D.validate([dict(base, red_kernel="ou2", red_sigma=(s1, s2), red_timescale=(scale, scale))])[0]
    one = D.validate([dict(base, red_sigma=float(np.hypot(s1, s2)), red_timescale=scale)])[0]
    A, g, omega = D.ss2_system(two)
    alpha, beta, w = D.ou_system(one)
    assert not A[:, 0, 1].any()                                    # the second state does not enter the prediction
    assert np.allclose(A[:-1, 0, 0], alpha[1:], rtol=1e-13, atol=0) and np.allclose(g[:-1, 0], beta[1:], rtol=1e-13, atol=0)
    assert np.allclose(omega, w, rtol=1e-13, atol=0)
    got = _numerics.ss2_halfchi2(y, A, g, omega, dtype=LD)
    want = _numerics.ou_halfchi2(y, alpha, beta, w, dtype=LD)
    assert (np.abs(np.asarray(got - want, dtype=np.float64)) <= row_bar(y, alpha, w)).all()


@pytest.mark.parametrize("scale", SCALES)
@pytest.mark.parametrize("ratio", RATIOS)
@pytest.mark.parametrize("T", SIZES)
def test_a_vanishing_second_term_is_one_ou_term(T, ratio, scale):
    t, err, y = light_curve(T)
    y = y + 2.0 * SIGMA
    s2 = 1e-9 * SIGMA
    base = dict(time=t, flux=np.ones(T), flux_err=err)
    two = D.validate([dict(base, red_kernel="ou2", red_sigma=(ratio * SIGMA, s2), red_timescale=(scale, 11.0 * scale))])[0]
    one = D.validate([dict(base, red_sigma=ratio * SIGMA, red_timescale=scale)])[0]
    alpha, beta, w = D.ou_system(one)
    got = _numerics.ss2_halfchi2(y, *D.ss2_system(two), dtype=LD)
    want = _numerics.ou_halfchi2(y, alpha, beta, w, dtype=LD)
    bound = 0.5 * s2 ** 2 * T / np.min(err) ** 2 * np.sum(y * y / err ** 2, axis=1) + row_bar(y, alpha, w)
    assert (np.abs(np.asarray(got - want, dtype=np.float64)) <= bound).all()


@pytest.mark.parametrize("T", SIZES)
def test_a_short_matern_length_is_white_noise(T):
    t, err, y = light_curve(T)
    s = 3.0 * SIGMA
    d = D.validate([dict(time=t, flux=np.ones(T), flux_err=err, red_kernel="matern32", red_sigma=s, red_timescale=1e-6)])[0]
    A, g, omega = D.ss2_system(d)
    assert not A.any() and not g.any()
    assert np.array_equal(omega, 1.0 / (s ** 2 + err ** 2))
    want = 0.5 * np.sum(y * y / (err ** 2 + s ** 2), axis=1)
    assert (np.abs(_numerics.ss2_halfchi2(y, A, g, omega) - want) <= 1e-13 * want).all()


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("fr", [1.0, 0.5, 0.37, 1.0 / 3.0, 0.0123])
def test_renorm_scales_every_amplitude_with_the_errors(fr, kernel):
    d, _ = case(50, kernel, 3.0, 5.0)
    star = D.Datasets([d, D.validate([_ds()])[0]]).renorm(fr)
    got = star.sets[0]
    assert type(got) is type(d) and got.red_kernel == kernel and star.sets[1].red_kernel is None
    assert np.array_equal(got.red_sigma, np.asarray(d.red_sigma) / fr) and np.array_equal(got.red_timescale, d.red_timescale)
    A0, g0, w0 = D.ss2_system(d)
    A1, g1, w1 = D.ss2_system(got)
    assert np.allclose(A1, A0, rtol=0, atol=1e-13 * np.abs(A0).max()) and np.allclose(g1, g0, rtol=0, atol=1e-13 * np.abs(g0).max())
    assert np.allclose(w1, w0 * fr * fr, rtol=1e-13, atol=0)
    if fr in (1.0, 0.5):
        assert np.array_equal(A1, A0) and np.array_equal(g1, g0)            # a power of two: no rounding at all


# ---------------------------------------------------------------------------------------
# the ABI
def _declared():
    text = open(os.path.join(ROOT, "include", "trx_ss.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(trxs_[a-z0-9_]+)\s*\(", text)))


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(ln.split()[-1] for ln in out.splitlines() if " T " in ln)


def test_header_libraries_and_binding_list_the_same_symbols():
    assert _declared() == sorted(_lib.SS_SYMBOLS) == ["trxs_chi2_grid_ss2"]
    assert not set(_lib.SS_SYMBOLS) & (set(_lib.ABI_SYMBOLS) | set(_lib.WARP_SYMBOLS) | set(_lib.NOISE_SYMBOLS)
                                       | set(_lib.MIX_SYMBOLS) | set(_lib.SHIFT_SYMBOLS) | set(_lib.ROBUST_SYMBOLS)
                                       | set(_lib.GLS_SYMBOLS) | set(_lib.DEBUG_SYMBOLS))
    assert len(_lib.ABI_SYMBOLS) == 29
    assert callable(_lib.chi2_grid_ss2)
    others = sorted(f for f in os.listdir(os.path.join(ROOT, "include")) if f != "trx_ss.h")
    assert len(others) == 8
    for other in others:
        assert "trxs_" not in open(os.path.join(ROOT, "include", other)).read().lower()
    if not (os.path.exists(_lib.LIB_PATH) and os.path.exists(_lib.TESTING_LIB_PATH)):
        pytest.skip("libtrx.so not built")
    for path in (_lib.LIB_PATH, _lib.TESTING_LIB_PATH):
        assert [s for s in _exports(path) if s.startswith("trxs_")] == _declared()


def test_argument_checks_need_no_gpu():
    """every refusal comes before anything touches a device: the pointers below are not device memory"""
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libtrx.so not built")
    L = _lib.lib()
    v = [np.zeros(8) for _ in range(7)]
    f, g, o, a, b, w, s = (x.ctypes.data for x in v)
    call = L.trxs_chi2_grid_ss2
    ERR_ARG = 1
    assert call(None, g, 2, 2, s, INF, 0, o, a, b, w, None) == ERR_ARG              # NULL flux
    assert call(f, None, 2, 2, s, INF, 0, o, a, b, w, None) == ERR_ARG              # NULL grid
    assert call(f, g, 2, 2, s, INF, 0, None, a, b, w, None) == ERR_ARG              # NULL out
    assert call(f, g, 2, 2, s, INF, 0, o, None, b, w, None) == ERR_ARG              # NULL A
    assert call(f, g, 2, 2, s, INF, 0, o, a, None, w, None) == ERR_ARG              # NULL g
    assert call(f, g, 2, 2, s, INF, 0, o, a, b, None, None) == ERR_ARG              # NULL omega
    assert b"null pointer" in L.trx_last_error()
    assert call(f, g, 2, -1, s, INF, 0, o, a, b, w, None) == ERR_ARG                # n < 0
    assert call(f, g, 0, 2, s, INF, 0, o, a, b, w, None) == ERR_ARG                 # n_time < 1
    assert call(f, g, -3, 0, s, INF, 0, o, a, b, w, None) == ERR_ARG                # ... also with no rows
    assert b"n_time" in L.trx_last_error()
    assert call(f, g, 2, 0, None, INF, 0, o, a, b, w, None) == 0                    # n == 0: nothing to launch
    assert not any(x.any() for x in v)
