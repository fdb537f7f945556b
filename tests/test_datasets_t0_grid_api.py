"""A transit-time shift grid per dataset on the host: the `t0_grid` key and datasets.t0_grids, its way
through Datasets and renorm, lightcurve.t0_shift_grid, _numerics.t0_mix_halfchi2 against the long-double log-sum-exp, and the
ABI entry of the soft minimum (include/trx_shift.h).  No GPU: every check here ends before the first device call.

Bars, none of them chosen from results:
  normalised weights: |sum - 1| <= 4 eps (J <= 8 quotients of one rounding each, summed by math.fsum);
  t0_mix_halfchi2 in float64 against -logsumexp(ln pi - h) in long double: |d T| <= 16 eps (1 + |T| + max_j |ln pi_j|) --
        a_j and m - a_j carry eps |a| each, at most 8 exponentials and one log a couple of ulp each, the soft minimum is
        1-Lipschitz in a; 16 is twice that count (the bar of tests/test_gpu_softmin_rows.py).
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
GRID = [(-0.01, 1.0), (0.0, 2.0), (0.0125, 1.0)]


def _ds(**keys):
    t = np.linspace(-0.1, 0.1, 7)
    return dict({"time": t, "flux": 1.0 - 1e-3 * (np.abs(t) < 0.04), "flux_err": 1e-3}, **keys)


# ---------------------------------------------------------------------------------------
# the key
@pytest.mark.parametrize("extra", [{}, {"offset_sigma": 1e-3}, {"red_sigma": 1e-3, "red_timescale": 0.1},
                                   {"baseline": np.linspace(-1, 1, 7), "baseline_sigma": 2.0},
                                   {"red_grid": [(1e-3, 0.1, 1.0), (2e-3, INF, 1.0)]}])
def test_validate_accepts_the_key_and_leaves_every_dataset_as_it_is(extra):
    a = D.validate([_ds(**extra), _ds()])
    b = D.validate([_ds(t0_grid=GRID, **extra), _ds(t0_grid=None)])
    assert D.Dataset._fields == ("time", "flux", "flux_err", "exptime", "nsamples", "offset_sigma", "baseline",
                                 "baseline_sigma", "red_grid", "red_sigma", "red_timescale")
    for x, y in zip(a, b):
        for name, u, v in zip(x._fields, x, y):
            assert (np.array_equal(u, v) if isinstance(u, np.ndarray) else u == v), name
    with pytest.raises(ValueError, match="unknown key"):
        D.validate([_ds(t0_grids=GRID)])


@pytest.mark.parametrize("grid", [GRID, np.array(GRID), [(0.5, 3)], [(0.001 * k, 1.0) for k in range(8)],
                                  [(np.float32(0.25), 1e-300), (-0.25, 1e-300)], [(-1e300, 1), (1e300, 1e10)]])
def test_t0_grids_returns_normalised_contiguous_arrays(grid):
    dicts = [_ds(), _ds(t0_grid=grid), _ds(t0_grid=None)]
    sets = D.validate(dicts)
    got = D.t0_grids(dicts, sets)
    assert isinstance(got, list) and len(got) == 3 and got[0] is None and got[2] is None
    g, want = got[1], np.array(grid, dtype=np.float64)
    assert g.dtype == np.float64 and g.shape == want.shape and g.flags["C_CONTIGUOUS"]
    assert np.array_equal(g[:, 0], want[:, 0])
    assert abs(math.fsum(g[:, 1]) - 1.0) <= 4 * EPS and np.allclose(g[:, 1], want[:, 1] / want[:, 1].sum(), rtol=4 * EPS)
    if want.shape[0] == 1:
        assert g[0, 1] == 1.0                                     # (ln 1 = 0: the one-node grid is exact)
    assert D.MAX_T0_NODES == 8
    with pytest.raises(ValueError):
        D.t0_grids(dicts[:2], sets)


@pytest.mark.parametrize("bad", [
    [], [(0.001 * k, 1.0) for k in range(9)],                                               # 1 ... 8 rows
    [(0.1,)], [(0.1, 1.0, 1.0)], (0.1, 1.0), 3.0, [[(0.1, 1.0)]],                           # the shape
    [(NAN, 1.0)], [(INF, 1.0)], [(-INF, 1.0)], [(0.1, NAN)], [(0.1, INF)], [(0.0, 1.0), (0.1, NAN)],
    [(0.1, 1.0), (0.1, 2.0)], [(0.0, 1.0), (0.1, 1.0), (-0.0, 1.0)],                        # repeated shifts
    [(0.1, 0.0)], [(0.1, -1.0)], [(0.0, 1.0), (0.1, 0.0)],                                  # a weight <= 0
    True, [(0.0, True)], [(False, 1.0)], np.array([[True, True]]),                          # a bool
    "grid", b"grid", [("0.1", 1.0)], [(0.1, "1")], [("a", 1.0)],                            # a string
])
def test_t0_grids_rejects(bad):
    dicts = [_ds(), _ds(t0_grid=bad)]
    sets = D.validate(dicts)                                      # (validate allows the key and does not read it)
    with pytest.raises(ValueError, match=r"dataset 1.*t0_grid"):
        D.t0_grids(dicts, sets)


@pytest.mark.parametrize("fr", [1.0, 0.37, 0.0123])
def test_datasets_stores_the_grids_and_renorm_carries_them_through(fr):
    dicts = [_ds(offset_sigma=1e-3), _ds(t0_grid=GRID)]
    sets = D.validate(dicts)
    grids = D.t0_grids(dicts, sets)
    plain, ds = D.Datasets(sets), D.Datasets(sets, grids)
    assert plain.t0_grids == (None, None) and not plain.has_t0_grids
    assert ds.has_t0_grids and ds.t0_grids[0] is None and ds.t0_grids[1] is grids[1]
    star = ds.renorm(fr)
    assert star.has_t0_grids and star.t0_grids[0] is None and np.array_equal(star.t0_grids[1], grids[1])
    assert not plain.renorm(fr).has_t0_grids
    # times are not touched, sigma_bar and the sets are what they are without the key
    for a, b in zip(star.sets, plain.renorm(fr).sets):
        assert np.array_equal(a.time, b.time) and np.array_equal(a.flux, b.flux) and np.array_equal(a.flux_err, b.flux_err)
    assert star.sigma_ref == plain.renorm(fr).sigma_ref and ds.sigma_ref == plain.sigma_ref
    with pytest.raises(ValueError):
        D.Datasets(sets, grids[:1])


@pytest.mark.parametrize("n,span", [(1, 3.0), (3, 1.0), (5, 3.0), (7, 2.5)])
def test_t0_shift_grid(n, span):
    sigma = 0.0123
    g = lc.t0_shift_grid(sigma, n=n, span=span)
    assert g.shape == (n, 2) and g.dtype == np.float64 and g.flags["C_CONTIGUOUS"]
    assert g[n // 2, 0] == 0.0 and np.array_equal(g[:, 0], -g[::-1, 0]) and np.array_equal(g[:, 1], g[::-1, 1])
    assert abs(math.fsum(g[:, 1]) - 1.0) <= 4 * EPS and (g[:, 1] > 0).all()
    if n > 1:
        assert np.all(np.diff(g[:, 0]) > 0) and np.allclose(np.diff(g[:, 0]), 2 * span * sigma / (n - 1), rtol=1e-14)
        assert np.isclose(g[-1, 0], span * sigma, rtol=1e-15)
        assert np.allclose(g[:, 1] / g[n // 2, 1], np.exp(-0.5 * (g[:, 0] / sigma) ** 2), rtol=1e-14)
    dicts = [_ds(t0_grid=g)]
    assert np.array_equal(D.t0_grids(dicts, D.validate(dicts))[0][:, 0], g[:, 0])


def test_t0_shift_grid_defaults_and_refusals_and_prepare_dataset():
    assert lc.t0_shift_grid(0.01).shape == (5, 2) and np.isclose(lc.t0_shift_grid(0.01)[0, 0], -0.03)
    for kw in ({"n": 4}, {"n": 0}, {"n": -1}, {"span": 0.0}, {"span": INF}):
        with pytest.raises(ValueError):
            lc.t0_shift_grid(0.01, **kw)
    for sigma in (0.0, -1.0, INF, NAN):
        with pytest.raises(ValueError):
            lc.t0_shift_grid(sigma)
    rng = np.random.default_rng(1)
    t = np.sort(rng.uniform(-0.5, 0.5, 4000))
    f = 1.0 + 1e-3 * rng.normal(size=t.size)
    plain = lc.prepare_dataset(t, f)
    assert "t0_grid" not in plain
    g = lc.t0_shift_grid(0.01)
    keyed = lc.prepare_dataset(t, f, t0_grid=g)
    assert keyed["t0_grid"] is g and set(keyed) == set(plain) | {"t0_grid"}
    assert all(np.array_equal(np.asarray(plain[k], dtype=object), np.asarray(keyed[k], dtype=object)) for k in plain)
    assert D.t0_grids([keyed], D.validate([keyed]))[0].shape == (5, 2)


# ---------------------------------------------------------------------------------------
# the numpy statement
def _reference(h, lnpi):
    """-logsumexp_j(lnpi_j - h_j) in long double, the maximum taken out; +inf where every term is -inf"""
    h = np.asarray(h, dtype=np.longdouble)
    x = np.asarray(lnpi, dtype=np.longdouble)[:, None] - h
    top = np.max(x, axis=0)
    with np.errstate(invalid="ignore", divide="ignore"):
        out = -(top + np.log(np.sum(np.exp(x - top), axis=0)))
    return np.where(np.isneginf(top), np.longdouble(INF), out)


@pytest.mark.parametrize("J", [1, 2, 3, 8])
@pytest.mark.parametrize("scale", [0.0, 50.0, 5000.0])
def test_statement_against_the_long_double_log_sum_exp(J, scale):
    rng = np.random.default_rng(100 * J + int(scale))
    n = 257
    h = np.abs(scale + 3.0 * rng.normal(size=(J, n))) if scale else np.zeros((J, n))
    w = rng.uniform(0.1, 1.0, J)
    for lnpi in (np.log(w / w.sum()), h[:, 0] - h[:, 0].min() - 1.0):       # the grid's own; the nodes balanced at row 0
        got = _numerics.t0_mix_halfchi2(h, lnpi)
        assert got.dtype == np.float64 and got.shape == (n,)
        want = np.maximum(_reference(h, lnpi), 0.0)
        bar = 16 * EPS * (1.0 + np.abs(want) + np.abs(lnpi).max())
        err = np.abs(got - want)
        print("J %d, h ~ %g: max |d T| / bar %.3g" % (J, scale, float(np.max(err / bar))))
        assert (err <= bar).all() and (got >= 0).all()
        # any dtype: the long-double run of the statement itself is its own reference to long-double rounding
        ld = _numerics.t0_mix_halfchi2(h.astype(np.longdouble), lnpi)
        assert ld.dtype == np.longdouble and (np.abs(ld - want) <= bar).all()


def test_statement_edge_values():
    rng = np.random.default_rng(5)
    h = rng.uniform(1.0, 40.0, (3, 9))
    # J = 1 at ln pi = 0: the input's bits, +inf and NaN included
    one = h[:1].copy()
    one[0, 3], one[0, 4] = INF, NAN
    got = _numerics.t0_mix_halfchi2(one, [0.0])
    assert got.tobytes() == one[0].tobytes()
    # an all-+inf row is +inf, a row with a NaN is NaN, a row with one +inf node drops that node
    e = h.copy()
    e[:, 1] = INF
    e[1, 2] = NAN
    e[2, 5] = INF
    lnpi = np.log([0.2, 0.3, 0.5])
    got = _numerics.t0_mix_halfchi2(e, lnpi)
    assert got[1] == INF and np.isnan(got[2]) and np.isfinite(np.delete(got, [1, 2])).all()
    want5 = np.maximum(_reference(e[:2, 5:6], lnpi[:2]), 0.0)[0]
    assert abs(got[5] - want5) <= 16 * EPS * (1.0 + abs(want5) + np.abs(lnpi).max())
    # a node at -inf is switched off; the others at -800 do not reach the sum: that node's bits
    off = _numerics.t0_mix_halfchi2(h, [-INF, 0.0, -INF])
    assert off.tobytes() == h[1].tobytes()
    far = _numerics.t0_mix_halfchi2(h, [-800.0, -800.0, 0.0])
    assert far.tobytes() == h[2].tobytes()
    # rounding below 0 is stored as 0
    assert _numerics.t0_mix_halfchi2(np.zeros((2, 4)), [math.log(0.5), math.log(0.5)]).tobytes() == np.zeros(4).tobytes()
    assert (_numerics.t0_mix_halfchi2(np.zeros((3, 4)), np.log([0.1, 0.2, 0.7])) >= 0).all()
    # a vector of J values is one row
    assert _numerics.t0_mix_halfchi2(h[:, 0], lnpi) == _numerics.t0_mix_halfchi2(h, lnpi)[0]


# ---------------------------------------------------------------------------------------
# the ABI
HEADERS = ("trx.h", "trx_warp.h", "trx_noise.h", "trx_mix.h", "trx_debug.h")


def _declared():
    text = open(os.path.join(ROOT, "include", "trx_shift.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(trxt_[a-z0-9_]+)\s*\(", text)))


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(ln.split()[-1] for ln in out.splitlines() if " T " in ln)


def test_header_libraries_and_binding_list_the_same_symbol():
    assert _declared() == sorted(_lib.SHIFT_SYMBOLS) == ["trxt_softmin_rows"]
    assert not set(_lib.SHIFT_SYMBOLS) & (set(_lib.ABI_SYMBOLS) | set(_lib.WARP_SYMBOLS) | set(_lib.NOISE_SYMBOLS)
                                          | set(_lib.MIX_SYMBOLS) | set(_lib.DEBUG_SYMBOLS))
    assert callable(_lib.softmin_rows)
    others = sorted(f for f in os.listdir(os.path.join(ROOT, "include")) if f != "trx_shift.h")
    assert set(HEADERS) <= set(others)
    for other in others:
        assert "trxt_" not in open(os.path.join(ROOT, "include", other)).read().lower()
    import __graft_entry__ as g
    g.build()
    for path in (_lib.LIB_PATH, _lib.TESTING_LIB_PATH):
        assert [s for s in _exports(path) if s.startswith("trxt_")] == _declared()
    for name in ("trx_softmin.hpp", "trx_shift.h"):
        assert any(os.path.basename(d) == name for d in g.DEPS), name


def test_argument_checks_need_no_gpu():
    """every refusal comes before anything touches a device: the pointers below are not device memory"""
    import __graft_entry__ as g
    g.build()
    L = _lib.lib()
    v = [np.zeros(64) for _ in range(3)]
    c, o, k = (x.ctypes.data for x in v)
    call = L.trxt_softmin_rows
    ERR_ARG = 1
    assert call(None, 8, 8, 2, k, 0, o, None) == ERR_ARG                    # NULL cand
    assert call(c, 8, 8, 2, None, 0, o, None) == ERR_ARG                    # NULL lnc
    assert call(c, 8, 8, 2, k, 0, None, None) == ERR_ARG                    # NULL out
    assert call(None, 8, 0, 2, k, 0, o, None) == ERR_ARG                    # ... also with no rows
    assert b"null pointer" in L.trx_last_error()
    assert call(c, 8, -1, 2, k, 0, o, None) == ERR_ARG                      # n < 0
    assert call(c, -2, -1, 2, k, 0, o, None) == ERR_ARG
    assert call(c, 7, 8, 2, k, 0, o, None) == ERR_ARG                       # stride < n
    assert call(c, -1, 0, 2, k, 0, o, None) == ERR_ARG                      # ... also with no rows
    assert b"stride" in L.trx_last_error()
    for n_cand in (0, -1, 9, 64):
        assert call(c, 8, 8, n_cand, k, 0, o, None) == ERR_ARG              # n_cand outside 1 ... 8
        assert call(c, 8, 0, n_cand, k, 0, o, None) == ERR_ARG              # ... also with no rows
    assert b"n_cand" in L.trx_last_error()
    for bad in (NAN, INF):
        for at in (0, 2):
            lnc = np.zeros(3)
            lnc[at] = bad
            for accumulate in (0, 1):
                assert call(c, 8, 8, 3, lnc.ctypes.data, accumulate, o, None) == ERR_ARG
            assert call(c, 8, 0, 3, lnc.ctypes.data, 0, o, None) == ERR_ARG
    assert b"lnc" in L.trx_last_error()
    # n == 0: nothing to launch -- for every n_cand, any stride >= 0, -inf in lnc allowed
    lnc = np.array([0.0, -INF, -3.0, 0.0, 0.0, 0.0, 0.0, 0.0])
    for n_cand in range(1, 9):
        for stride in (0, 5):
            assert call(c, stride, 0, n_cand, lnc.ctypes.data, 1, o, None) == 0
    assert not any(x.any() for x in v)
