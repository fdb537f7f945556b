"""Posterior-predictive light-curve bands: trx_grid_quantiles against np.quantile, and target.fit_bands against the
CPU oracle's curves of the same posterior samples.

Tolerances.  The order statistics of a column are exact whatever finds them, so against np.quantile on the SAME grid the
only freedom is whether the interpolation's multiply-add is contracted: one rounding of a value <= 1, at most one ulp
(2.2e-16), doubled for margin: 4.5e-16 absolute; where the two order statistics are equal the result is that value,
bit for bit.  End to end the curves come from two implementations of the light-curve model, which agree to 5e-13 in
flux; a quantile is an order statistic or a convex combination of two, so the bands agree to the
same bound."""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
ATOL = 4.5e-16
FLUX_TOL = 5e-13
Q = (0.0, 0.16, 0.5, 0.84, 1.0, 1.0 / 3.0)


def make_grid(n_rows, n_cols, rng, depth=0.01):
    """model-curve-like columns: two thirds of every column exactly 1.0 (out of transit), the rest 1 - depth * rand"""
    g = 1.0 - depth * rng.random((n_rows, n_cols))
    for c in range(n_cols):
        g[rng.permutation(n_rows)[:(2 * n_rows) // 3], c] = 1.0
    return g


def integer_q(n_rows):
    """a level q for which (n_rows - 1) q is an integer in floating point: an interior one where there is one"""
    for k in range(max(n_rows - 2, 0), 0, -1):
        q = k / (n_rows - 1)
        if (n_rows - 1) * q == k:
            return q
    return 1.0


def quantiles(grid, q, rows=None, scale=None, dev=None):
    """(the device result, the grid as downloaded)"""
    import torch
    from triceratops_amd import _lib
    g_d = _lib.dev(grid) if dev is None else dev
    rows_d = None if rows is None else torch.as_tensor(np.asarray(rows, dtype=np.int64)).to(g_d.device)
    scale_d = None if scale is None else _lib.dev(scale)
    out = _lib.grid_quantiles(g_d, q, rows_d=rows_d, scale_d=scale_d)
    return out.cpu().numpy(), g_d.cpu().numpy()


def check_definition(got, values, q):
    """got against np.quantile(values, q, axis=0): ATOL, and bitwise where the two order statistics are equal"""
    want = np.quantile(values, q, axis=0)
    assert got.shape == want.shape
    err = float(np.abs(got - want).max())
    print("n_rows = %d, n_cols = %d: max |device - np.quantile| = %.3g" % (values.shape[0], values.shape[1], err))
    assert err <= ATOL
    s = np.sort(values, axis=0)
    n = values.shape[0]
    ties = 0
    for i, qq in enumerate(q):
        lo = int(np.floor((n - 1) * qq))
        hi = min(lo + 1, n - 1)
        same = s[lo] == s[hi]
        ties += int(same.sum())
        assert got[i][same].tobytes() == s[lo][same].tobytes()
    return ties


@pytest.mark.parametrize("n_cols", [1, 5, 64, 77])
@pytest.mark.parametrize("n_rows", [1, 2, 3, 63, 64, 65, 255, 257, 1000, 4096])
def test_quantiles_match_the_definition(n_rows, n_cols):
    from triceratops_amd import _lib
    _lib.require_gpu()
    rng = np.random.default_rng(7919 * n_rows + n_cols)
    q = Q + (integer_q(n_rows),)
    assert float((n_rows - 1) * q[-1]).is_integer()
    got, grid = quantiles(make_grid(n_rows, n_cols, rng), q)
    ties = check_definition(got, grid, q)
    assert ties >= n_cols                       # (the median of a column that is 1.0 in two thirds of its rows)
    assert np.all(got[4] == grid.max(axis=0)) and np.all(got[0] == grid.min(axis=0))


def test_a_nan_poisons_its_column_only():
    rng = np.random.default_rng(11)
    grid = make_grid(100, 7, rng)
    clean, _ = quantiles(grid, Q)
    grid[17, 3] = np.nan
    got, _ = quantiles(grid, Q)
    assert np.all(np.isnan(got[:, 3]))
    keep = [0, 1, 2, 4, 5, 6]
    assert got[:, keep].tobytes() == clean[:, keep].tobytes()
    assert np.array_equal(np.isnan(got), np.isnan(np.quantile(grid, Q, axis=0)))


@pytest.mark.parametrize("n_grid_rows,n_rows,n_cols", [(300, 500, 13), (10, 4096, 5), (257, 1, 3), (64, 65, 9)])
def test_gather_and_scale(n_grid_rows, n_rows, n_cols):
    rng = np.random.default_rng(n_grid_rows + n_rows)
    grid = make_grid(n_grid_rows, n_cols, rng)
    rows = rng.integers(0, n_grid_rows, n_rows)             # repeats, out of order
    s = 1.0 - rng.random(n_rows)                            # (0, 1]
    q = Q + (integer_q(n_rows),)
    got, g = quantiles(grid, q, rows=rows, scale=s)
    check_definition(got, 1 - s[:, None] * (1 - g[rows]), q)
    got, g = quantiles(grid, q, rows=rows)
    check_definition(got, g[rows], q)
    if n_rows <= n_grid_rows:
        got, g = quantiles(grid[:n_rows], q, scale=s)
        check_definition(got, 1 - s[:, None] * (1 - g), q)


def test_the_result_repeats_bit_for_bit_on_any_stream():
    import torch
    from triceratops_amd import _lib
    rng = np.random.default_rng(5)
    grid = make_grid(1000, 77, rng)
    rows = rng.integers(0, 1000, 700)
    s = 1.0 - rng.random(700)
    g_d = _lib.dev(grid)
    first, _ = quantiles(grid, Q, rows=rows, scale=s, dev=g_d)
    again, _ = quantiles(grid, Q, rows=rows, scale=s, dev=g_d)
    assert first.tobytes() == again.tobytes()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        other, _ = quantiles(grid, Q, rows=rows, scale=s, dev=g_d)
    side.synchronize()
    assert first.tobytes() == other.tobytes()


def test_argument_errors():
    """through ctypes, on the production library"""
    import torch
    from triceratops_amd import _lib
    _lib.require_gpu()
    L = _lib.lib()
    assert L.trx_testing is False
    g = torch.ones((8, 4), dtype=torch.float64, device="cuda")
    out = torch.zeros((17, 4), dtype=torch.float64, device="cuda")

    def call(n_rows, q):
        qa = (ctypes.c_double * len(q))(*q)
        return L.trx_grid_quantiles(g.data_ptr(), 8, 4, None, None, n_rows, qa, len(q), out.data_ptr(), None)

    TRX_ERR_ARG = 1
    assert call(8, [0.5]) == 0
    assert call(0, [0.5]) == TRX_ERR_ARG
    assert call(_lib.POST_MAX_ROWS + 1, [0.5]) == TRX_ERR_ARG
    assert call(8, [0.5] * 17) == TRX_ERR_ARG
    assert call(8, [1.5]) == TRX_ERR_ARG
    assert call(8, [float("nan")]) == TRX_ERR_ARG
    assert call(8, [-0.25]) == TRX_ERR_ARG
    qa = (ctypes.c_double * 1)(0.5)
    assert L.trx_grid_quantiles(None, 8, 4, None, None, 8, qa, 1, out.data_ptr(), None) == TRX_ERR_ARG
    assert L.trx_grid_quantiles(g.data_ptr(), 8, 4, None, None, 8, None, 1, out.data_ptr(), None) == TRX_ERR_ARG
    assert L.trx_grid_quantiles(g.data_ptr(), 8, 4, None, None, 8, qa, 1, None, None) == TRX_ERR_ARG
    assert L.trx_grid_quantiles(g.data_ptr(), 8, 0, None, None, 8, qa, 1, out.data_ptr(), None) == TRX_ERR_ARG
    torch.cuda.synchronize()
    assert np.all(out.cpu().numpy()[1:] == 0) and np.all(out.cpu().numpy()[0] == 1)    # only the good call wrote


# ---------------------------------------------------------------------------------------------------------------------
# end to end: TOI-465.01, the 15-scenario case of tests/test_gpu_posterior.py
N_DRAWS, M_ROWS, N_MODEL, N_MIX = 20000, 64, 50, 256
BAND_Q = (0.16, 0.5, 0.84)


def _gold():
    from helpers import gold
    return gold("toi465_calc_probs.npz")


def _target():
    import pandas as pd
    from triceratops_amd.triceratops import target
    G = _gold()
    cols = ("ID", "Tmag", "Jmag", "Hmag", "Kmag", "ra", "dec", "mass", "rad", "Teff", "plx", "fluxratio", "tdepth")
    st = pd.DataFrame({c: G["real_stars_%s" % c] for c in cols})
    st["ID"] = st["ID"].astype(np.int64)
    return target(270380593, np.array([4]), stars=st, trilegal_fname=os.path.join(GOLD, "trilegal_synth.csv"))


@pytest.fixture(scope="module")
def case():
    """the target after calc_posteriors, its fit_curves before and after fit_bands, and the bands: computed once"""
    import torch
    import triceratops_amd
    from triceratops_amd import _lib
    _lib.require_gpu()
    G = _gold()
    data = (G["time"], G["flux"], float(G["sigma"][0]))
    tg = _target()
    triceratops_amd.set_sampling("device")
    try:
        torch.manual_seed(465)
        tg.calc_posteriors(*data, float(G["P_orb"][0]), n_samples=M_ROWS, N=N_DRAWS, parallel=True, verbose=0,
                           contrast_curve_file=os.path.join(GOLD, "toi465_cc.csv"))
    finally:
        triceratops_amd.set_sampling("numpy")
    before = tg.fit_curves(*data, n_model=N_MODEL)
    model_time, bands = tg.fit_bands(*data, n_model=N_MODEL, q=BAND_Q, model_average=N_MIX, rng=np.random.default_rng(7))
    after = tg.fit_curves(*data, n_model=N_MODEL)
    return {"tg": tg, "data": data, "before": before, "after": after, "model_time": model_time, "bands": bands}


def host_curves(tg, j, p, model_time):
    """the model curves of the parameter sets p (a dict of arrays under the posterior's names) of scenario row j, by the
    CPU oracle: the block is rebuilt here, column for column (include/trx.h: the parameter-block rows)"""
    from oracle import oracle as O
    from triceratops_amd.constants import G, Msun, pi
    is_tp, comp = j % 3 == 0, bool(tg.star_num[j] != 1)
    M = p["M_s"] + (0.0 if is_tp else p["M_EB"])              # Kepler's third law: the binary's total mass
    a = ((G * M * Msun) / (4 * pi ** 2) * (p["P_orb"] * 86400) ** 2) ** (1 / 3)
    tail = (p["P_orb"], p["inc"], a, p["R_s"], p["u1"], p["u2"], p["ecc"], p["argp"], p["fluxratio_comp"])
    if is_tp:
        model, block = O.MODEL_TP, O.pack_params(O.MODEL_TP, p["R_p"], *tail)
    else:
        model, block = O.MODEL_EB, O.pack_params(O.MODEL_EB, p["R_EB"], p["fluxratio_EB"], *tail)
    return O.flux_grid(model, model_time, block, companion_is_host=comp, exptime=0.00139, nsamples=20, scalar_k=True)[0]


def test_bands_of_every_scenario_against_the_oracle(case):
    tg, bands, (mt_c, curves) = case["tg"], case["bands"], case["before"]
    assert np.array_equal(case["model_time"], mt_c) and len(case["model_time"]) == N_MODEL
    assert len(tg.posterior) == 15 and len(bands) == 15 + 1
    with_band = 0
    for j, (b, c) in enumerate(zip(bands, curves)):
        assert b["ID"] == c["ID"] and b["scenario"] == c["scenario"] and tuple(b["q"]) == BAND_Q
        assert np.asarray(b["flux"]).tobytes() == np.asarray(c["flux"]).tobytes()
        assert np.asarray(b["flux_err"]).tobytes() == np.asarray(c["flux_err"]).tobytes()
        assert set(b) == {"ID", "scenario", "flux", "flux_err", "q", "band", "n_samples"}
        p = tg.posterior[j]
        if p is None:
            assert b["band"] is None and b["n_samples"] == 0
            continue
        with_band += 1
        assert b["n_samples"] == M_ROWS and b["band"].shape == (len(BAND_Q), N_MODEL)
        want = np.quantile(host_curves(tg, j, p, case["model_time"]), BAND_Q, axis=0)
        err = float(np.abs(b["band"] - want).max())
        print("%-7s band against the oracle: %.3g (depth %.3g)" % (b["scenario"], err, 1 - want.min()))
        assert err < FLUX_TOL, b["scenario"]
        assert np.all(np.diff(b["band"], axis=0) >= 0)
    assert with_band == int(np.isfinite(tg.lnZ).sum()) and bands[0]["band"] is not None      # (TOI-465.01 is a planet)
    assert any(b["band"] is not None and b["band"].min() < 0.9999 for b in bands[:-1])     # (a transit is in there)


def test_model_average_band(case):
    tg, mix = case["tg"], case["bands"][-1]
    assert mix["scenario"] == "model average" and mix["ID"] == tg.ID and mix["n_samples"] == N_MIX
    G = _gold()
    assert np.array_equal(mix["flux"], G["flux"]) and mix["flux_err"] == float(G["sigma"][0])
    df = tg.posterior_samples(N_MIX, np.random.default_rng(7))
    # the picks are posterior_samples' own
    which, sample = mix["rows"], mix["samples"]
    assert which.shape == sample.shape == (N_MIX,)
    for c in ("R_s", "P_orb"):
        picked = np.array([tg.posterior[j][c][i] for j, i in zip(which, sample)])
        assert picked.tobytes() == df[c].values.tobytes(), c
    assert list(np.asarray(tg.probs["scenario"])[which]) == list(df["scenario"])
    # ... and the band is the host computation over them, each curve back in the target's normalisation
    star_ids = tg.stars["ID"].astype(str).values
    values = np.empty((N_MIX, N_MODEL))
    for j in np.unique(which):
        sel = which == j
        p = {c: df[c].values[sel] for c in tg.posterior[j] if c in df}
        share = tg.stars["fluxratio"].values[np.argwhere(star_ids == str(tg.probs["ID"].values[j]))[0, 0]]
        values[sel] = 1 - share * (1 - host_curves(tg, j, p, case["model_time"]))
    want = np.quantile(values, BAND_Q, axis=0)
    err = float(np.abs(mix["band"] - want).max())
    print("model average over %d scenarios: %.3g" % (np.unique(which).size, err))
    assert err < FLUX_TOL
    assert np.all(np.diff(mix["band"], axis=0) >= 0)


def test_fit_curves_is_unchanged_by_fit_bands(case):
    (t0, c0), (t1, c1) = case["before"], case["after"]
    assert t0.tobytes() == t1.tobytes() and len(c0) == len(c1)
    for a, b in zip(c0, c1):
        assert a["ID"] == b["ID"] and a["scenario"] == b["scenario"]
        for k in ("flux", "flux_err", "model"):
            assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k


def test_fit_bands_needs_samples(case):
    """the errors of posterior_samples, word for word"""
    tg = _target()
    G = _gold()
    data = (G["time"], G["flux"], float(G["sigma"][0]))
    for call in (lambda: tg.fit_bands(*data), lambda: tg.posterior_samples(3)):
        with pytest.raises(ValueError, match="no posterior samples: run calc_posteriors first"):
            call()
    done = case["tg"]
    keep = done.posterior
    try:
        done.posterior = [None] * len(keep)
        for call in (lambda: done.fit_bands(*data), lambda: done.posterior_samples(3)):
            with pytest.raises(ValueError, match="no scenario with posterior samples carries probability"):
                call()
        done.posterior, done.posterior_quantiles = None, [None] * len(keep)
        for call in (lambda: done.fit_bands(*data), lambda: done.posterior_samples(3)):
            with pytest.raises(ValueError, match="holds quantiles only"):
                call()
    finally:
        done.posterior, done.posterior_quantiles = keep, None
