"""target.calc_probs_datasets with baseline columns marginalised under correlated noise (`red_baseline` /
`red_baseline_sigma` next to `red_sigma` / `red_timescale`), end to end on the fixtures of
tests/test_gpu_datasets_red_noise.py: TOI-465.01, two cadences, N = 20 000, set_sampling("device"), one seed for every pass.

Bars, none of them chosen from results (u: the unit time of dataset 1, lightcurve.polynomial_baseline):
  no keys / keys = None: the same bits, and _lib.chi2_grid_ou_baseline is never called;
  cross-path: red_sigma = s, red_timescale = inf, red_baseline = [u] (flat) on dataset 1 against offset_sigma = s,
        baseline = [u] (flat) through the white kernel (s = 3 sigma_bar of that dataset; K = diag(sigma^2) + s^2 1 1^T is
        white noise plus a constant of prior s): the same masked counts; |d lnZ| <= the sum of the two kernels' bars on one
        draw's h, with the plain chi^2/2 of the pass's best draw in place of their sums, as tests/test_gpu_datasets_red_noise.py
        does: 1e-12 (1 + 1 / (1 - max alpha)) chi^2/2 (1 + 4 sqrt(1 / lambda_min)) + 1e-12 (tests/test_gpu_chi2_ou_baseline.py)
        plus 1e-12 chi^2/2 (1 + 4 sqrt(2 / lambda_min')) + 1e-12 (tests/test_gpu_chi2_baseline.py); the same best draw
        wherever the row's two smallest h differ by more than that, and at most a quarter of the finite rows excused;
  vanishing prior, red_baseline_sigma = 1e-9 sigma_bar, against red_sigma alone: per draw
        |d h| <= 0.5 K max(s^2 D) x (plain chi^2/2) x 2 (tests/test_datasets_red_baseline_api.py: 0.5 K max(s^2 D) S2, and
        S2 <= 2 x the plain chi^2/2 because K^-1 <= diag(1 / sigma^2)); s^2 D is of the order of 1e-17 here, so the one
        rounding of S2 - q, one spacing of h, is added;
  a linear trend and an OU realisation added to dataset 1, the matching keys, against the CPU oracle's model grid reduced
        with _numerics.ou_baseline_halfchi2: |d lnZ| <= 1e-9, the bar of the offset's, the baseline's and the red noise's
        oracle checks; dataset_red_baselines of the best draw against the host statement's coefficients (long double, on
        the model row the device evaluated for that draw) to the coef_out bar of tests/test_gpu_chi2_ou_baseline.py;
  trend invariance: the same data with 0.003 u added, u under a flat prior: the same lnZ within the device bar of
        tests/test_gpu_chi2_ou_baseline.py on the best draw's residuals at the shifted level;
  three chunks of the grid, calc_probs_datasets_refined(n_adapt = 0), and a one-node t0_grid (delta, 1) against
        time + delta (delta = 4 cadences): the same bits;
  evaluation = "fused": NotImplementedError naming red_baseline.
Measured (one MI355X): cross-path max |d lnZ| 2.8e-6 of the summed bars over 15 finite rows, the same best draw in all 15,
1 row excused (its two smallest h tie: gap 0); vanishing prior: max s^2 D 4.2e-19, the same h in bits; against the oracle
max |d lnZ| 1.8e-12, the coefficients 1.9e-6 of the coef_out bar; 0.003 u added: max |d lnZ| 4.7e-5 of the device bar.
"""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from test_datasets_red_baseline_api import coef_bar, gls_bar
from test_gpu_datasets import KW, KW2, LC, SEED, TARGET_SHARE, _target, _two_cadences, device_mode  # noqa: F401
from triceratops_amd import _lib, _numerics, fused
from triceratops_amd import datasets as D
from triceratops_amd.lightcurve import polynomial_baseline, trend_columns

pytestmark = pytest.mark.gpu

INF = float("inf")
LD = np.longdouble
SIGMA_BAR = D.Datasets(D.validate(_two_cadences())).sigma_ref          # of the input, the target's normalisation
SIGMA_1 = D.Datasets(D.validate(_two_cadences()[1:])).sigma_ref        # sigma_bar of dataset 1 alone
CADENCE_1 = float(np.median(np.diff(_two_cadences()[1]["time"])))
U = polynomial_baseline(_two_cadences()[1]["time"], 1)[0]
COLS = ("M_s", "R_s", "P_orb", "inc", "b", "ecc", "w", "R_p", "M_EB", "R_EB")


def _inputs(add=None, **keys):
    a, b = _two_cadences()
    if add is not None:
        b = dict(b, flux=b["flux"] + add)
    return [a, dict(b, **keys)]


def _system(data, l=1):
    """the system of dataset l in the input's normalisation (lambda_min, max alpha and s^2 D are those of every star)"""
    sets = D.validate(data)
    pair = D.red_baselines(data, sets)[l]
    return D.ou_baseline_system(sets[l], *pair)


class _Spy:
    """per evidence of a pass, in order: h as the evidence saw it, h with nothing marginalised and white noise (the same
    rows evaluated again with the plain reduction), the draws' priors; the calls of _lib.chi2_grid_ou_baseline, and of its
    one-row calls that ask for coefficients (the best draw of a branch) the residuals, tables and coefficients"""

    def __init__(self, monkeypatch, replay):
        self.h, self.plain, self.lp, self.calls, self.best = [], [], [], 0, []
        real_h, real_z, real_g = fused._Scenario._datasets_halfchi2, _lib.lnz_from_halfchi2, _lib.chi2_grid_ou_baseline
        spy = self

        def halfchi2(scen, model, flags, block):
            h = real_h(scen, model, flags, block)
            if replay:
                kept = scen.datasets
                scen.datasets = [d._replace(term=None) for d in scen.datasets]
                try:
                    spy.plain.append(real_h(scen, model, flags, block).cpu().numpy())
                finally:
                    scen.datasets = kept
            return h

        def lnz(h_d, lp_d, n_total, lnsigma):
            spy.h.append(h_d.cpu().numpy())
            spy.lp.append(None if lp_d is None else lp_d.cpu().numpy())
            return real_z(h_d, lp_d, n_total, lnsigma)

        def gls(flux_d, grid_d, alpha_d, beta_d, omega_d, cols_d, minv, *a, **k):
            spy.calls += 1
            out = real_g(flux_d, grid_d, alpha_d, beta_d, omega_d, cols_d, minv, *a, **k)
            if k.get("coef_out") is not None and grid_d.shape[0] == 1:
                spy.best.append(dict(y=flux_d.cpu().numpy() - grid_d.cpu().numpy()[0], alpha=alpha_d.cpu().numpy(),
                                     beta=beta_d.cpu().numpy(), omega=omega_d.cpu().numpy(), c=cols_d.cpu().numpy(),
                                     minv=np.array(minv), coef=k["coef_out"].cpu().numpy()[0].copy(),
                                     h=float(out.cpu()[0])))
            return out

        monkeypatch.setattr(fused._Scenario, "_datasets_halfchi2", halfchi2)
        monkeypatch.setattr(_lib, "lnz_from_halfchi2", lnz)
        monkeypatch.setattr(_lib, "chi2_grid_ou_baseline", gls)


def _run(monkeypatch, datasets, replay=False, refined=False, kw=KW, **more):
    tg = _target()
    s = _Spy(monkeypatch, replay)
    torch.manual_seed(SEED)
    _lib.reset_stats()
    if refined:
        tg.calc_probs_datasets_refined(datasets, LC["P_orb"], n_adapt=0, **dict(kw, **more))
    else:
        tg.calc_probs_datasets(datasets, LC["P_orb"], **dict(kw, **more))
    rows = _lib.STATS["rows"]
    monkeypatch.undo()
    return {"lnZ": tg.lnZ.copy(), "prob": tg.probs.prob.values.copy(), "rows": rows // (2 if replay else 1),
            "best": np.stack([tg.probs[c].values for c in COLS]), "target": tg, "h": s.h, "plain": s.plain, "lp": s.lp,
            "calls": s.calls, "best_calls": s.best, "coefs": tg.dataset_red_baselines}


def _same_bits(a, b):
    return (a["lnZ"].tobytes() == b["lnZ"].tobytes() and a["prob"].tobytes() == b["prob"].tobytes()
            and a["best"].tobytes() == b["best"].tobytes() and a["rows"] == b["rows"] > 0)


def _ou(seed=465):
    """an OU realisation on dataset 1's stamps (s_r = 2 sigma of dataset 1, tau = 20 cadences; a fixed seed)"""
    t = _two_cadences()[1]["time"]
    s_r, tau = 2.0 * SIGMA_1, 20.0 * CADENCE_1
    rng = np.random.default_rng(seed)
    x = np.empty(t.size)
    x[0] = s_r * rng.normal()
    for n in range(1, t.size):
        phi = np.exp(-(t[n] - t[n - 1]) / tau)
        x[n] = phi * x[n - 1] + s_r * np.sqrt(1.0 - phi * phi) * rng.normal()
    return x, s_r, tau


A_TREND, B_TREND = 2.0 * SIGMA_1, 3.0 * SIGMA_1          # a linear trend of a few sigma_bar


def _trend_inputs(extra=0.0, **more):
    """dataset 1 with a + b u and an OU realisation added, the matching noise keys and the columns (1, u), flat"""
    x, s_r, tau = _ou()
    keys = dict(red_sigma=s_r, red_timescale=tau, red_baseline=trend_columns(_two_cadences()[1]["time"], 1))
    keys.update(more)
    return _inputs(add=A_TREND + B_TREND * U + x + extra, **keys)


_runs = {}


def _passes(monkeypatch):
    if not _runs:
        _runs["none"] = _run(monkeypatch, _inputs())
        _runs["trend"] = _run(monkeypatch, _trend_inputs(), replay=True)
    return _runs


def test_without_the_keys_nothing_changes(device_mode, monkeypatch):
    a = _passes(monkeypatch)["none"]
    b = _run(monkeypatch, _inputs(red_baseline=None, red_baseline_sigma=None))
    assert np.isfinite(a["lnZ"]).sum() >= 10 and _same_bits(a, b)
    assert a["calls"] == b["calls"] == 0 and a["coefs"] is None and b["coefs"] is None
    # red noise alone keeps its kernel
    x, s_r, tau = _ou()
    c = _run(monkeypatch, _inputs(add=x, red_sigma=s_r, red_timescale=tau), kw=KW2)
    assert c["calls"] == 0 and c["coefs"] is None and np.isfinite(c["lnZ"]).sum() >= 4
    assert _passes(monkeypatch)["trend"]["calls"] > 0


def test_infinite_timescale_is_the_white_baseline_with_a_constant(device_mode, monkeypatch):
    s_in = 3.0 * SIGMA_1
    g_in = _inputs(red_sigma=s_in, red_timescale=INF, red_baseline=U)
    b_in = _inputs(offset_sigma=s_in, baseline=U)
    g, b = _run(monkeypatch, g_in, replay=True), _run(monkeypatch, b_in, replay=True)
    sys_g = _system(g_in)
    sys_b = D.baseline_system(D.validate(b_in)[1])
    amp_g = (1.0 + 1.0 / (1.0 - sys_g.alpha.max())) * (1.0 + 4.0 * np.sqrt(1.0 / sys_g.lambda_min))
    amp_b = 1.0 + 4.0 * np.sqrt(2.0 / sys_b.lambda_min)
    assert g["calls"] > 0 and b["calls"] == 0
    assert len(g["h"]) == len(b["h"]) == len(g["plain"]) == g["lnZ"].size
    assert g["rows"] == b["rows"] == _passes(monkeypatch)["none"]["rows"] > 0, "masked counts differ"
    fin = np.isfinite(g["lnZ"])
    assert np.array_equal(fin, np.isfinite(b["lnZ"])) and fin.sum() >= 10
    n_sep = n_same = 0
    worst = 0.0
    gaps = []
    for j in np.flatnonzero(fin):
        h = g["h"][j]
        best = int(np.argmin(h))
        bar = 1e-12 * (amp_g + amp_b) * g["plain"][j][best] + 2e-12
        d = abs(g["lnZ"][j] - b["lnZ"][j])
        worst = max(worst, d / bar)
        print("row %d: |d lnZ| %.3g, bar %.3g" % (j, d, bar))
        assert d <= bar, (j, d, bar)
        two = np.partition(h, 1)[:2] if h.size > 1 else np.array([h[0], np.inf])
        same = np.array_equal(g["best"][:, j], b["best"][:, j])
        gaps.append((two[1] - two[0]) / bar)
        if two[1] - two[0] > bar:
            n_sep += 1
            assert same, "row %d: best draws differ although the two smallest h are %g apart" % (j, two[1] - two[0])
        n_same += same
    print("tau = inf + [u] against offset_sigma + baseline [u]: amplifications %.4g and %.4g, max |d lnZ| / bar %.3g over %d "
          "finite rows; two smallest h further apart than the bar in %d rows (smallest gap / bar %.3g), excused %d, the same "
          "best draw in %d" % (amp_g, amp_b, worst, fin.sum(), n_sep, min(gaps), fin.sum() - n_sep, n_same))
    assert fin.sum() - n_sep <= 0.25 * fin.sum()
    # the keys change the evidence: the point of the feature
    assert np.abs(g["lnZ"][fin] - _passes(monkeypatch)["none"]["lnZ"][fin]).max() > 1e-3


def test_a_vanishing_prior_is_the_red_noise_alone(device_mode, monkeypatch):
    x, s_r, tau = _ou()
    s_in = 1e-9 * SIGMA_BAR
    cols = trend_columns(_two_cadences()[1]["time"], 1)
    t_in = _inputs(add=x, red_sigma=s_r, red_timescale=tau, red_baseline=cols, red_baseline_sigma=s_in)
    t = _run(monkeypatch, t_in, replay=True)
    plain = _run(monkeypatch, _inputs(add=x, red_sigma=s_r, red_timescale=tau))
    assert t["calls"] > 0 and plain["calls"] == 0
    fin = np.isfinite(plain["lnZ"])
    assert np.array_equal(fin, np.isfinite(t["lnZ"])) and t["rows"] == plain["rows"] and fin.sum() >= 10
    sys_t = _system(t_in)
    s2D = float(np.max(s_in ** 2 * sys_t.D))
    worst = worst_bound = 0.0
    for j in np.flatnonzero(fin):
        h, h0, p = t["h"][j], plain["h"][j], t["plain"][j]
        live = np.isfinite(h0)
        assert np.array_equal(live, np.isfinite(h)) and live.any()
        bound = 0.5 * 2 * s2D * p[live] * 2.0 + np.spacing(h0[live])
        assert (np.abs(h[live] - h0[live]) <= bound).all()
        worst, worst_bound = max(worst, float(np.abs(h[live] - h0[live]).max())), max(worst_bound, float(bound.max()))
    d = np.abs(t["lnZ"][fin] - plain["lnZ"][fin]).max()
    print("vanishing prior: max s^2 D = %.3g, largest bound on |d h| %.3g, measured %.3g, max |d lnZ| %.3g"
          % (s2D, worst_bound, worst, d))
    assert s2D <= 1e-12 and d <= worst_bound + 1e-12
    assert np.array_equal(t["best"], plain["best"])
    assert all(row[0] is None and row[1].shape == (2,) for row in t["coefs"])


def _device_bar(call, lambda_min):
    """the device bar of tests/test_gpu_chi2_ou_baseline.py on the residuals of a best-draw call"""
    system = D.OuBaselineSystem(call["alpha"], call["beta"], call["omega"], call["c"], None, None, None, lambda_min)
    return float(gls_bar(call["y"][None, :], system)[0])


def test_a_flat_column_in_the_data_does_not_show(device_mode, monkeypatch):
    base = _passes(monkeypatch)["trend"]
    moved = _run(monkeypatch, _trend_inputs(extra=0.003 * U), replay=True)
    lam = _system(_trend_inputs()).lambda_min
    fin = np.isfinite(base["lnZ"])
    assert np.array_equal(fin, np.isfinite(moved["lnZ"])) and base["rows"] == moved["rows"] and fin.sum() >= 10
    live = [j for j in range(fin.size) if moved["h"][j].size > 0]
    assert len(live) == len(moved["best_calls"]) == len(base["best_calls"])
    worst = 0.0
    for call, j in zip(moved["best_calls"], live):
        if not fin[j]:
            continue
        bar = _device_bar(call, lam)                            # (at the shifted level: the larger of the two passes')
        d = abs(moved["lnZ"][j] - base["lnZ"][j])
        worst = max(worst, d / bar)
        print("row %d: |d lnZ| %.3g, bar %.3g (plain chi^2/2 of the best draw %.4g -> %.4g)"
              % (j, d, bar, base["plain"][j][int(np.argmin(base["h"][j]))], moved["plain"][j][int(np.argmin(moved["h"][j]))]))
        assert d <= bar, (j, d, bar)
    print("0.003 u added under a flat prior on u (lambda_min %.3g): max |d lnZ| / bar %.3g over %d rows" % (lam, worst, fin.sum()))
    same = np.array([np.array_equal(base["best"][:, j], moved["best"][:, j]) for j in np.flatnonzero(fin)])
    assert same.mean() >= 0.75
    # the slope coefficient took the shift up
    star = np.array([moved["coefs"][j][1][1] - base["coefs"][j][1][1] for j in np.flatnonzero(fin)[same]])
    assert np.allclose(star, 0.003, rtol=1e-6, atol=0)


def test_chunks_refined_t0_node_and_fused_refusal(device_mode, monkeypatch):
    data = _trend_inputs()
    whole = _run(monkeypatch, data, kw=KW2)
    assert whole["calls"] > 0 and np.isfinite(whole["lnZ"]).sum() >= 4
    n_min = min(h.size for h in whole["h"] if h.size >= 3)
    # (a chunk of n_min // 3 rows of the longer dataset: every branch of at least n_min rows takes three chunks or more)
    with fused.switches(DATASET_GRID_BYTES=8 * 50 * (n_min // 3)):
        chunked = _run(monkeypatch, data, kw=KW2)
    assert chunked["calls"] > whole["calls"]
    assert _same_bits(whole, chunked)
    refined = _run(monkeypatch, data, refined=True, kw=KW2)
    assert _same_bits(whole, refined)
    for a, b in zip(whole["coefs"], refined["coefs"]):
        assert a[0] is None and b[0] is None and np.array_equal(a[1], b[1], equal_nan=True)
    # a one-node t0_grid (delta, 1) is the stamps time + delta: the columns follow the points
    # (delta = 4 cadences, as tests/test_gpu_datasets_t0_grid.py: the differences of the shifted stamps keep their bits,
    # so the noise tables of the two inputs are the same)
    delta = 4.0 * CADENCE_1
    shifted = _trend_inputs()
    moved_t = dict(shifted[1], time=shifted[1]["time"] + delta)
    node = dict(shifted[1], t0_grid=[(delta, 1.0)])
    a = _run(monkeypatch, [shifted[0], moved_t], kw=KW2)
    b = _run(monkeypatch, [shifted[0], node], kw=KW2)
    assert _same_bits(a, b)
    for x, y in zip(a["coefs"], b["coefs"]):
        assert np.array_equal(x[1], y[1], equal_nan=True)
    tg = _target()
    with pytest.raises(NotImplementedError, match="red_baseline"):
        tg.calc_probs_datasets(data, LC["P_orb"], evaluation="fused", **KW2)


def test_trend_and_red_noise_evidence_against_the_oracle(device_mode, monkeypatch):
    """TP and EB (+ twin) of the target star on two cadences, errors varying 3x; a linear trend, an OU realisation, the
    noise keys and the columns (1, u) -- the slope under a prior -- on dataset 1: the model curves from the oracle, the
    recurrence, the projection and the evidence in numpy."""
    data = _trend_inputs(red_baseline_sigma=[INF, 30.0 * SIGMA_BAR])
    kw = dict(KW2, drop_scenario=KW2["drop_scenario"] + ["PTP", "PEB"])
    tg = _target()
    dump = []
    spy = _Spy(monkeypatch, False)
    monkeypatch.setattr(fused, "DUMP", dump)
    torch.manual_seed(SEED)
    tg.calc_probs_datasets(data, LC["P_orb"], **kw)
    monkeypatch.undo()
    assert len(dump) == 2
    ds = D.Datasets(D.validate(data), red_baselines=D.red_baselines(data, D.validate(data))).renorm(float(TARGET_SHARE))
    assert ds.red_baselines[0] is None and ds.red_baselines[1] is not None and ds.sets[1].red_sigma is not None
    system = D.ou_baseline_system(ds.sets[1], *ds.red_baselines[1])
    want = []
    for d in dump:
        cols = d["cols"].cpu().numpy()
        mask, mask2 = d["mask"].cpu().numpy(), None if d["mask_twin"] is None else d["mask_twin"].cpu().numpy()
        lnprior = None if d["lnprior"] is None else d["lnprior"].cpu().numpy()
        planet = mask2 is None
        branches = ((O.MODEL_TP, mask, False),) if planet else ((O.MODEL_EB, mask, False), (O.MODEL_EB_TWIN, mask2, True))
        for model, m, twin in branches:
            idx = np.flatnonzero(m)
            block = cols[:10 if planet else 11][:, idx].copy()
            if twin:
                block[2] *= 2.0
                block[4] = cols[11][idx]
            h = np.zeros(idx.size)
            for l, s in enumerate(ds.sets):
                grid, sec = O.flux_grid(model, s.time, block, exptime=s.exptime, nsamples=s.nsamples)
                r = s.flux - grid
                if ds.red_baselines[l] is None:
                    h += 0.5 * np.sum(r * r / s.flux_err ** 2, axis=1)
                else:
                    h += _numerics.ou_baseline_halfchi2(r, system)
                if l == 0 and model == O.MODEL_EB:
                    h[sec >= 1.5 * ds.sigma_ref] = np.inf
            x = -0.5 * np.log(2 * np.pi) - np.log(ds.sigma_ref) - h
            if lnprior is not None:
                x = x + lnprior[idx]
            full = np.full(m.size, -np.inf)
            full[idx] = x
            want.append(O.log_mean_exp(full, m.size))
    want = np.array(want)
    got = tg.lnZ[:3]
    assert np.array_equal(np.isfinite(want), np.isfinite(got)) and np.isfinite(want).sum() >= 2
    fin = np.isfinite(want)
    print("trend + red-noise dataset against the oracle: max |d lnZ| %.3g" % np.abs(got[fin] - want[fin]).max())
    assert np.abs(got[fin] - want[fin]).max() <= 1e-9
    # the best draws' coefficients: the host statement in long double on the model row the device evaluated
    live = [j for j in range(3) if spy.h[j].size > 0]
    assert len(spy.best) == len(live) and len(tg.dataset_red_baselines) == tg.lnZ.size
    worst = 0.0
    for call, j in zip(spy.best, live):
        assert np.array_equal(call["c"], system.c) and np.array_equal(call["minv"], system.minv)
        _, coef = _numerics.ou_baseline_halfchi2(call["y"][None, :], system, dtype=LD, return_coef=True)
        bar = coef_bar(call["y"][None, :], system)[0]
        scaled = tg.dataset_red_baselines[j][1] / float(TARGET_SHARE) * np.sqrt(system.D)
        r = float(np.max(np.abs(np.asarray(scaled.astype(LD) - coef[0], dtype=np.float64))) / bar)
        worst = max(worst, r)
        print("row %d: coefficients %s (flux units), |d coef~| / bar %.3g" % (j, tg.dataset_red_baselines[j][1], r))
        assert tg.dataset_red_baselines[j][0] is None and np.isfinite(got[j])
        # (the division by sqrt(D) and the two factors of the flux ratio: three roundings of the coefficient itself)
        assert r <= 1.0 + 4 * np.finfo(float).eps * float(np.max(np.abs(coef[0]))) / bar
    print("dataset_red_baselines against the long-double statement: largest |d coef~| / bar %.3g" % worst)
