"""target.calc_probs_datasets with baseline columns marginalised under a dataset's Matern-3/2 or two-term noise
(`red_kernel_baseline` / `red_kernel_baseline_sigma` next to `red_kernel`), end to end on the fixtures
of tests/test_gpu_datasets.py: TOI-465.01, two cadences, N = 20 000, set_sampling("device"), one seed for every pass.

Bars, none of them chosen from results.  With plain = the white-noise chi^2/2 of a pass's best draw (the same rows
evaluated again with the plain reduction, as tests/test_gpu_datasets_red_kernel.py does), amp_ou = 1 + 1 / (1 - max alpha),
amp_ss = 1 + Gamma (the l1 gain of the dataset's predictor) and pf = 1 + 4 sqrt(K / lambda_min) of each path's system
(lambda_min does not depend on the star's normalisation: Datasets.renorm):
  without the keys, and with red_kernel alone: the same bits with the keys absent or None, _lib.chi2_grid_ss2_baseline is
        never called and target.dataset_red_kernel_baselines is None;
  cross-path, "ou2" with tau_1 = tau_2 and the columns [1, u] against red_sigma = hypot(s_1, s_2) + red_baseline of the
        same columns (the same covariance): the same masked counts; |d lnZ| <= 1e-12 (amp_ou pf_ou + amp_ss pf_ss) plain
        + 2e-12 -- the two kernels' bars of that file, each times its projection factor --; the same best draw wherever the
        row's two smallest sums of h differ by more than that, and at most a quarter of the finite rows excused (a cap);
  vanishing prior, s_k = 1e-9 sigma_bar of the dataset, against red_kernel alone, row by row on the h the evidence saw:
        |d h| <= 0.5 K s^2 D_max S2 + the device bar, from b~_k^2 <= S2 (Cauchy-Schwarz on unit columns) and
        lambda_min(A~) >= 1 / (s^2 D_max); S2 = 2 h of that dataset <= 2 (the row's sum of h), s^2 D the same in every
        star's normalisation;
  the same data with 0.003 u added to dataset 1, flat priors on [1, u]: |d lnZ| <= the device bar of the two passes; the
        best draws are the same, and each one's slope coefficient is larger by 0.003 to the two passes' coefficient bars,
        ss2_coef_bar / sqrt(D_u) with sum omega (|y| + Gamma max|y|)^2 <= 4 plain (1 + Gamma^2 max sigma^2 sum 1 / sigma^2)
        (omega <= 1 / sigma^2, |y_n| <= sigma_n sqrt(2 plain); the constant's coefficient is held the same way; the
        roundings of flux + 0.003 u are eps against the bar's 1e-12);
  a Matern-3/2 realisation and a slope added to dataset 1, against the CPU oracle's model grid reduced with
        _numerics.ss2_baseline_halfchi2: |d lnZ| <= 1e-9, the bar of the other oracle checks of this path;
  three chunks of the grid, calc_probs_datasets_refined(n_adapt = 0), and a one-node t0_grid (delta, 1) against
        time + delta with the columns moved along (delta = 4 cadences): the same bits;
  evaluation = "fused": NotImplementedError.
Measured (one MI355X): cross-path the same lnZ in bits over 15 finite rows (amp_ou 2.858, amp_ss 1.909, both projection
factors 6.657), the same best draw in all 15, 1 row excused; the vanishing prior every row's h in bits (K s^2 D_max = 8.9e-19);
the added trend max |d lnZ| 6.7e-5 of its bar, every slope coefficient larger by 0.003 to 6.5e-18 (4.9e-5 of its bar);
against the oracle max |d lnZ| 1.2e-11.
"""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from test_gpu_chi2_ss2 import gain
from test_gpu_datasets import KW, KW2, LC, SEED, TARGET_SHARE, _target, _two_cadences, device_mode  # noqa: F401
from test_gpu_datasets_red_kernel import CADENCE_1, COLS, S1, S2, S_ONE, SIGMA_1, TAU, _matern_inputs
from triceratops_amd import _lib, _numerics, fused
from triceratops_amd import datasets as D
from triceratops_amd import lightcurve as lc

pytestmark = pytest.mark.gpu

T_1 = _two_cadences()[1]["time"]
B_1 = lc.trend_columns(T_1, 1)               # [1, u] on dataset 1's stamps
SLOPE = 0.003
OU2 = dict(red_kernel="ou2", red_sigma=(S1, S2), red_timescale=(TAU, TAU))


def _inputs(**keys):
    a, b = _two_cadences()
    return [a, dict(b, **keys)]


class _Spy:
    """per evidence of a pass, in order: h as the evidence saw it and -- replay -- h with white noise and no baseline (the
    same rows evaluated again with the plain reduction); and the calls of the reductions of the correlated-noise paths"""

    def __init__(self, monkeypatch, replay):
        self.h, self.plain = [], []
        self.calls = {"chi2_grid_ss2_baseline": 0, "chi2_grid_ss2": 0, "chi2_grid_ou_baseline": 0, "chi2_grid_ou": 0}
        real_h, real_z = fused._Scenario._datasets_halfchi2, _lib.lnz_from_halfchi2
        spy = self

        def halfchi2(scen, model, flags, block):
            h = real_h(scen, model, flags, block)
            if replay:
                kept, scen.datasets = scen.datasets, [d._replace(term=None) for d in scen.datasets]
                try:
                    spy.plain.append(real_h(scen, model, flags, block).cpu().numpy())
                finally:
                    scen.datasets = kept
            return h

        def lnz(h_d, lp_d, n_total, lnsigma):
            spy.h.append(h_d.cpu().numpy())
            return real_z(h_d, lp_d, n_total, lnsigma)

        def counted(name):
            real = getattr(_lib, name)

            def call(*a, **k):
                spy.calls[name] += 1
                return real(*a, **k)
            return call

        monkeypatch.setattr(fused._Scenario, "_datasets_halfchi2", halfchi2)
        monkeypatch.setattr(_lib, "lnz_from_halfchi2", lnz)
        for name in self.calls:
            monkeypatch.setattr(_lib, name, counted(name))


def _run(monkeypatch, datasets, replay=False, refined=False, **kw):
    tg = _target()
    s = _Spy(monkeypatch, replay)
    torch.manual_seed(SEED)
    _lib.reset_stats()
    if refined:
        tg.calc_probs_datasets_refined(datasets, LC["P_orb"], n_adapt=0, **dict(KW, **kw))
    else:
        tg.calc_probs_datasets(datasets, LC["P_orb"], **dict(KW, **kw))
    rows = _lib.STATS["rows"]
    monkeypatch.undo()
    return {"lnZ": tg.lnZ.copy(), "prob": tg.probs.prob.values.copy(), "rows": rows // (2 if replay else 1),
            "best": np.stack([tg.probs[c].values for c in COLS]), "h": s.h, "plain": s.plain, "calls": s.calls,
            "coef": tg.dataset_red_kernel_baselines, "coef_ou": tg.dataset_red_baselines}


_runs = {}


def _passes(monkeypatch):
    if not _runs:
        _runs["none"] = _run(monkeypatch, _inputs())
        _runs["ou2"] = _run(monkeypatch, _inputs(**OU2), replay=True)
        _runs["ou_gls"] = _run(monkeypatch, _inputs(red_sigma=S_ONE, red_timescale=TAU, red_baseline=B_1), replay=True)
        _runs["ou2_gls"] = _run(monkeypatch, _inputs(red_kernel_baseline=B_1, **OU2), replay=True)
    return _runs


def _same_bits(a, b):
    return (a["lnZ"].tobytes() == b["lnZ"].tobytes() and a["prob"].tobytes() == b["prob"].tobytes()
            and a["best"].tobytes() == b["best"].tobytes() and a["rows"] == b["rows"] > 0)


def _system(keys, B=B_1, sigmas=np.inf):
    """dataset 1's system in the input's normalisation, its 1 + Gamma and its projection factor"""
    d = D.validate(_inputs(**keys))[1]
    s = D.ss2_baseline_system(d, B, sigmas)
    return d, s, 1.0 + gain(s.A, s.g), 1.0 + 4.0 * np.sqrt(B.shape[0] / s.lambda_min)


def test_without_the_keys_no_new_call(device_mode, monkeypatch):
    r = _passes(monkeypatch)
    assert np.isfinite(r["none"]["lnZ"]).sum() >= 10
    for name in ("none", "ou2", "ou_gls"):
        assert r[name]["calls"]["chi2_grid_ss2_baseline"] == 0 and r[name]["coef"] is None, name
    absent = _run(monkeypatch, _inputs(red_kernel_baseline=None, red_kernel_baseline_sigma=None))
    assert _same_bits(r["none"], absent) and absent["calls"]["chi2_grid_ss2_baseline"] == 0 and absent["coef"] is None
    alone = _run(monkeypatch, _inputs(red_kernel_baseline=None, **OU2))
    assert _same_bits(r["ou2"], alone) and alone["calls"]["chi2_grid_ss2_baseline"] == 0 and alone["coef"] is None
    assert alone["calls"]["chi2_grid_ss2"] == r["ou2"]["calls"]["chi2_grid_ss2"] > 0
    # with the keys the new reduction runs in place of the kernel's own
    g = r["ou2_gls"]
    assert g["calls"]["chi2_grid_ss2_baseline"] > 0 and g["calls"]["chi2_grid_ss2"] == 0 and g["calls"]["chi2_grid_ou"] == 0
    assert g["coef_ou"] is None and len(g["coef"]) == g["lnZ"].size
    fin = np.isfinite(g["lnZ"])
    for k, per in enumerate(g["coef"]):
        assert per[0] is None and per[1].shape == (2,) and np.isfinite(per[1]).all() == fin[k]


def test_two_equal_time_scales_are_the_ou_baseline(device_mode, monkeypatch):
    r = _passes(monkeypatch)
    u, s = r["ou_gls"], r["ou2_gls"]
    d_ou = D.validate(_inputs(red_sigma=S_ONE, red_timescale=TAU))[1]
    sys_ou = D.ou_baseline_system(d_ou, B_1, np.inf)
    _, sys_ss, amp_ss, pf_ss = _system(OU2)
    amp_ou, pf_ou = 1.0 + 1.0 / (1.0 - sys_ou.alpha.max()), 1.0 + 4.0 * np.sqrt(2 / sys_ou.lambda_min)
    assert len(s["h"]) == len(u["h"]) == len(s["plain"]) == s["lnZ"].size
    assert u["rows"] == s["rows"] == r["none"]["rows"] > 0, "masked counts differ"
    fin = np.isfinite(u["lnZ"])
    assert np.array_equal(fin, np.isfinite(s["lnZ"])) and fin.sum() >= 10
    n_sep = n_same = 0
    worst = 0.0
    for j in np.flatnonzero(fin):
        h = s["h"][j]
        best = int(np.argmin(h))
        bar = 1e-12 * (amp_ou * pf_ou + amp_ss * pf_ss) * s["plain"][j][best] + 2e-12
        d = abs(u["lnZ"][j] - s["lnZ"][j])
        worst = max(worst, d / bar)
        print("row %d: |d lnZ| %.3g, bar %.3g" % (j, d, bar))
        assert d <= bar, (j, d, bar)
        two = np.partition(h, 1)[:2] if h.size > 1 else np.array([h[0], np.inf])
        same = np.array_equal(u["best"][:, j], s["best"][:, j])
        if two[1] - two[0] > bar:
            n_sep += 1
            assert same, "row %d: best draws differ although the two smallest h are %g apart" % (j, two[1] - two[0])
        n_same += same
    print("ou2 with equal time scales and [1, u] against red_sigma = hypot + red_baseline: amp_ou %.4g pf_ou %.4g, amp_ss %.4g "
          "pf_ss %.4g, max |d lnZ| / bar %.3g over %d finite rows; two smallest h further apart than the bar in %d rows, the "
          "same best draw in %d" % (amp_ou, pf_ou, amp_ss, pf_ss, worst, fin.sum(), n_sep, n_same))
    assert fin.sum() - n_sep <= 0.25 * fin.sum()
    # the columns change the evidence: the point of the feature
    assert np.abs(s["lnZ"][fin] - r["ou2"]["lnZ"][fin]).max() > 1e-3


def test_a_vanishing_prior_is_the_kernel_alone(device_mode, monkeypatch):
    r = _passes(monkeypatch)
    sig = np.full(2, 1e-9 * SIGMA_1)
    _, system, amp_ss, pf_ss = _system(OU2, sigmas=sig)
    got = _run(monkeypatch, _inputs(red_kernel_baseline=B_1, red_kernel_baseline_sigma=sig, **OU2))
    alone = r["ou2"]
    assert got["calls"]["chi2_grid_ss2_baseline"] > 0 and got["rows"] == alone["rows"] and len(got["h"]) == len(alone["h"])
    factor = 0.5 * 2 * float(np.max(sig * sig * system.D)) * 2.0           # 0.5 K s^2 D_max x (S2 <= 2 h)
    worst = 0.0
    for a, b, plain in zip(got["h"], alone["h"], alone["plain"]):
        assert a.shape == b.shape and np.array_equal(np.isfinite(a), np.isfinite(b))
        fin = np.isfinite(b)
        bar = factor * b[fin] + 1e-12 * amp_ss * pf_ss * plain[fin] + 2e-12
        if fin.any():
            worst = max(worst, float(np.max(np.abs(a[fin] - b[fin]) / bar)))
        assert (np.abs(a[fin] - b[fin]) <= bar).all()
    print("vanishing prior against red_kernel alone: K s^2 D_max = %.3g, max |d h| / bar %.3g" % (factor, worst))
    fin = np.isfinite(alone["lnZ"])
    assert np.array_equal(fin, np.isfinite(got["lnZ"])) and np.array_equal(got["best"][:, fin], alone["best"][:, fin])


def test_an_added_trend_is_absorbed_and_reported(device_mode, monkeypatch):
    r = _passes(monkeypatch)
    base = r["ou2_gls"]
    flux = _two_cadences()[1]["flux"] + SLOPE * B_1[1]
    tilted = _run(monkeypatch, _inputs(flux=flux, red_kernel_baseline=B_1, **OU2), replay=True)
    d, system, amp_ss, pf_ss = _system(OU2)
    gamma = amp_ss - 1.0
    spread = 1.0 + gamma ** 2 * float(np.max(d.flux_err ** 2) * np.sum(1.0 / d.flux_err ** 2))
    fin = np.isfinite(base["lnZ"])
    assert np.array_equal(fin, np.isfinite(tilted["lnZ"])) and fin.sum() >= 10 and base["rows"] == tilted["rows"]
    worst = worst_c = 0.0
    for j in np.flatnonzero(fin):
        p0 = base["plain"][j][int(np.argmin(base["h"][j]))]
        p1 = tilted["plain"][j][int(np.argmin(tilted["h"][j]))]
        bar = 1e-12 * amp_ss * pf_ss * (p0 + p1) + 4e-12
        dz = abs(base["lnZ"][j] - tilted["lnZ"][j])
        worst = max(worst, dz / bar)
        assert dz <= bar, (j, dz, bar)
        two = np.partition(base["h"][j], 1)[:2] if base["h"][j].size > 1 else np.array([0.0, np.inf])
        if two[1] - two[0] <= bar:
            continue                                             # (a tie within the bar: either draw may be reported)
        assert np.array_equal(base["best"][:, j], tilted["best"][:, j])
        c0, c1 = base["coef"][j][1], tilted["coef"][j][1]
        bar_c = sum(1e-12 * amp_ss * np.sqrt(2 * 4.0 * p * spread) / system.lambda_min + 1e-15 for p in (p0, p1)) \
            / np.sqrt(system.D)
        print("row %d: |d lnZ| %.3g (bar %.3g), slope %.6g -> %.6g, |d - 0.003| %.3g (bar %.3g)"
              % (j, dz, bar, c0[1], c1[1], abs(c1[1] - c0[1] - SLOPE), bar_c[1]))
        worst_c = max(worst_c, abs(c1[1] - c0[1] - SLOPE) / bar_c[1], abs(c1[0] - c0[0]) / bar_c[0])
        assert abs(c1[1] - c0[1] - SLOPE) <= bar_c[1] and abs(c1[0] - c0[0]) <= bar_c[0]
    print("0.003 u added to dataset 1: max |d lnZ| / bar %.3g, max |d coef| / bar %.3g" % (worst, worst_c))
    # without the columns the same trend moves the evidence
    plain = _run(monkeypatch, _inputs(flux=flux, **OU2))
    assert np.abs(plain["lnZ"][fin] - r["ou2"]["lnZ"][fin]).max() > 1e-3


def _sloped_matern_inputs():
    """tests/test_gpu_datasets_red_kernel.py's Matern-3/2 realisation on dataset 1, a slope added, and the keys"""
    a, b = _matern_inputs()
    return [a, dict(b, flux=b["flux"] + SLOPE * B_1[1], red_kernel_baseline=B_1, red_kernel_baseline_sigma=[np.inf, 5e-3])]


def test_chunks_refined_shift_node_and_fused_refusal(device_mode, monkeypatch):
    data = _sloped_matern_inputs()
    whole = _run(monkeypatch, data)
    assert whole["calls"]["chi2_grid_ss2_baseline"] > 0 and whole["calls"]["chi2_grid_ss2"] == 0
    assert np.isfinite(whole["lnZ"]).sum() >= 10
    n_min = min(h.size for h in whole["h"] if h.size >= 3)
    # (a chunk of n_min // 3 rows of the longer dataset: every branch of at least n_min rows takes three chunks or more)
    with fused.switches(DATASET_GRID_BYTES=8 * 50 * (n_min // 3)):
        chunked = _run(monkeypatch, data)
    assert chunked["calls"]["chi2_grid_ss2_baseline"] >= 3 * sum(h.size >= 3 for h in whole["h"])
    assert chunked["calls"]["chi2_grid_ss2_baseline"] > whole["calls"]["chi2_grid_ss2_baseline"]
    assert _same_bits(whole, chunked)
    refined = _run(monkeypatch, data, refined=True)
    assert _same_bits(whole, refined)
    for a, b in zip(whole["coef"], refined["coef"]):
        assert a[0] is None and b[0] is None and np.array_equal(a[1], b[1], equal_nan=True)
    # a one-node t0_grid (delta, 1) is the stamps time + delta with the columns moved along (they are aligned by index)
    delta = 4.0 * CADENCE_1
    moved = dict(data[1], time=data[1]["time"] + delta)
    for u, v in zip(D.ss2_system(D.validate([moved])[0]), D.ss2_system(D.validate([data[1]])[0])):
        assert u.tobytes() == v.tobytes()
    a = _run(monkeypatch, [data[0], moved])
    b = _run(monkeypatch, [data[0], dict(data[1], t0_grid=[(delta, 1.0)])])
    assert _same_bits(a, b) and not _same_bits(a, whole)
    for x, y in zip(a["coef"], b["coef"]):
        assert np.array_equal(x[1], y[1], equal_nan=True)        # reported at the grid's one node
    tg = _target()
    with pytest.raises(NotImplementedError):
        tg.calc_probs_datasets(data, LC["P_orb"], evaluation="fused", **KW2)


def test_evidence_against_the_oracle(device_mode, monkeypatch):
    """TP and EB (+ twin) of the target star on two cadences, errors varying 3x, a Matern-3/2 realisation plus a slope and
    the keys on dataset 1: the model curves from the oracle, the statement and the evidence in numpy."""
    data = _sloped_matern_inputs()
    kw = dict(KW, drop_scenario=KW2["drop_scenario"] + ["PTP", "PEB"])
    tg = _target()
    dump = []
    monkeypatch.setattr(fused, "DUMP", dump)
    torch.manual_seed(SEED)
    tg.calc_probs_datasets(data, LC["P_orb"], **kw)
    monkeypatch.undo()
    assert len(dump) == 2
    sets = D.validate(data)
    ds = D.Datasets(sets, red_kernel_baselines=D.red_kernel_baselines(data, sets)).renorm(float(TARGET_SHARE))
    assert ds.sets[0].red_kernel is None and ds.sets[1].red_kernel == "matern32" and ds.red_kernel_baselines[0] is None
    system = D.ss2_baseline_system(ds.sets[1], *ds.red_kernel_baselines[1])
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
                resid = s.flux - grid
                if l == 0:
                    h += 0.5 * np.sum(resid * resid / s.flux_err ** 2, axis=1)
                else:
                    h += _numerics.ss2_baseline_halfchi2(resid, system)
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
    print("matern32 dataset with [1, u] against the oracle: max |d lnZ| %.3g" % np.abs(got[fin] - want[fin]).max())
    assert np.abs(got[fin] - want[fin]).max() <= 1e-9
