"""target.calc_probs_datasets with correlated (red) noise per dataset (`red_sigma` / `red_timescale`),
end to end on the fixtures of tests/test_gpu_datasets.py: TOI-465.01, two cadences, N = 20 000, set_sampling("device"), one
seed for every pass.

Bars, none of them chosen from results:
  no keys / keys = None: the same bits, and _lib.chi2_grid_ou is never called;
  red_timescale = inf, red_sigma = s on dataset 1 against offset_sigma = s (s = 3 sigma_bar of that dataset): the same
        masked counts; |d lnZ| <= 1e-12 (1 + 1 / (1 - max alpha)) x (chi^2/2 of the best draw, nothing marginalised) + 1e-12
        -- the kernel's bound on one draw's h (tests/test_gpu_chi2_ou.py); the same best draw wherever the row's two
        smallest sums of h differ by more than that, and at most a quarter of the finite rows excused by that condition;
  red_sigma = 1e-6 sigma_bar, tau = 10 cadences: |d h| <= s_r^2 S0 x 0.5 S2 per draw against no keys (Cauchy-Schwarz on
        0.5 s_r^2 (sum |y| / sigma^2)^2), computed per draw in the test;
  an OU realisation added to dataset 1, the matching keys, against the CPU oracle's model grid reduced with
        _numerics.ou_halfchi2: |d lnZ| <= 1e-9, the bar of the offset's and the baseline's oracle checks;
  three chunks of the grid, and calc_probs_datasets_refined(n_adapt = 0): the same bits.
"""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from test_gpu_datasets import KW, KW2, LC, SEED, TARGET_SHARE, _target, _two_cadences, device_mode  # noqa: F401
from triceratops_amd import _lib, _numerics, fused
from triceratops_amd.datasets import Datasets, ou_system, validate

pytestmark = pytest.mark.gpu

INF = float("inf")
SIGMA_BAR = Datasets(validate(_two_cadences())).sigma_ref          # of the input, the target's normalisation
SIGMA_1 = Datasets(validate(_two_cadences()[1:])).sigma_ref        # sigma_bar of dataset 1 alone
CADENCE_1 = float(np.median(np.diff(_two_cadences()[1]["time"])))
COLS = ("M_s", "R_s", "P_orb", "inc", "b", "ecc", "w", "R_p", "M_EB", "R_EB")


def _inputs(**keys):
    a, b = _two_cadences()
    return [a, dict(b, **keys)]


class _Spy:
    """per evidence of a pass, in order: h as the evidence saw it, h with nothing marginalised and white noise (the same
    rows evaluated again with the plain reduction), the draws' priors; and the calls of _lib.chi2_grid_ou"""

    def __init__(self, monkeypatch, replay):
        self.h, self.plain, self.lp, self.ou_calls = [], [], [], 0
        real_h, real_z, real_ou = fused._Scenario._datasets_halfchi2, _lib.lnz_from_halfchi2, _lib.chi2_grid_ou
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
            spy.lp.append(None if lp_d is None else lp_d.cpu().numpy())
            return real_z(h_d, lp_d, n_total, lnsigma)

        def ou(*a, **k):
            spy.ou_calls += 1
            return real_ou(*a, **k)

        monkeypatch.setattr(fused._Scenario, "_datasets_halfchi2", halfchi2)
        monkeypatch.setattr(_lib, "lnz_from_halfchi2", lnz)
        monkeypatch.setattr(_lib, "chi2_grid_ou", ou)


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
            "best": np.stack([tg.probs[c].values for c in COLS]), "target": tg, "h": s.h, "plain": s.plain, "lp": s.lp,
            "ou_calls": s.ou_calls}


_runs = {}


def _passes(monkeypatch):
    if not _runs:
        s = 3.0 * SIGMA_1
        _runs["none"] = _run(monkeypatch, _inputs())
        _runs["offset"] = _run(monkeypatch, _inputs(offset_sigma=s), replay=True)
        _runs["red_inf"] = _run(monkeypatch, _inputs(red_sigma=s, red_timescale=INF), replay=True)
    return _runs


def _same_bits(a, b):
    return (a["lnZ"].tobytes() == b["lnZ"].tobytes() and a["prob"].tobytes() == b["prob"].tobytes()
            and a["best"].tobytes() == b["best"].tobytes() and a["rows"] == b["rows"] > 0)


def test_without_the_keys_nothing_changes(device_mode, monkeypatch):
    a = _passes(monkeypatch)["none"]
    b = _run(monkeypatch, _inputs(red_sigma=None, red_timescale=None))
    assert np.isfinite(a["lnZ"]).sum() >= 10 and _same_bits(a, b)
    assert a["ou_calls"] == b["ou_calls"] == 0
    assert _passes(monkeypatch)["offset"]["ou_calls"] == 0 and _passes(monkeypatch)["red_inf"]["ou_calls"] > 0


def test_infinite_timescale_is_the_marginalised_offset(device_mode, monkeypatch):
    r = _passes(monkeypatch)
    u, s = r["offset"], r["red_inf"]
    d1 = validate(_inputs(red_sigma=3.0 * SIGMA_1, red_timescale=INF))[1]
    amp = 1.0 + 1.0 / (1.0 - ou_system(d1)[0].max())          # (alpha does not depend on the star's normalisation)
    assert len(s["h"]) == len(u["h"]) == len(s["plain"]) == s["lnZ"].size
    assert u["rows"] == s["rows"] == r["none"]["rows"] > 0, "masked counts differ"
    fin = np.isfinite(u["lnZ"])
    assert np.array_equal(fin, np.isfinite(s["lnZ"])) and fin.sum() >= 10
    # (the spy's lists hold one entry per evidence, in the rows' order: the finite rows and those without a finite draw)
    n_sep = n_same = 0
    worst = 0.0
    for j in np.flatnonzero(fin):
        h = s["h"][j]
        best = int(np.argmin(h))
        bar = 1e-12 * amp * s["plain"][j][best] + 1e-12
        d = abs(u["lnZ"][j] - s["lnZ"][j])
        worst = max(worst, d / bar)
        assert d <= bar, (j, d, bar)
        two = np.partition(h, 1)[:2] if h.size > 1 else np.array([h[0], np.inf])
        same = np.array_equal(u["best"][:, j], s["best"][:, j])
        if two[1] - two[0] > bar:
            n_sep += 1
            assert same, "row %d: best draws differ although the two smallest h are %g apart" % (j, two[1] - two[0])
        n_same += same
    print("tau = inf against offset_sigma: 1 + 1 / (1 - max alpha) = %.4g, max |d lnZ| / bar %.3g over %d finite rows; two "
          "smallest h further apart than the bar in %d rows, the same best draw in %d" % (amp, worst, fin.sum(), n_sep, n_same))
    assert fin.sum() - n_sep <= 0.25 * fin.sum()
    # the key changes the evidence: the point of the feature
    assert np.abs(s["lnZ"][fin] - r["none"]["lnZ"][fin]).max() > 1e-3


def test_tiny_red_sigma_is_white_noise(device_mode, monkeypatch):
    plain = _passes(monkeypatch)["none"]
    s_in = 1e-6 * SIGMA_BAR
    t = _run(monkeypatch, _inputs(red_sigma=s_in, red_timescale=10.0 * CADENCE_1), replay=True)
    assert t["ou_calls"] > 0
    fin = np.isfinite(plain["lnZ"])
    assert np.array_equal(fin, np.isfinite(t["lnZ"])) and t["rows"] == plain["rows"]
    # K = Sigma + s_r^2 R, R's entries in [0, 1]: 0 <= 0.5 y^T (Sigma^-1 - K^-1) y <= 0.5 s_r^2 (sum |y| / sigma^2)^2
    # <= s_r^2 S0 x 0.5 S2 <= s_r^2 S0 x (the draw's h under white noise).  s_r^2 S0 is the same in every star's
    # normalisation (Datasets.renorm).  + 1e-12 relative for the two reductions' rounding.
    d1 = validate(_inputs(red_sigma=s_in, red_timescale=1.0))[1]
    s2S0 = d1.red_sigma ** 2 * float(np.sum(1.0 / d1.flux_err ** 2))
    worst_bound = worst = 0.0
    for j in np.flatnonzero(fin):
        h, p, lp = t["h"][j], t["plain"][j], t["lp"][j]
        x = -p if lp is None else lp - p
        live = np.isfinite(x) & (x >= np.nanmax(np.where(np.isfinite(x), x, -np.inf)) - 80.0)
        assert live.any()
        bound = s2S0 * p[live] + 1e-12 * p[live]
        assert (np.abs(h[live] - p[live]) <= bound).all()
        worst_bound, worst = max(worst_bound, float(bound.max())), max(worst, float(np.abs(h[live] - p[live]).max()))
    d = np.abs(t["lnZ"][fin] - plain["lnZ"][fin]).max()
    print("tiny red_sigma: s_r^2 S0 = %.3g, computed bound on |d h| of the draws with weight %.3g, measured %.3g, "
          "max |d lnZ| %.3g" % (s2S0, worst_bound, worst, d))
    assert worst_bound <= 1e-6 and d <= worst_bound + 1e-12
    assert np.array_equal(t["best"], plain["best"])


def _ou_inputs():
    """dataset 1 with an OU realisation added (s_r = 2 sigma of dataset 1, tau = 20 cadences; a fixed seed) and its keys"""
    a, b = _two_cadences()
    s_r, tau = 2.0 * SIGMA_1, 20.0 * CADENCE_1
    rng = np.random.default_rng(465)
    t = b["time"]
    x = np.empty(t.size)
    x[0] = s_r * rng.normal()
    for n in range(1, t.size):
        phi = np.exp(-(t[n] - t[n - 1]) / tau)
        x[n] = phi * x[n - 1] + s_r * np.sqrt(1.0 - phi * phi) * rng.normal()
    return [a, dict(b, flux=b["flux"] + x, red_sigma=s_r, red_timescale=tau)]


def test_chunks_fused_refusal_and_refined(device_mode, monkeypatch):
    data = _ou_inputs()
    whole = _run(monkeypatch, data)
    assert whole["ou_calls"] > 0 and np.isfinite(whole["lnZ"]).sum() >= 10
    n_min = min(h.size for h in whole["h"] if h.size >= 3)
    # (a chunk of n_min // 3 rows of the longer dataset: every branch of at least n_min rows takes three chunks or more)
    with fused.switches(DATASET_GRID_BYTES=8 * 50 * (n_min // 3)):
        chunked = _run(monkeypatch, data)
    assert chunked["ou_calls"] >= 3 * sum(h.size >= 3 for h in whole["h"]) > whole["ou_calls"] // 2
    assert chunked["ou_calls"] > whole["ou_calls"]
    assert _same_bits(whole, chunked)
    assert _same_bits(whole, _run(monkeypatch, data, refined=True))
    tg = _target()
    with pytest.raises(NotImplementedError):
        tg.calc_probs_datasets(data, LC["P_orb"], evaluation="fused", **KW2)


def test_red_noise_evidence_against_the_oracle(device_mode, monkeypatch):
    """TP and EB (+ twin) of the target star on two cadences, errors varying 3x, an OU realisation and its keys on dataset
    1: the model curves from the oracle, the recurrence and the evidence in numpy."""
    data = _ou_inputs()
    kw = dict(KW2, drop_scenario=KW2["drop_scenario"] + ["PTP", "PEB"])
    tg = _target()
    dump = []
    monkeypatch.setattr(fused, "DUMP", dump)
    torch.manual_seed(SEED)
    tg.calc_probs_datasets(data, LC["P_orb"], **kw)
    monkeypatch.undo()
    assert len(dump) == 2
    ds = Datasets(validate(data)).renorm(float(TARGET_SHARE))
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
                if s.red_sigma is None:
                    h += 0.5 * np.sum(r * r / s.flux_err ** 2, axis=1)
                else:
                    h += _numerics.ou_halfchi2(r, *ou_system(s))
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
    assert ds.sets[0].red_sigma is None and ds.sets[1].red_sigma is not None
    assert np.array_equal(np.isfinite(want), np.isfinite(got)) and np.isfinite(want).sum() >= 2
    fin = np.isfinite(want)
    print("red-noise dataset against the oracle: max |d lnZ| %.3g" % np.abs(got[fin] - want[fin]).max())
    assert np.abs(got[fin] - want[fin]).max() <= 1e-9
