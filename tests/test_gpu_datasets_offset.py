"""target.calc_probs_datasets with per-dataset baseline offsets marginalised (`offset_sigma`), end
to end on the fixtures of tests/test_gpu_datasets.py: TOI-465.01, two cadences, N = 20 000, set_sampling("device"), one
seed for every pass.

Bars, none of them chosen from results:
  no key / offset_sigma = None: the same bits;
  flat prior, dataset 1 shifted by 3 sigma_bar: |d lnZ| <= 1e-12 x (chi^2/2 of the shifted pass's best draw, unprofiled)
        + 1e-12 -- the kernel's bound on one draw's h (tests/test_gpu_chi2_offset.py); the best draw is the same wherever
        the row's two smallest sums of h differ by more than that;
  dataset_offsets: shifted - unshifted = 3 sigma_bar to 1e-9 relative where the best draw is the same;
  tight prior s = 1e-6 sigma_bar: |d lnZ| <= 1e-6, from |d h| <= 0.5 s^2 S1^2 (computed per draw in the test);
  against the CPU oracle: |d lnZ| <= 1e-9, the bar of tests/test_gpu_lnl_weighted.py.
"""
import numpy as np
import pytest
import torch

from oracle import oracle as O
from test_gpu_datasets import KW, KW2, LC, SEED, TARGET_SHARE, _target, _two_cadences, device_mode  # noqa: F401
from triceratops_amd import _lib, fused
from triceratops_amd.datasets import Datasets, validate

pytestmark = pytest.mark.gpu

INF = float("inf")
SIGMA_BAR = Datasets(validate(_two_cadences())).sigma_ref          # of the input, the target's normalisation
COLS = ("M_s", "R_s", "P_orb", "inc", "b", "ecc", "w", "R_p", "M_EB", "R_EB")


def _inputs(offset_sigma="absent", shift=0.0):
    a, b = _two_cadences()
    b = dict(b, flux=b["flux"] + shift)
    if offset_sigma != "absent":
        b["offset_sigma"] = offset_sigma
    return [a, b]


class _Spy:
    """per evidence of a pass, in order: h as the evidence saw it, h with no offset marginalised (the same rows evaluated
    again with the offsets switched off), the draws' priors"""

    def __init__(self, monkeypatch):
        self.h, self.plain, self.lp = [], [], []
        real_h, real_z = fused._Scenario._datasets_halfchi2, _lib.lnz_from_halfchi2
        spy = self

        def halfchi2(scen, model, flags, block):
            h = real_h(scen, model, flags, block)
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

        monkeypatch.setattr(fused._Scenario, "_datasets_halfchi2", halfchi2)
        monkeypatch.setattr(_lib, "lnz_from_halfchi2", lnz)


def _run(monkeypatch, datasets, spy=False, **kw):
    tg = _target()
    s = _Spy(monkeypatch) if spy else None
    torch.manual_seed(SEED)
    _lib.reset_stats()
    tg.calc_probs_datasets(datasets, LC["P_orb"], **dict(KW, **kw))
    rows = _lib.STATS["rows"]
    monkeypatch.undo()
    out = {"lnZ": tg.lnZ.copy(), "prob": tg.probs.prob.values.copy(), "rows": rows // (2 if spy else 1),
           "best": np.stack([tg.probs[c].values for c in COLS]), "offsets": tg.dataset_offsets, "target": tg,
           "sigma_ref": tg.sigma_ref}
    if spy:
        out.update(h=s.h, plain=s.plain, lp=s.lp)
        assert len(s.h) == len(s.plain) > 0          # (one per evidence, in the rows' order: a dropped scenario has none)
    return out


_runs = {}


def _passes(monkeypatch):
    if not _runs:
        _runs["none"] = _run(monkeypatch, _inputs())
        _runs["flat"] = _run(monkeypatch, _inputs(INF), spy=True)
        _runs["flat_shifted"] = _run(monkeypatch, _inputs(INF, 3.0 * SIGMA_BAR), spy=True)
        _runs["none_shifted"] = _run(monkeypatch, _inputs(shift=3.0 * SIGMA_BAR))
    return _runs


def test_without_the_key_nothing_changes(device_mode, monkeypatch):
    a = _passes(monkeypatch)["none"]
    b = _run(monkeypatch, _inputs(None))
    assert a["offsets"] is None and b["offsets"] is None
    assert np.isfinite(a["lnZ"]).sum() >= 10 and a["rows"] == b["rows"] > 0
    assert a["lnZ"].tobytes() == b["lnZ"].tobytes() and a["prob"].tobytes() == b["prob"].tobytes()
    assert a["best"].tobytes() == b["best"].tobytes()


def test_flat_offset_absorbs_a_shift_of_the_dataset(device_mode, monkeypatch):
    r = _passes(monkeypatch)
    u, s, plain, plain_s = r["flat"], r["flat_shifted"], r["none"], r["none_shifted"]
    assert len(s["h"]) == len(u["h"]) == s["lnZ"].size
    assert u["rows"] == s["rows"] == plain["rows"] > 0, "masked counts differ"
    fin = np.isfinite(u["lnZ"])
    assert np.array_equal(fin, np.isfinite(s["lnZ"])) and fin.sum() >= 10
    n_same = n_sep = 0
    worst = 0.0
    for j in np.flatnonzero(fin):
        h = s["h"][j]
        best = int(np.argmin(h))
        bar = 1e-12 * s["plain"][j][best] + 1e-12
        d = abs(u["lnZ"][j] - s["lnZ"][j])
        worst = max(worst, d / bar)
        assert d <= bar, (j, d, bar)
        two = np.partition(h, 1)[:2] if h.size > 1 else np.array([h[0], np.inf])
        same = np.array_equal(u["best"][:, j], s["best"][:, j])
        if two[1] - two[0] > bar:
            n_sep += 1
            assert same, "row %d: best draws differ although the two smallest h are %g apart" % (j, two[1] - two[0])
        n_same += same
    print("flat offset, shift 3 sigma_bar: max |d lnZ| / bar %.3g over %d finite rows; two smallest h further apart than "
          "the bar in %d rows, the same best draw in %d" % (worst, fin.sum(), n_sep, n_same))
    assert n_sep >= 0.9 * fin.sum()
    # without the key the same shift moves the evidence of the best-fitting row by more than 1: the point of the feature
    top = int(np.nanargmax(np.where(np.isfinite(plain["lnZ"]), plain["lnZ"], -np.inf)))
    moved = abs(plain["lnZ"][top] - plain_s["lnZ"][top])
    print("no offset_sigma: lnZ of row %d moves by %.4g under the same shift" % (top, moved))
    assert moved > 1.0


def test_dataset_offsets_recover_the_shift(device_mode, monkeypatch):
    r = _passes(monkeypatch)
    u, s = r["flat"], r["flat_shifted"]
    n_scen = u["lnZ"].size
    assert u["offsets"].shape == s["offsets"].shape == (n_scen, 2)
    assert np.isnan(u["offsets"][:, 0]).all() and np.isnan(s["offsets"][:, 0]).all()        # dataset 0 has no offset
    fin = np.isfinite(u["lnZ"])
    assert np.array_equal(np.isfinite(u["offsets"][:, 1]), fin) and np.array_equal(np.isfinite(s["offsets"][:, 1]), fin)
    same = fin & np.array([np.array_equal(u["best"][:, j], s["best"][:, j]) for j in range(n_scen)])
    assert same.sum() >= 0.9 * fin.sum()
    d = s["offsets"][same, 1] - u["offsets"][same, 1]
    rel = np.abs(d - 3.0 * SIGMA_BAR) / (3.0 * SIGMA_BAR)
    print("dataset_offsets: shifted - unshifted against 3 sigma_bar, max relative error %.3g over %d rows; the unshifted "
          "offsets span %.3g .. %.3g sigma_bar" % (rel.max(), same.sum(), u["offsets"][fin, 1].min() / SIGMA_BAR,
                                                   u["offsets"][fin, 1].max() / SIGMA_BAR))
    assert rel.max() <= 1e-9
    assert r["none"]["offsets"] is None


def test_tight_prior_is_no_offset(device_mode, monkeypatch):
    r = _passes(monkeypatch)
    s_in = 1e-6 * SIGMA_BAR
    t = _run(monkeypatch, _inputs(s_in), spy=True)
    plain = r["none"]
    fin = np.isfinite(plain["lnZ"])
    assert np.array_equal(fin, np.isfinite(t["lnZ"])) and t["rows"] == plain["rows"]
    assert len(t["h"]) == t["lnZ"].size
    # |d h| <= 0.5 s^2 S1^2 per draw, and S1^2 <= S0 S2 (Cauchy-Schwarz; the form of S1 <~ S0 |r|max that needs no guess
    # at the residuals): |d h| <= s^2 S0 x 0.5 S2 <= s^2 S0 x (the draw's h without offsets).  s^2 S0 is the same in every
    # star's normalisation (Datasets.renorm).  Only draws within 80 of the row's best log-weight enter lnZ (the reduction
    # drops the others: exp(-80)); their h is a few hundred at most, so the bound is ~1e-8 against the 1e-6 asked.
    d1 = validate(_inputs(s_in))[1]
    s2S0 = d1.offset_sigma ** 2 * float(np.sum(1.0 / d1.flux_err ** 2))
    worst_bound = worst = 0.0
    for j in np.flatnonzero(fin):
        h, p, lp = t["h"][j], t["plain"][j], t["lp"][j]
        x = -p if lp is None else lp - p
        live = np.isfinite(x) & (x >= np.nanmax(np.where(np.isfinite(x), x, -np.inf)) - 80.0)
        assert live.any()
        bound = s2S0 * p[live] + 1e-12 * p[live]              # (+ the two reductions' rounding: test_gpu_chi2_offset.py)
        assert (np.abs(h[live] - p[live]) <= bound).all()
        worst_bound, worst = max(worst_bound, float(bound.max())), max(worst, float(np.abs(h[live] - p[live]).max()))
    d = np.abs(t["lnZ"][fin] - plain["lnZ"][fin]).max()
    print("tight prior: s^2 S0 = %.3g, computed bound on |d h| of the draws with weight %.3g, measured %.3g, max |d lnZ| %.3g"
          % (s2S0, worst_bound, worst, d))
    assert worst_bound <= 1e-6 and d <= 1e-6
    assert np.array_equal(t["best"], plain["best"])


def test_fused_evaluation_is_refused_and_posteriors_follow_h(device_mode, monkeypatch):
    tg = _target()
    with pytest.raises(NotImplementedError):
        tg.calc_probs_datasets(_inputs(INF), LC["P_orb"], evaluation="fused", **KW2)
    tg.calc_probs_datasets(_inputs(None), LC["P_orb"], evaluation="fused", **KW2)          # no offset: as before
    assert np.isfinite(tg.lnZ).sum() >= 4 and tg.dataset_offsets is None
    p = _run(monkeypatch, _inputs(INF), spy=True, n_samples=50, **{k: v for k, v in KW2.items() if k != "N"})
    post = p["target"].posterior
    lnsig = float(np.log(p["sigma_ref"]))
    checked = 0
    assert len(p["h"]) == 6                                       # TP, EB, EBx2P, PTP, PEB, PEBx2P: rows 0 .. 5
    assert all(q is None for q in post[6:])
    for j, lnz in enumerate(p["lnZ"][:6]):
        if not np.isfinite(lnz):
            assert post[j] is None
            continue
        q = post[j]
        assert q is not None and q["lnw"].shape == (50,) and q["row"].min() >= 0 and q["row"].max() < p["h"][j].size
        x = -0.5 * np.log(2 * np.pi) - lnsig - p["h"][j][q["row"]]
        if p["lp"][j] is not None:
            x = x + p["lp"][j][q["row"]]
        assert np.abs(q["lnw"] - x).max() <= 1e-12 * np.abs(x).max() + 1e-12
        # the rows were weighted with the marginalised h, not the plain one
        assert np.abs(p["plain"][j][q["row"]] - p["h"][j][q["row"]]).max() > 0.0
        checked += 1
    assert checked >= 4


def test_offset_evidence_against_the_oracle(device_mode, monkeypatch):
    """TP and EB (+ twin) of the target star on two cadences, errors varying 3x, a flat offset on dataset 1 and a Gaussian
    one (s = 2 sigma_bar) on dataset 0: the model curves from the oracle, the sums and the evidence in numpy."""
    data = _two_cadences()
    data[0]["offset_sigma"], data[1]["offset_sigma"] = 2.0 * SIGMA_BAR, INF
    data[1]["flux"] = data[1]["flux"] + 3.0 * SIGMA_BAR
    kw = dict(KW2, drop_scenario=KW2["drop_scenario"] + ["PTP", "PEB"])
    tg = _target()
    dump = []
    monkeypatch.setattr(fused, "DUMP", dump)
    torch.manual_seed(SEED)
    tg.calc_probs_datasets(data, LC["P_orb"], **kw)
    monkeypatch.undo()
    assert len(dump) == 2
    ds = Datasets(validate(data)).renorm(float(TARGET_SHARE))
    want, chat = [], []
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
            c_rows = []
            for l, s in enumerate(ds.sets):
                grid, sec = O.flux_grid(model, s.time, block, exptime=s.exptime, nsamples=s.nsamples)
                w = 1.0 / s.flux_err ** 2
                r = s.flux - grid
                prec = 0.0 if np.isinf(s.offset_sigma) else 1.0 / s.offset_sigma ** 2
                S0, S1, S2 = np.sum(w), np.sum(w * r, axis=1), np.sum(w * r * r, axis=1)
                h += 0.5 * (S2 - S1 * S1 / (S0 + prec))
                c_rows.append(S1 / (S0 + prec))
                if l == 0 and model == O.MODEL_EB:
                    h[sec >= 1.5 * ds.sigma_ref] = np.inf
            x = -0.5 * np.log(2 * np.pi) - np.log(ds.sigma_ref) - h
            if lnprior is not None:
                x = x + lnprior[idx]
            full = np.full(m.size, -np.inf)
            full[idx] = x
            want.append(O.log_mean_exp(full, m.size))
            best = int(np.argmin(h)) if idx.size else 0
            chat.append([c[best] * float(TARGET_SHARE) if idx.size else np.nan for c in c_rows])
    want, chat = np.array(want), np.array(chat)
    got = tg.lnZ[:3]
    assert np.array_equal(np.isfinite(want), np.isfinite(got)) and np.isfinite(want).sum() >= 2
    fin = np.isfinite(want)
    print("offset datasets against the oracle: max |d lnZ| %.3g" % np.abs(got[fin] - want[fin]).max())
    assert np.abs(got[fin] - want[fin]).max() <= 1e-9
    # the best draw's offsets: an offset is a weighted mean of residuals, so two models that agree to ATOL_FLUX = 5e-13 in
    # every cell (tests/test_gpu_kernels.py) give offsets that agree to 5e-13 in the star's normalisation (x share <= 1);
    # + 1e-12 relative for the two orders of summation
    offs = tg.dataset_offsets[:3]
    print("best-draw offsets (sigma_bar):", (offs[fin] / SIGMA_BAR).tolist(), "oracle:", (chat[fin] / SIGMA_BAR).tolist(),
          "max difference %.3g" % np.abs(offs[fin] - chat[fin]).max())
    assert np.isfinite(offs[fin]).all() and np.isnan(offs[~fin]).all()
    assert (np.abs(offs[fin] - chat[fin]) <= 5e-13 + 1e-12 * np.abs(chat[fin])).all()
