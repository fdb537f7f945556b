"""target.calc_probs_datasets_refined (DESIGN.md sections 12 and 14): adaptive importance sampling on the datasets path.

Exact: n_adapt = 0 is calc_probs_datasets; the identity grid is no grid; nothing persists after a refined call; a
refined run repeats from its seed in both evaluations; offsets and baselines go through.
Against the library's own chain: the first adaptation pass of one dataset with one error is calc_probs_refined's, to
the bound of tests/test_gpu_datasets.py::_check_same_evidence.
Statistical (seeds and run counts fixed before any run was looked at): unbiased under an arbitrary grid, by
tests/test_gpu_refined.py's criterion; on Kepler-10b the effective sample size grows and the scatter of lnZ shrinks."""
import time as _time

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from test_gpu_datasets import CC, DROP, LC, LNZ_TOL, SEED, _target, _two_cadences, _weights_spy, device_mode  # noqa: F401
from test_gpu_refined import N_UNBIASED, _EveryUnit, _synthetic, _wrong_grid
from test_gpu_refined import _target as _anchor_target

pytestmark = pytest.mark.gpu

KW = dict(contrast_curve_file=CC, N=20000, parallel=True, verbose=0, drop_scenario=DROP)
P = LC["P_orb"]


def _state(tg, posterior=False):
    cols = ("M_s", "R_s", "P_orb", "inc", "b", "ecc", "w", "R_p", "M_EB", "R_EB", "prob")
    parts = [np.asarray(getattr(tg, k), dtype=np.float64) for k in ("lnZ", "ess", "lnZ_err", "w_max_frac")]
    parts += [tg.probs[c].values.astype(np.float64) for c in cols]
    parts += [np.array([tg.FPP, tg.NFPP, tg.FPP_err, tg.NFPP_err, tg.sigma_ref], dtype=np.float64)]
    if posterior:
        for p in tg.posterior:
            parts += [np.zeros(1)] if p is None else [np.asarray(p[k], dtype=np.float64) for k in sorted(p)]
    return np.concatenate(parts).tobytes()


_plain = {}


def _plain_state():
    """calc_probs_datasets on the two cadences with 200 posterior samples from SEED, made once"""
    if not _plain:
        tg = _target()
        torch.manual_seed(SEED)
        tg.calc_probs_datasets(_two_cadences(), P, n_samples=200, **KW)
        _plain["state"] = _state(tg, posterior=True)
        _plain["fin"] = int(np.isfinite(tg.lnZ).sum())
        assert _plain["fin"] >= 4 and sum(p is not None for p in tg.posterior) == _plain["fin"]
    return _plain["state"]


# ---- exact -----------------------------------------------------------------------------------------------------------
def test_n_adapt_zero_is_calc_probs_datasets(device_mode):
    plain = _plain_state()
    tg = _target()
    torch.manual_seed(SEED)
    tg.calc_probs_datasets_refined(_two_cadences(), P, n_adapt=0, n_samples=200, **KW)
    assert _state(tg, posterior=True) == plain
    assert len(tg.refine_history) == 1 and np.array_equal(tg.refine_history[0]["lnZ"], tg.lnZ)


def test_identity_grid_is_no_grid(device_mode):
    from triceratops_amd import fused
    plain = _plain_state()
    tg = _target()
    with fused.switches(WARP_GRIDS=_EveryUnit(fused.warp_identity())):
        torch.manual_seed(SEED)
        tg.calc_probs_datasets(_two_cadences(), P, n_samples=200, **KW)
    assert _state(tg, posterior=True) == plain


def test_nothing_persists_after_a_refined_call(device_mode):
    from triceratops_amd import fused
    plain = _plain_state()
    tg = _target()
    torch.manual_seed(5)
    tg.calc_probs_datasets_refined(_two_cadences(), P, n_adapt=2, N_adapt=10000, n_samples=50, **KW)
    assert len(tg.refine_history) == 3
    assert fused.WARP_GRIDS is None and fused.DATASET_WARP_HIST is None and fused.POSTERIOR_ROWS == 0
    assert fused.WARP_HIST is False and fused.DATASET_OFFSETS is None and fused.DATASET_BASELINES is None
    torch.manual_seed(SEED)
    tg.calc_probs_datasets(_two_cadences(), P, n_samples=200, **KW)
    assert _state(tg, posterior=True) == plain


@pytest.mark.parametrize("evaluation", ["grid", "fused"])
def test_refined_repeats_from_its_seed(evaluation, device_mode):
    tg = _target()
    states = []
    for _ in range(2):
        torch.manual_seed(31)
        tg.calc_probs_datasets_refined(_two_cadences(), P, n_adapt=2, n_samples=100, evaluation=evaluation, **KW)
        states.append(_state(tg, posterior=True))
    assert states[0] == states[1]
    assert len(tg.refine_history) == 3
    for h in tg.refine_history:
        assert h["lnZ"].shape == h["ess"].shape == h["w_max_frac"].shape == tg.lnZ.shape
    assert np.array_equal(tg.refine_history[-1]["lnZ"], tg.lnZ)
    assert not np.array_equal(tg.refine_history[0]["lnZ"], tg.lnZ)
    fin = np.isfinite(tg.lnZ)
    # (FPP = 1 - the planet rows' share: within rounding of [0, 1])
    assert fin.sum() >= 4 and abs(tg.probs["prob"].sum() - 1.0) < 1e-12 and -1e-12 <= tg.FPP <= 1.0
    for j in range(tg.lnZ.size):
        assert (tg.posterior[j] is not None) == bool(fin[j])
    print("\n%s: TP ess per pass:" % evaluation, [float(h["ess"][0]) for h in tg.refine_history])


def test_the_two_evaluations_adapt_alike(device_mode):
    """the histogram is fed the same way by both: the first adaptation pass, whose draws are unmapped in both, gives the
    same evidences to the evaluations' own rounding (1e-12 relative in chi^2/2; LNZ_TOL is the suite's absolute bar on
    lnZ)"""
    tg = _target()
    first = {}
    for evaluation in ("grid", "fused"):
        torch.manual_seed(31)
        tg.calc_probs_datasets_refined(_two_cadences(), P, n_adapt=1, evaluation=evaluation, **KW)
        first[evaluation] = tg.refine_history[0]["lnZ"]
    fin = np.isfinite(first["grid"])
    assert np.array_equal(fin, np.isfinite(first["fused"]))
    assert np.abs(first["grid"][fin] - first["fused"][fin]).max() < LNZ_TOL


def test_offsets_and_baselines_go_through(device_mode):
    from triceratops_amd.lightcurve import polynomial_baseline
    a, b = _two_cadences()
    a = dict(a, offset_sigma=float("inf"))
    b = dict(b, baseline=polynomial_baseline(b["time"], 1)[0])
    tg = _target()
    torch.manual_seed(31)
    tg.calc_probs_datasets_refined([a, b], P, n_adapt=2, N_adapt=10000, **KW)
    fin = np.isfinite(tg.lnZ)
    assert fin.sum() >= 4 and len(tg.refine_history) == 3
    assert tg.dataset_offsets.shape == (tg.lnZ.size, 2)
    assert np.array_equal(np.isfinite(tg.dataset_offsets[:, 0]), fin) and np.isnan(tg.dataset_offsets[:, 1]).all()
    assert len(tg.dataset_baselines) == tg.lnZ.size
    for j, per in enumerate(tg.dataset_baselines):
        assert per[0] is None and per[1].shape == (1,) and bool(np.isfinite(per[1]).all()) == bool(fin[j])


# ---- against the library's own chain -------------------------------------------------------------------------------------
def test_first_pass_is_the_native_first_pass(device_mode, monkeypatch):
    """one dataset, one error for all points, the same seed: pass 0 of both loops draws the same unmapped draws, so its
    evidences agree within B = 1e-12 h_max + 1e-12 per row (tests/test_gpu_datasets.py::_check_same_evidence) and its
    effective sample sizes within 4 B relative: ln ess = ln N + 2 lnZ - lnM2, and lnM2 sees twice the shift of x.
    (Later passes draw under grids that differ in their last bits: the statistical tests below cover them.)"""
    from triceratops_amd import _lib, fused, sharding
    tg = _target()
    torch.manual_seed(SEED)
    tg.calc_probs_refined(LC["time"], LC["flux"], LC["sigma"], P, n_adapt=1, **KW)
    native = tg.refine_history[0]
    # h_max per scenario row: per evidence of the datasets pass, filed under the work unit that formed it
    seen, units = {}, []
    real_lnz, real_run = _lib.lnz_from_halfchi2, sharding.run_units
    flat = _weights_spy(monkeypatch)                # (_lib.lnz_from_halfchi2 now appends the h_max of every evidence)
    spied = _lib.lnz_from_halfchi2

    def by_unit(h_d, lp_d, n_total, lnsigma):
        out = spied(h_d, lp_d, n_total, lnsigma)
        seen.setdefault(getattr(fused._tls, "unit", None), []).append(flat[-1])
        return out

    def keep_units(us, **kw):
        units.append(sharding.as_units(us))
        return real_run(us, **kw)

    monkeypatch.setattr(_lib, "lnz_from_halfchi2", by_unit)
    monkeypatch.setattr(sharding, "run_units", keep_units)
    one = [{"time": LC["time"], "flux": LC["flux"], "flux_err": LC["sigma"]}]
    torch.manual_seed(SEED)
    tg.calc_probs_datasets_refined(one, P, n_adapt=1, **KW)
    monkeypatch.undo()
    assert _lib.lnz_from_halfchi2 is real_lnz and sharding.run_units is real_run
    mine = tg.refine_history[0]
    assert len(units) == 2 and len(tg.refine_history) == 2
    hmax = np.zeros(tg.lnZ.size)
    for k, u in enumerate(units[0]):
        if u.thunk is not None:
            assert len(seen[k]) == 2 * len(u.names)                      # the adaptation pass, then the final one
            hmax[u.first_row:u.first_row + len(u.names)] = seen[k][:len(u.names)]
    fin = np.isfinite(native["lnZ"])
    assert np.array_equal(fin, np.isfinite(mine["lnZ"])) and fin.sum() >= 4
    B = 1e-12 * hmax[fin] + 1e-12
    d = np.abs(mine["lnZ"][fin] - native["lnZ"][fin])
    r = np.abs(mine["ess"][fin] - native["ess"][fin]) / native["ess"][fin]
    print("\npass 0 against the native pass: max |d lnZ| %.3g (%.3g of its bound), max relative |d ess| %.3g (%.3g of its bound)"
          % (d.max(), (d / B).max(), r.max(), (r / (4 * B)).max()))
    assert (d <= B).all(), (d, B)
    assert (r <= 4 * B).all(), (r, 4 * B)


# ---- statistical ---------------------------------------------------------------------------------------------------------
def _split(t, flux, sigma):
    """a light curve as its even and odd points, two datasets, the error as per-point arrays"""
    return [{"time": t[k::2], "flux": flux[k::2], "flux_err": np.full(t[k::2].size, float(sigma))} for k in (0, 1)]


N_WRONG = 1_000_000


def test_unbiased_under_an_arbitrary_grid(device_mode):
    """tests/test_gpu_refined.py::test_unbiased_under_an_arbitrary_grid on the datasets path: its wrong grid, its
    N_UNBIASED seeds, its criterion (|z| < 4 on the mean of lnZ per row) and its precondition on the plain runs
    (w_max_frac < 0.05), on its synthetic curve given as an even / odd split with per-point errors -- by
    test_split_light_curve_is_the_same_evidence the plain side is calc_probs' evidence to rounding, so the precondition
    carries over.  N is that test's 1e6 (were the test to exceed about ten seconds, N would be lowered, not the number
    of seeds)."""
    from triceratops_amd import fused
    tg, (t, flux, sigma, P_orb), kw = _synthetic()
    data = _split(t, flux, sigma)
    plain, wrong, wmax, ess_wrong = [], [], [], []
    t0 = _time.time()
    for s in range(N_UNBIASED):
        torch.manual_seed(4000 + s)
        tg.calc_probs_datasets(data, P_orb, N=N_WRONG, **kw)
        plain.append(np.array(tg.lnZ))
        wmax.append(np.array(tg.w_max_frac))
        with fused.switches(WARP_GRIDS=_EveryUnit(_wrong_grid())):
            torch.manual_seed(9000 + s)
            tg.calc_probs_datasets(data, P_orb, N=N_WRONG, **kw)
        wrong.append(np.array(tg.lnZ))
        ess_wrong.append(np.array(tg.ess))
    print("\n%d + %d passes of %d draws: %.1f s" % (N_UNBIASED, N_UNBIASED, N_WRONG, _time.time() - t0))
    plain, wrong, wmax = np.array(plain), np.array(wrong), np.array(wmax)
    print("wrong grid, median ess per row:", np.round(np.median(np.array(ess_wrong), axis=0), 1))
    fin = np.all(np.isfinite(plain), axis=0) & np.all(np.isfinite(wrong), axis=0)
    assert fin.sum() >= 10
    print("plain w_max_frac, largest per row:", np.round(np.nanmax(wmax, axis=0), 4))
    assert np.nanmax(wmax[:, fin]) < 0.05                               # the property of the PLAIN runs this test rests on
    se = np.sqrt(plain.var(axis=0, ddof=1) / N_UNBIASED + wrong.var(axis=0, ddof=1) / N_UNBIASED)
    z = (wrong.mean(axis=0) - plain.mean(axis=0)) / se
    for j in np.flatnonzero(fin):
        print("row %2d lnZ plain %.4f +- %.4f  wrong grid %.4f +- %.4f  z %.2f" % (j, plain[:, j].mean(),
              plain[:, j].std(ddof=1), wrong[:, j].mean(), wrong[:, j].std(ddof=1), z[j]))
    assert np.all(np.abs(z[fin]) < 4.0), z


KEP10_SEEDS = range(3000, 3008)          # 8 seeds, fixed before looking
N_KEP10 = 1_000_000


def test_refinement_does_what_it_is_for_on_kepler10(device_mode):
    """Kepler-10b as an even / odd split: two adaptation passes and a final pass of N draws against plain
    calc_probs_datasets at the same total, 3 N.  Strict inequalities, no measured bar: the median effective sample size
    of the TP row is larger and the scatter of its lnZ smaller.  (The native path's gains at 16 seeds: 35 and 10.7,
    profiles/warp/results.txt.)"""
    tg, (t, flux, sigma, P_orb), kw = _anchor_target("kep10")
    data = _split(np.asarray(t, dtype=np.float64), np.asarray(flux, dtype=np.float64), sigma)
    lnZ_r, ess_r, lnZ_p, ess_p, wmax_p = [], [], [], [], []
    t0 = _time.time()
    for s in KEP10_SEEDS:
        torch.manual_seed(s)
        tg.calc_probs_datasets_refined(data, P_orb, n_adapt=2, N=N_KEP10, **kw)
        lnZ_r.append(tg.lnZ[0])
        ess_r.append(tg.ess[0])
        if s == KEP10_SEEDS[0]:
            for k, h in enumerate(tg.refine_history):
                print("\nseed %d pass %d: TP lnZ %.4f ess %.1f w_max_frac %.3f" % (s, k, h["lnZ"][0], h["ess"][0], h["w_max_frac"][0]))
    t1 = _time.time()
    for s in KEP10_SEEDS:
        torch.manual_seed(s)
        tg.calc_probs_datasets(data, P_orb, N=3 * N_KEP10, **kw)
        lnZ_p.append(tg.lnZ[0])
        ess_p.append(tg.ess[0])
        wmax_p.append(tg.w_max_frac[0])
    t2 = _time.time()
    sd_r, sd_p = np.std(lnZ_r, ddof=1), np.std(lnZ_p, ddof=1)
    me_r, me_p = np.median(ess_r), np.median(ess_p)
    print("Kepler-10b TP, datasets path, %d seeds, N = %d: lnZ scatter plain (3 N) %.4f, refined %.4f: gain %.2f; median ess "
          "plain %.1f, refined %.1f: gain %.2f; plain median w_max_frac %.3f; refined runs %.1f s, plain runs %.1f s"
          % (len(KEP10_SEEDS), N_KEP10, sd_p, sd_r, sd_p / sd_r, me_p, me_r, me_r / me_p, np.median(wmax_p), t1 - t0, t2 - t1))
    assert me_r > me_p
    assert sd_r < sd_p
