"""target.calc_probs_refined: adaptive importance sampling of every evidence.

Exact: n_adapt = 0 is calc_probs; nothing persists after a refined call; a refined run repeats from its seed.
Statistical (run counts fixed before any run was looked at): the estimate is unbiased under an arbitrary grid; the
refined evidences agree with the reference's own runs (tests/golden/reference_runs.npz) by the criterion the anchors
test uses for calc_probs; on Kepler-10b, where plain sampling lives off one draw, the scatter of lnZ shrinks."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import anchors
from helpers import gold

pytestmark = pytest.mark.gpu


def _target(case):
    from triceratops_amd.triceratops import target
    c = anchors.CASES[case]
    stars, t, f, sigma, P = anchors.inputs(case)
    tg = target(c["ID"], np.array([1]), mission=c["mission"], stars=stars, trilegal_fname=anchors.TRILEGAL)
    return tg, (t, f, sigma, P), dict(contrast_curve_file=c["cc"], parallel=True, verbose=0)


class _device:
    def __enter__(self):
        import triceratops_amd
        self.prev = triceratops_amd.get_sampling()
        triceratops_amd.set_sampling("device")

    def __exit__(self, *exc):
        import triceratops_amd
        triceratops_amd.set_sampling(self.prev)


def _state(tg):
    cols = ("M_s", "R_s", "P_orb", "inc", "b", "ecc", "w", "R_p", "M_EB", "R_EB", "prob")
    parts = [np.asarray(getattr(tg, k), dtype=np.float64) for k in ("lnZ", "ess", "lnZ_err", "w_max_frac")]
    parts += [tg.probs[c].values.astype(np.float64) for c in cols]
    parts += [np.array([tg.FPP, tg.NFPP, tg.FPP_err, tg.NFPP_err], dtype=np.float64)]
    return np.concatenate(parts).tobytes()


# ---- exact -----------------------------------------------------------------------------------------------------------
def test_n_adapt_zero_is_calc_probs_and_nothing_persists():
    from triceratops_amd import _lib, fused
    _lib.require_gpu()
    tg, call, kw = _target("toi465_cc")
    with _device():
        torch.manual_seed(77)
        tg.calc_probs(*call, N=100_000, **kw)
        plain = _state(tg)
        torch.manual_seed(77)
        tg.calc_probs_refined(*call, n_adapt=0, N=100_000, **kw)
        assert _state(tg) == plain and len(tg.refine_history) == 1
        assert np.array_equal(tg.refine_history[0]["lnZ"], tg.lnZ)
        # a refined call in between leaves no trace: the same seed gives the same bits afterwards
        torch.manual_seed(5)
        tg.calc_probs_refined(*call, n_adapt=2, N_adapt=50_000, N=100_000, **kw)
        assert fused.WARP_GRIDS is None and fused.WARP_HIST is False and fused.POSTERIOR_ROWS == 0
        torch.manual_seed(77)
        tg.calc_probs(*call, N=100_000, **kw)
        assert _state(tg) == plain


def test_refined_repeats_from_its_seed_fills_the_target_and_the_posterior():
    from triceratops_amd import _lib
    _lib.require_gpu()
    tg, call, kw = _target("toi465_cc")
    with _device():
        states = []
        for _ in range(2):
            torch.manual_seed(31)
            tg.calc_probs_refined(*call, n_adapt=2, N=100_000, n_samples=500, **kw)
            states.append(_state(tg))
        assert states[0] == states[1]
        assert len(tg.refine_history) == 3
        for h in tg.refine_history:
            assert h["lnZ"].shape == h["ess"].shape == h["w_max_frac"].shape == tg.lnZ.shape
        assert np.array_equal(tg.refine_history[-1]["lnZ"], tg.lnZ)
        assert not np.array_equal(tg.refine_history[0]["lnZ"], tg.lnZ)
        fin = np.isfinite(tg.lnZ)
        assert fin.sum() >= 10 and abs(tg.probs["prob"].sum() - 1.0) < 1e-12 and 0.0 <= tg.FPP <= 1.0
        for j in range(tg.lnZ.size):
            assert (tg.posterior[j] is not None) == bool(fin[j])
            if fin[j]:
                assert tg.posterior[j]["R_p"].shape == (500,)
        # the adaptation does what it is for on the rows that carry the table: the effective sample size of the TP row grows
        print("\nTP ess per pass:", [float(h["ess"][0]) for h in tg.refine_history])
        # the numpy modes stage their uniforms
        import triceratops_amd
        triceratops_amd.set_sampling("numpy-device")
        with pytest.raises(NotImplementedError):
            tg.calc_probs_refined(*call, n_adapt=1, N=20_000, **kw)
        triceratops_amd.set_sampling("device")


# ---- statistical -----------------------------------------------------------------------------------------------------
class _EveryUnit(dict):
    """fused.WARP_GRIDS that hands every work unit the same grid"""

    def __init__(self, grid):
        super().__init__()
        self.grid = grid

    def get(self, unit, default=None):
        return self.grid


def _wrong_grid():
    """Deliberately wrong: in every dimension 45 % of the proposal sits in [51/64, 53/64) -- off the posterior of every
    scenario (small planets and companions, inclinations near 90 degrees: uniforms near 0) -- and the rest is spread
    evenly (well above the density floor of 0.1).  Everywhere else the proposal's density is rho = 0.55, and ln J
    varies between ln(1 / 0.55) = 0.6 there and -2.7 inside the band: a slot left out of ln J, a sign error or a J added
    before the clamp moves lnZ by tenths, against standard errors of a few 1e-3.

    Why not denser in the band: the criterion is the MEAN OF lnZ, and ln of an unbiased estimate is biased by
    -1 / (2 ess) (Jensen).  Against the standard error of a 32-run mean, (1 / sqrt(ess)) / sqrt(32), that bias is
    2.8 / sqrt(ess) standard errors: it needs ess >~ 50 under the wrong grid to stay below half a standard error.  A
    scenario consumes k = 4 or 5 mapped uniforms, so the wrong grid leaves about ess_plain rho^k; the plain rows here
    have ess of a few thousand (w_max_frac < 1e-3), hence rho^5 >~ 0.01, rho >~ 0.4.  (With rho = 0.1 -- all but the floor
    in the band -- rho^5 = 1e-5 leaves a handful of effective draws: the binary rows' lnZ then scatter by 1.0 per run and
    their mean sits 0.6-1.3 low, Jensen's -var/2, while the planet rows still agree.)"""
    from triceratops_amd import _numerics as nm
    B = nm.WARP_BINS
    rho, lo, hi = 0.55, 51 / B, 53 / B
    knots = np.array([0.0, lo, hi, 1.0])
    F = np.array([0.0, rho * lo, 1.0 - rho * (1.0 - hi), 1.0])          # the proposal's CDF: u -> y
    row = np.interp(np.arange(B + 1) / B, F, knots)
    row[0], row[-1] = 0.0, 1.0
    dens = 1.0 / (B * np.diff(row))
    assert np.all(np.diff(row) > 0) and 0.1 < 0.5 < dens.min() < 0.56 and dens.max() > 10.0
    return np.tile(row, (nm.WARP_DIMS, 1))


def _synthetic():
    """a noise-free shallow transit under a large error bar on TOI-411.02's star table and time stamps: the posterior
    is broad against the prior, so plain sampling is well behaved and its reported errors mean something"""
    tg, (t, f, sigma, P), kw = _target("toi411")
    t = np.asarray(t, dtype=np.float64)
    flux = np.ones_like(t)
    flux[np.abs(t) < 0.04] -= 3e-4
    return tg, (t, flux, 1.5e-3, P), kw


N_UNBIASED = 32           # seeds; fixed before looking


def test_unbiased_under_an_arbitrary_grid():
    from triceratops_amd import _lib, fused
    _lib.require_gpu()
    tg, call, kw = _synthetic()
    plain, wrong, wmax, ess_wrong = [], [], [], []
    with _device():
        for s in range(N_UNBIASED):
            torch.manual_seed(4000 + s)
            tg.calc_probs(*call, N=1_000_000, **kw)
            plain.append(np.array(tg.lnZ))
            wmax.append(np.array(tg.w_max_frac))
            fused.WARP_GRIDS = _EveryUnit(_wrong_grid())
            try:
                torch.manual_seed(9000 + s)
                tg.calc_probs(*call, N=1_000_000, **kw)
            finally:
                fused.WARP_GRIDS = None
            wrong.append(np.array(tg.lnZ))
            ess_wrong.append(np.array(tg.ess))
    plain, wrong, wmax = np.array(plain), np.array(wrong), np.array(wmax)
    print("\nwrong grid, median ess per row:", np.round(np.median(np.array(ess_wrong), axis=0), 1))
    fin = np.all(np.isfinite(plain), axis=0) & np.all(np.isfinite(wrong), axis=0)
    assert fin.sum() >= 10
    print("\nplain w_max_frac, largest per row:", np.round(np.nanmax(wmax, axis=0), 4))
    # the property of the PLAIN runs this test rests on
    assert np.nanmax(wmax[:, fin]) < 0.05
    se = np.sqrt(plain.var(axis=0, ddof=1) / N_UNBIASED + wrong.var(axis=0, ddof=1) / N_UNBIASED)
    z = (wrong.mean(axis=0) - plain.mean(axis=0)) / se
    for j in np.flatnonzero(fin):
        print("%-6s lnZ plain %.4f +- %.4f  wrong grid %.4f +- %.4f  z %.2f" % (anchors.SCENARIOS[j], plain[:, j].mean(),
              plain[:, j].std(ddof=1), wrong[:, j].mean(), wrong[:, j].std(ddof=1), z[j]))
    assert np.all(np.abs(z[fin]) < 4.0), z


N_REF = 16


def welch(m1, s1, n1, m2, s2, n2):
    return (m1 - m2) / np.sqrt(s1 ** 2 / n1 + s2 ** 2 / n2)


def _refined_runs(case, seeds, **refine):
    tg, call, kw = _target(case)
    lnZ, fpp, ess, hist = [], [], [], []
    with _device():
        for s in seeds:
            torch.manual_seed(s)
            tg.calc_probs_refined(*call, N=1_000_000, **refine, **kw)
            lnZ.append(np.array(tg.lnZ))
            fpp.append(float(tg.FPP))
            ess.append(np.array(tg.ess))
            hist.append(tg.refine_history)
    return np.array(lnZ), np.array(fpp), np.array(ess), hist


@pytest.mark.parametrize("case", ["toi411", "toi465_nocc"])
def test_refined_agrees_with_runs_of_the_reference_code(case):
    from triceratops_amd import _lib
    _lib.require_gpu()
    R = gold("reference_runs.npz")
    lnZ, fpp, _, _ = _refined_runs(case, range(2000, 2000 + N_REF), n_adapt=2)
    cols = [anchors.SCENARIOS.index(s) for s in ("TP", "PTP", "STP")]
    ref_lnZ, ref_fpp = R[case + "_lnZ"], R[case + "_FPP"]
    t = [welch(lnZ[:, c].mean(), lnZ[:, c].std(ddof=1), N_REF, ref_lnZ[:, j].mean(), ref_lnZ[:, j].std(ddof=1), ref_lnZ.shape[0])
         for j, c in enumerate(cols)]
    t.append(welch(fpp.mean(), fpp.std(ddof=1), N_REF, ref_fpp.mean(), ref_fpp.std(ddof=1), ref_fpp.size))
    print("\n%s refined vs reference code: lnZ TP/PTP/STP %s +- %s, reference %s +- %s; FPP %.5f +- %.5f, reference %.5f +- %.5f; "
          "Welch t %s" % (case, lnZ[:, cols].mean(axis=0), lnZ[:, cols].std(axis=0, ddof=1), ref_lnZ.mean(axis=0),
                          ref_lnZ.std(axis=0, ddof=1), fpp.mean(), fpp.std(ddof=1), ref_fpp.mean(), ref_fpp.std(ddof=1), np.round(t, 2)))
    assert np.all(np.abs(t) < 3.0), t


# Kepler-10b: plain sampling lives off one draw on the TP row (w_max_frac 0.8-1.0).  Bars = half the gain measured
# against calc_probs at the same total number of draws, 3 N (profiles/warp/results.txt: scatter of lnZ_TP 2.317 -> 0.217,
# a gain of 10.7; median ess 1.5 -> 52.4, a gain of 35).
KEP10_SCATTER_GAIN_BAR = 5.3
KEP10_ESS_GAIN_BAR = 17.6


def test_refinement_shrinks_the_scatter_on_kepler10():
    from triceratops_amd import _lib
    _lib.require_gpu()
    seeds = range(3000, 3000 + N_REF)
    lnZ_r, _, ess_r, hist = _refined_runs("kep10", seeds, n_adapt=2)
    tg, call, kw = _target("kep10")
    lnZ_p, ess_p, wmax_p = [], [], []
    with _device():
        for s in seeds:
            torch.manual_seed(s)
            tg.calc_probs(*call, N=3_000_000, **kw)          # the same total number of draws
            lnZ_p.append(tg.lnZ[0])
            ess_p.append(tg.ess[0])
            wmax_p.append(tg.w_max_frac[0])
    sd_r, sd_p = lnZ_r[:, 0].std(ddof=1), np.std(lnZ_p, ddof=1)
    me_r, me_p = np.median(ess_r[:, 0]), np.median(ess_p)
    print("\nKepler-10b TP: lnZ scatter plain (3 N) %.4f, refined %.4f: gain %.2f; median ess plain %.1f, refined %.1f: gain %.2f; "
          "plain median w_max_frac %.3f" % (sd_p, sd_r, sd_p / sd_r, me_p, me_r, me_r / me_p, np.median(wmax_p)))
    for k, h in enumerate(hist[0]):
        print("seed %d pass %d: TP lnZ %.4f ess %.1f w_max_frac %.3f" % (seeds[0], k, h["lnZ"][0], h["ess"][0], h["w_max_frac"][0]))
    assert sd_r < sd_p
    assert sd_p / sd_r >= KEP10_SCATTER_GAIN_BAR
    assert me_r / me_p >= KEP10_ESS_GAIN_BAR
