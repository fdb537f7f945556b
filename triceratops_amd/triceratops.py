"""`target`: the calc_probs() driver of the reference, on the MI355X kernels.

Mirrors the compute half of triceratops/triceratops.py `class target`:
  calc_depths  (triceratops.py:559-671)   aperture flux ratios and per-star transit depths
  calc_probs   (triceratops.py:673-1485)  scenario loop, probability table, FPP / NFPP
with the same argument lists and the same result attributes (.probs .lnZ .FPP .NFPP
.FPP_degenerate .star_num .u1 .u2 .fluxratio_EB .fluxratio_comp).

and the data half of plot_fits:
  fit_curves (triceratops.py:1502-1597)   best-fit model light curve per scenario

Out of scope: the catalogue / cut-out / TRILEGAL web queries of
__init__, plot_field, the matplotlib figure of plot_fits and the star-table edits (plain pandas: edit
`target.stars` directly).  A `target` here is built from a ready star table (and, for
calc_depths, pixel coordinates); the TRILEGAL population is a local csv (`trilegal_fname`).

With torch.distributed initialised (one process per GPU, RCCL) calc_probs shards the
(star, lnZ_* call) units over the ranks and finishes with ONE all_gather of the per-scenario
results; see triceratops_amd/sharding.py.
"""
import warnings

import numpy as np
from pandas import DataFrame
from scipy.special import ndtr

from . import _lib
from ._numerics import _mc_errors, _normalize_probabilities
from .constants import G, Msun, pi
from .datasets import (Datasets, outliers as _outliers, red_baselines as _red_baselines, t0_grids as _t0_grids,
                       white_grids as _white_grids, white_baselines as _white_baselines,
                       red_kernel_baselines as _red_kernel_baselines,
                       validate as _validate_datasets)
from .funcs import renorm_flux
from .marginal_likelihoods import *  # noqa: F401,F403  (reference re-exports the lnZ_* names)
from .marginal_likelihoods import (lnZ_BEB, lnZ_BTP, lnZ_DEB, lnZ_DTP, lnZ_PEB, lnZ_PTP, lnZ_SEB,
                                   lnZ_STP, lnZ_TEB, lnZ_TTP)
from . import sharding

_COLS = ("M_s", "R_s", "u1", "u2", "P_orb", "inc", "b", "R_p", "ecc", "argp", "M_EB", "R_EB",
         "fluxratio_EB", "fluxratio_comp")
_POSTERIOR_PARAMS = _COLS        # the physical columns of a scenario's posterior samples (fused.POSTERIOR_KEYS less lnw, row)

# (drop key, scenario names, first row index, star_num) of the nine target-star calls, in the
# reference's order (triceratops.py:784-1340)
_TARGET_CALLS = (
    ("TP", ("TP",), 0, 1), ("EB", ("EB", "EBx2P"), 1, 1),
    ("PTP", ("PTP",), 3, 1), ("PEB", ("PEB", "PEBx2P"), 4, 1),
    ("STP", ("STP",), 6, 2), ("SEB", ("SEB", "SEBx2P"), 7, 2),
    ("DTP", ("DTP",), 9, 1), ("DEB", ("DEB", "DEBx2P"), 10, 1),
    ("BTP", ("BTP",), 12, 2), ("BEB", ("BEB", "BEBx2P"), 13, 2),
)

# (Datasets flag, wording) of what evaluation="fused" refuses, in the order in which a list of several kinds is answered
_FUSED_REFUSALS = (
    ("has_offsets", "an offset_sigma"), ("has_baselines", "a baseline"), ("has_red_baselines", "a red_baseline"),
    ("has_red_kernel_baselines", "a red_kernel_baseline"), ("has_red_noise", "a red_sigma or red_grid"),
    ("has_t0_grids", "a t0_grid"), ("has_white_grids", "a white_grid"), ("has_white_baselines", "a white_baseline"),
    ("has_outliers", "an outlier_frac"),
)


def _model_block(is_tp, comp, c):
    """(model, flags, [n_param][n] host block) of the light curves of n parameter sets of one kind -- is_tp: planets
    (else binaries), comp: the companion hosts the transit --, c: the per-set arrays under the names of _COLS.  Kepler's
    third law on M_s (planets) or M_s + M_EB (binaries) at P_orb as given (a twin row holds 2 P_orb), and the
    reference's scalar-path radius-ratio rule (likelihoods.py:63-66, 122-131)."""
    M = c["M_s"] + (0.0 if is_tp else c["M_EB"])
    P = c["P_orb"]
    a = ((G * M * Msun) / (4 * pi ** 2) * (P * 86400) ** 2) ** (1 / 3)
    common = (P, c["inc"], a, c["R_s"], c["u1"], c["u2"], c["ecc"], c["argp"], c["fluxratio_comp"])
    if is_tp:
        model, cols = _lib.MODEL_TP, (c["R_p"],) + common
    else:
        model, cols = _lib.MODEL_EB, (c["R_EB"], c["fluxratio_EB"]) + common
    flags = _lib.FLAG_SCALAR_K | (_lib.FLAG_COMPANION_IS_HOST if comp else 0)
    return model, flags, _lib.pack_params(model, cols, len(P))


class target:
    def __init__(self, ID: int, sectors=None, search_radius: int = 10, mission: str = "TESS",
                 lightkurve_cache_dir=None, trilegal_fname=None, ra: float = None,
                 dec: float = None, verify_ssl: bool = True, stars: DataFrame = None,
                 pix_coords=None):
        """ID, sectors, search_radius, mission, trilegal_fname as in the reference; `stars` is the
        table the reference builds from the TIC (columns ID Tmag Jmag Hmag Kmag ra dec mass rad
        Teff plx [sep PA fluxratio tdepth]); `pix_coords` the per-sector pixel positions of those
        stars (list of (n_stars, 2) arrays), needed by calc_depths only."""
        if mission != "TESS" and mission != "Kepler" and mission != "K2":
            raise ValueError("Introduced invalid mission: " + mission)
        if stars is None:
            raise NotImplementedError(
                "triceratops_amd.target needs a ready `stars` table: the MAST/TIC/TessCut/TRILEGAL "
                "queries of the reference constructor are outside the accelerated path")
        self.ID = ID
        self.mission = mission
        self.sectors = sectors
        self.search_radius = search_radius
        self.N_pix = 2 * search_radius + 2
        self.trilegal_fname = trilegal_fname
        self.trilegal_url = None
        self.stars = stars.reset_index(drop=True)
        self.pix_coords = pix_coords

    # -----------------------------------------------------------------------------------
    def calc_depths(self, tdepth: float, all_ap_pixels=None):
        """Flux share of every star in the extraction apertures (circular Gaussian PSF,
        sigma = 0.75 px, closed-form pixel integrals) and the transit depth each star would
        need to produce the observed depth `tdepth` (fractional, like the reference)."""
        if self.pix_coords is None:
            raise ValueError("calc_depths needs pix_coords")
        if all_ap_pixels is None:
            print("No apertures provided, assuming 5x5 centered on target.")
            all_ap_pixels = []
            for coords in self.pix_coords:
                c = np.round(coords[0])
                xs = np.arange(c[0] - 2, c[0] + 3, 1)
                ys = np.arange(c[1] - 2, c[1] + 3, 1)
                all_ap_pixels.append(np.array([np.repeat(xs, 5), np.tile(ys, 5)]).T)
        sigma = 0.75
        Tmag = self.stars.Tmag.values
        amp = 10 ** ((np.min(Tmag) - Tmag) / 2.5)
        ratios = np.zeros([len(all_ap_pixels), len(self.stars)])
        for k, ap in enumerate(all_ap_pixels):
            px = np.array(ap)
            mu = np.asarray(self.pix_coords[k])
            wx = (ndtr((px[:, None, 0] + 0.5 - mu[None, :, 0]) / sigma)
                  - ndtr((px[:, None, 0] - 0.5 - mu[None, :, 0]) / sigma))
            wy = (ndtr((px[:, None, 1] + 0.5 - mu[None, :, 1]) / sigma)
                  - ndtr((px[:, None, 1] - 0.5 - mu[None, :, 1]) / sigma))
            rel = amp * np.sum(wx * wy, axis=0)
            ratios[k, :] = rel / np.sum(rel)
        flux_ratios = np.mean(ratios, axis=0)
        self.stars["fluxratio"] = flux_ratios
        tdepths = np.zeros(len(self.stars))
        nz = flux_ratios != 0
        tdepths[nz] = 1 - (flux_ratios[nz] - tdepth) / flux_ratios[nz]
        tdepths[tdepths > 1] = 0
        self.stars["tdepth"] = tdepths
        filtered = self.stars[self.stars["tdepth"] > 0]
        for i, ID in enumerate(filtered["ID"].values):
            vals = [filtered[c].values[i] for c in ("mass", "rad", "Teff")]
            if i == 0:
                vals.append(filtered["plx"].values[i])
            if np.any(np.isnan(np.array(vals, dtype=float))):
                print("WARNING: " + str(ID) + " is missing stellar properties"
                      + (" required for validation." if i == 0
                         else ". Solar values will be assumed."))
        return

    # -----------------------------------------------------------------------------------
    def _units(self, filtered, flux_0, flux_err_0, time, P_orb, contrast_curve_file, filt, N,
               parallel, drop_scenario, flatpriors, exptime, nsamples, molusc_file, job=0):
        """The independent (star, lnZ_* call) work units of one calc_probs, in the reference's
        order: sharding.Unit, the thunk None for a dropped scenario.
        Building the list touches nothing but the star table's columns (once each): a unit's arguments --
        the light curve renormalised to its star, the argument tuples -- are put together when its thunk
        is called, i.e. only on the rank that owns it (sharding.run_units)."""
        units = []
        Unit, weight, draws = sharding.Unit, float(N) * max(1, time.size), int(N)      # (weight: the job's relative size)
        ok = True
        keep, stars, column = filtered
        cache = {}

        def col(c):
            """column c of the stars that can host the signal, on first use (a rank that does not own the target never
            asks for most of them)"""
            v = cache.get(c)
            if v is None:
                v = cache[c] = column(c)[keep]
            return v
        tail = (N, parallel, self.mission, flatpriors, exptime, nsamples)
        trilegal = self.trilegal_fname
        fns = {"TP": lnZ_TTP, "EB": lnZ_TEB, "PTP": lnZ_PTP, "PEB": lnZ_PEB, "STP": lnZ_STP, "SEB": lnZ_SEB,
               "DTP": lnZ_DTP, "DEB": lnZ_DEB, "BTP": lnZ_BTP, "BEB": lnZ_BEB}

        def star_args(i, cache={}):
            """(time, flux, flux_err, P_orb, M_s, R_s, Teff) of star i, built on first use"""
            if i not in cache:
                if isinstance(time, Datasets):
                    # (calc_probs_datasets: every dataset renormalised to the star; sigma is their sigma_bar)
                    ds = time.renorm(col("fluxratio")[i])
                    t_i, flux, flux_err = ds, None, ds.sigma_ref
                else:
                    t_i = time
                    flux, flux_err = renorm_flux(flux_0, flux_err_0, col("fluxratio")[i])
                M_s, R_s, Teff = col("mass")[i], col("rad")[i], col("Teff")[i]
                if i > 0:      # nearby star: unknown properties default to solar values
                    Teff = 5777 if np.isnan(Teff) else Teff
                    M_s = 1.0 if np.isnan(M_s) else M_s
                    R_s = 1.0 if np.isnan(R_s) else R_s
                cache[i] = (t_i, flux, flux_err, P_orb, M_s, R_s, Teff)
            return cache[i]

        def target_call(key):
            b, Z = star_args(0), 0.0
            if key in ("TP", "EB"):
                return fns[key](*b, Z, *tail)
            if key in ("PTP", "PEB", "STP", "SEB"):
                return fns[key](*b, Z, col("plx")[0], contrast_curve_file, filt, *tail, molusc_file)
            mags = (col("Tmag")[0], col("Jmag")[0], col("Hmag")[0], col("Kmag")[0])
            field = mags + (trilegal, contrast_curve_file, filt) + tail
            if key in ("DTP", "DEB"):
                return fns[key](*b, Z, *field)
            return fns[key](*b, *field)

        def nearby_call(i, fn):
            return fn(*star_args(i), 0.0, *tail)

        for i, ID in enumerate(stars["ID"].to_numpy()[keep]):
            if i == 0:
                if (np.isnan(col("mass")[0]) or np.isnan(col("rad")[0]) or np.isnan(col("Teff")[0])
                        or np.isnan(col("plx")[0])):
                    print("Insufficient information to validate " + str(ID)
                          + ". Please ensure a stellar mass (in M_Sun), radius (in R_Sun), Teff "
                          + "(in K), and plx (in mas) are provided in the .stars dataframe.")
                    ok = False
                    break
                for key, names, j0, snum in _TARGET_CALLS:
                    fn = None if key in drop_scenario else (lambda k=key: target_call(k))
                    units.append(Unit(j0, names, snum, ID, fn, key, weight, draws, (job, 0)))
            else:
                j0 = 15 + 3 * (i - 1)
                units.append(Unit(j0, ("NTP",), 1, ID, lambda i=i: nearby_call(i, lnZ_TTP), "NTP", weight, draws, (job, i)))
                units.append(Unit(j0 + 1, ("NEB", "NEBx2P"), 1, ID, lambda i=i: nearby_call(i, lnZ_TEB), "NEB", weight,
                                  draws, (job, i)))
        return units, ok

    def calc_probs(self, time, flux_0, flux_err_0: float, P_orb, contrast_curve_file: str = None,
                   filt: str = "TESS", N: int = 1000000, parallel: bool = False,
                   drop_scenario: list = [], verbose: int = 1, flatpriors: bool = False,
                   exptime: float = 0.00139, nsamples: int = 20, molusc_file: str = None):
        """Relative probability of every scenario, FPP and NFPP (same arguments as the reference).

        `parallel` selects the reference's vector-path or per-draw-loop semantics (App. C of
        SURVEY.md); both run on the GPU."""
        units, book = self._prepare(time, flux_0, flux_err_0, P_orb, contrast_curve_file, filt, N,
                                    parallel, drop_scenario, flatpriors, exptime, nsamples,
                                    molusc_file)
        self._finish(units, sharding.run_units(units, verbose=verbose, as_rows=True), book, layout=sharding.last_layout)
        return

    def calc_posteriors(self, time, flux_0, flux_err_0: float, P_orb, n_samples: int = 1000, **calc_probs_kwargs):
        """calc_probs with posterior samples: the same pass -- from the same seed `.probs`, `.lnZ`, `.FPP`, `.NFPP`, the
        best-draw columns and the error attributes are bit for bit those of calc_probs -- in which every lnZ_* call also
        draws n_samples of its draws in proportion to their weight in the evidence (systematic resampling on the
        device).  Fills `.posterior`: a list with one entry per scenario row -- a dict of
        [n_samples] arrays (M_s R_s u1 u2 P_orb inc b R_p ecc argp M_EB R_EB fluxratio_EB fluxratio_comp, "lnw" the
        draws' log-weights, "row" their positions among the call's masked draws), or None for a dropped scenario or one
        none of whose draws carries weight.  The samples of a row are equally weighted.  Needs a device sampling mode
        (set_sampling("device") or "numpy-device")."""
        from . import fused
        n_samples = int(n_samples)
        if not 1 <= n_samples <= fused.POST_MAX_ROWS:
            raise ValueError("n_samples must lie in [1, %d]" % fused.POST_MAX_ROWS)
        with fused.switches(POSTERIOR_ROWS=n_samples):
            self.calc_probs(time, flux_0, flux_err_0, P_orb, **calc_probs_kwargs)
        if all(p is None for p in self.posterior) and np.isfinite(self.lnZ).any():
            raise NotImplementedError("calc_posteriors needs the device paths (set_sampling('device') or "
                                      "'numpy-device'): this sampling mode returns no posterior rows")
        return

    @staticmethod
    def _datasets_args(datasets, n_samples, evaluation, calc_probs_kwargs):
        """the checked arguments of calc_probs_datasets: (Datasets, n_samples, calc_probs' keywords less verbose, verbose)"""
        from . import fused
        if evaluation not in fused.DATASET_EVALUATIONS:
            raise ValueError("evaluation must be one of %s (got %r)" % (fused.DATASET_EVALUATIONS, evaluation))
        for k in ("exptime", "nsamples"):
            if k in calc_probs_kwargs:
                raise TypeError("calc_probs_datasets() got the keyword '%s': every dataset carries its own" % k)
        sets = _validate_datasets(datasets)
        ds = Datasets(sets, _t0_grids(datasets, sets), _outliers(datasets, sets), _red_baselines(datasets, sets),
                      white_grids=_white_grids(datasets, sets), white_baselines=_white_baselines(datasets, sets),
                      red_kernel_baselines=_red_kernel_baselines(datasets, sets))
        n_samples = int(n_samples)
        if not 0 <= n_samples <= fused.POST_MAX_ROWS:
            raise ValueError("n_samples must lie in [0, %d]" % fused.POST_MAX_ROWS)
        from .marginal_likelihoods import _sampling
        if _sampling["mode"] == "numpy":
            raise NotImplementedError("calc_probs_datasets needs a device sampling mode: set_sampling('device') or "
                                      "'numpy-device'")
        kw = dict(calc_probs_kwargs)
        verbose = kw.pop("verbose", 1)
        return ds, n_samples, kw, verbose

    def _datasets_pass(self, ds, P_orb, kw, verbose, evaluation, n_samples=0, **dataset_switches):
        """one pass of the datasets path over the target's work units: (units, rows, n_scen) for _finish.
        dataset_switches: fused.DATASET_OFFSETS / DATASET_BASELINES / DATASET_RED_NOISE / DATASET_T0 / DATASET_OUTLIERS / DATASET_RED_BASELINES / DATASET_WHITE_NOISE / DATASET_WHITE_BASELINES / DATASET_RED_KERNEL_BASELINES / DATASET_WARP_HIST for
        the length of the pass."""
        from . import fused
        units, n_scen = self._prepare(ds, None, None, P_orb, **kw)
        for flag, what in _FUSED_REFUSALS:
            if getattr(ds, flag) and evaluation == "fused":
                raise NotImplementedError("evaluation='fused' with %s dataset is not built: use evaluation='grid'" % what)
        with fused.switches(POSTERIOR_ROWS=n_samples, DATASET_EVALUATION=evaluation, **dataset_switches):
            rows = sharding.run_units(units, verbose=verbose, as_rows=True)
        return units, rows, n_scen

    def calc_probs_datasets(self, datasets, P_orb, n_samples: int = 0, evaluation: str = "grid", **calc_probs_kwargs):
        """calc_probs on several light curves of one candidate, each with its own cadence and with per-point flux
        errors (no reference counterpart).

        datasets: a list of 1 to 16 dicts {"time", "flux", "flux_err": a number or an array of len(time),
        "exptime": 0.00139, "nsamples": 20}.  Points with a NaN time or flux are dropped with their error.  The
        log-weight of a draw is -ln(sigma_bar) - 0.5 ln 2 pi - sum over the datasets of
        0.5 sum_t (flux_t - model_t)^2 / sigma_t^2 + lnprior, sigma_bar = mean(sigma_t^-2)^-1/2 over all points: one
        dataset with one error for all points gives calc_probs' evidences.  calc_probs_kwargs: the other arguments of
        calc_probs, except exptime and nsamples (each dataset has its own).

        Fills the target as calc_probs does -- and `.posterior` as calc_posteriors does when n_samples > 0 --, plus
        `.sigma_ref`: sigma_bar in the target star's normalisation.  Every masked draw is evaluated in full on every
        dataset: no bounded evaluation, no launch chains -- several times the time of calc_probs.  evaluation="grid"
        (default): the model curves of a chunk of rows are written to a grid, then reduced; "fused": model and weighted
        chi^2 in one kernel per dataset (trx_lnl_batch_weighted), no grid -- the same evidences to rounding (1e-12
        relative in chi^2/2), the same masked draws and best draws.  Needs set_sampling("device") or "numpy-device".

        A dataset may carry "offset_sigma": s > 0 or inf.  Its light curve is then taken to be normalised up to a
        constant offset c ~ N(0, s^2) (inf: a flat prior), in the units of its flux, and c is marginalised in closed
        form per draw: with r_t = flux_t - model_t, w_t = sigma_t^-2, S0 = sum w, S1 = sum w r, S2 = sum w r^2 the
        dataset's term of the log-weight is 0.5 (S2 - S1^2 / (S0 + 1 / s^2)) in place of 0.5 S2.  The factor
        (1 + s^2 S0)^(-1/2) of the marginal is dropped: it depends on the dataset only -- s scales with the errors when a
        light curve is renormalised to a star -- so it is common to every scenario of every star, and `.probs`, `.FPP`
        and `.NFPP` are those of the full marginal (`.lnZ` is short of it by that constant).  Grid evaluation only:
        evaluation="fused" with such a dataset raises NotImplementedError.  `.dataset_offsets` is then an
        [n_scenarios][n_datasets] array: the posterior-mean offset S1 / (S0 + 1 / s^2) of each scenario's best draw, in
        the target's normalisation; NaN for a dataset without offset_sigma and for a scenario without a finite lnZ (on
        several ranks also for the scenarios another rank evaluated).  None when no dataset has an offset.

        A dataset may also carry "baseline": K_b columns B_k[t] ([K_b][len(time)], or [len(time)] for one) of a linear
        baseline model -- a trend with time, airmass, seeing, detector position (lightcurve.polynomial_baseline makes the
        powers of the scaled time) -- and "baseline_sigma": the prior sigma s_k of each coefficient, a number or [K_b],
        each > 0 or inf, in flux units per unit of its column (absent: inf, a flat prior).  The data model is
        model_t + sum_k c_k B_k[t], c_k ~ N(0, s_k^2) independent, and the c_k are marginalised in closed form per draw,
        together with the constant of offset_sigma if the dataset has one (the column of ones, term 0 of the same system;
        at most 4 terms in all): the dataset's term of the log-weight is 0.5 (S2 - b^T A^-1 b), b_k = sum w B_k r,
        A = B^T W B + diag(1 / s_k^2).  The factor det(I + diag(s^2) B^T W B)^(-1/2) of the marginal is dropped for the
        same reason as the offset's: every finite s_k scales with the errors under renormalisation, so it is common to all
        scenarios of all stars.  Collinear terms (a constant column next to offset_sigma, more flat terms than points: the
        smallest eigenvalue of the unit-diagonal scaling of A below 1e-6) are a ValueError.  Grid evaluation only.
        `.dataset_baselines` is then a list per scenario of a list per dataset: the [K_b] posterior-mean coefficients
        A^-1 b of the scenario's best draw in the target's normalisation (NaN without a finite lnZ), None for a dataset
        without "baseline"; the whole attribute is None when no dataset has one.  `.dataset_offsets` reports the offset of
        a baseline dataset that has offset_sigma as well.  Not built: a multiplicative normalisation, baselines in the
        fused evaluation, calc_probs_many with datasets.

        A dataset may carry "red_sigma": s_r, finite and > 0, in flux units, and "red_timescale": tau > 0 (inf allowed),
        in the units of its time -- both or neither: correlated noise next to the white errors, with the covariance
        K = diag(sigma_t^2) + s_r^2 exp(-|t_i - t_j| / tau) (one Ornstein-Uhlenbeck term).  The dataset's term of the
        log-weight is then 0.5 y^T K^-1 y, y_t = flux_t - model_t, evaluated exactly in O(len(time)) per draw by the
        process' Kalman recurrence (datasets.ou_system, trxn_chi2_grid_ou).  det K depends on the dataset only -- s_r
        scales with the errors when a light curve is renormalised to a star -- and is dropped as the offset's factor is.
        sigma_bar, the secondary-eclipse rule and the best draw (the smallest sum of the datasets' terms) are formed as
        without the keys.  tau -> 0: white noise with sigma_t^2 + s_r^2; tau = inf: offset_sigma = s_r.  The kept
        stamps must be in non-decreasing order (ValueError otherwise: the model is a process in time), and the keys do
        not combine with offset_sigma or baseline on the same dataset (ValueError).  Grid evaluation only:
        evaluation="fused" with such a dataset raises NotImplementedError.

        Where s_r and tau are not known, a dataset may carry "red_grid" in their place: 1 to 8 candidates (s_r, tau, weight)
        -- lightcurve.red_noise_grid makes a product grid --, s_r finite and > 0, tau > 0 or inf, the prior weights > 0
        (normalised to sum 1; repeated pairs are allowed).  The pair is then integrated out per draw, determinants
        included: with h_j = 0.5 y^T K_j^-1 y of candidate j and c_j proportional to weight_j |K_j|^(-1/2), sum_j c_j = 1
        (datasets.ou_mix_system), the dataset's term of the log-weight is -ln sum_j c_j exp(-h_j), in one pass over the
        model grid for all candidates (trxm_chi2_grid_ou_mix).  The normaliser sum_j weight_j |K_j|^(-1/2) depends on the
        dataset only (every s_r scales with the errors under renormalisation, so the c_j are the same for every star) and is
        dropped as det K is.  One candidate of weight 1 gives the bits of red_sigma / red_timescale.  The same conditions:
        stamps in non-decreasing order, not next to red_sigma / red_timescale, offset_sigma or baseline on the same dataset
        (ValueError), grid evaluation only.  `.dataset_red_noise` is then a list per scenario of a list per dataset: None
        for a dataset without "red_grid", else {"grid": the [J][3] candidates as validated (s_r, tau, normalised prior
        weight, in the units given), "weight": the [J] posterior weights of the candidates at the scenario's best draw,
        softmax_j(ln c_j - h_j) (NaN without a finite lnZ)}; the whole attribute is None when no dataset has a grid.
        Not built: per-draw candidate posteriors, a continuous fit of s_r and tau, candidates of another kernel than the
        one exponential term, red noise next to offset or baseline.

        Where the transit time of a dataset is uncertain -- a follow-up night long after the ephemeris was measured --
        the dataset may carry "t0_grid" next to any of the keys above: 1 to 8 nodes (shift, weight), the shifts in the units
        of `time`, finite and all different, the prior weights > 0 (normalised to sum 1); lightcurve.t0_shift_grid makes
        the nodes of a Gaussian prior.  With h_j the dataset's term of the log-weight on the stamps time + shift_j -- by
        whichever reduction the dataset uses --, its term becomes -ln sum_j weight_j exp(-h_j): J model grids and J
        reductions per draw, folded by trxt_softmin_rows.  Nothing is dropped: the weights sum to 1, and a shift leaves the
        stamp differences, the baseline columns (they follow the points, not the shifted stamps) and the determinants as
        they are.  One node (d, 1) gives the bits of the same dataset with time + d.  Grid evaluation only.
        `.dataset_t0` is then a list per scenario of a list per dataset: None for a dataset without the key, else
        {"shift": the [J] shifts, "weight": the [J] posterior weights of the nodes at the scenario's best draw,
        softmax_j(ln weight_j - h_j) (NaN without a finite lnZ), "mean": sum_j weight_j shift_j}; the whole attribute is
        None when no dataset has the key.  `.dataset_offsets`, `.dataset_baselines` and `.dataset_red_noise` of such a
        dataset are those of its node of largest weight (the first of equal ones).  Not built: a shift shared between
        datasets, a continuous fit of the shift, per-draw shift posteriors.

        Where single points of a dataset may be off by far more than their errors -- a passing cloud, a cosmic ray --, the
        dataset may carry "outlier_frac": eps, 0 < eps <= 0.5, and "outlier_scale": kappa, finite and > 1 -- both or
        neither: every point is then, with prior probability eps, an outlier from a Gaussian kappa times wider than its
        flux_err, and its membership is integrated out per point and per draw.  With a_t = 0.5 (flux_t - model_t)^2 /
        sigma_t^2 the dataset's term of the log-weight is sum_t -ln[(1 - eps) exp(-a_t) + (eps / kappa) exp(-a_t / kappa^2)]
        in place of sum_t a_t (_numerics.robust_halfchi2, trxr_chi2_grid_robust): an 8 sigma point costs about
        ln(kappa / eps) + 32 / kappa^2 instead of 32.  Only the common factor prod_t (sigma_t sqrt(2 pi))^-1 is dropped, as it
        is without the keys; only (flux_t - model_t) / sigma_t enters, so the term is the same in every star's
        normalisation.  sigma_bar and the secondary-eclipse rule use flux_err as given.  The keys stand next to "t0_grid"
        but not next to offset_sigma, baseline, red_sigma / red_timescale or red_grid on the same dataset (ValueError).
        Grid evaluation only.  `.dataset_outliers` is then a list per scenario of a list per dataset: None for a dataset
        without the keys, else {"frac", "scale", "prob": the [len(kept points)] posterior probabilities
        1 / (1 + (1 - eps) kappa / eps exp(-a_t (1 - 1 / kappa^2))) that each point is an outlier at the scenario's best draw
        (NaN without a finite lnZ; with a t0_grid on its node of largest weight)}; the whole attribute is None when no
        dataset has the keys.  Not built: the keys next to offset, baseline or red noise, a Student-t form, a fit of eps,
        per-draw outlier probabilities, the scalar calc_probs path.

        A dataset with red_sigma / red_timescale may carry a trend as well: "red_baseline": 1 ... 4 columns B_k
        [K_b][len(time)] (or [len(time)]) aligned with `time`, finite at the kept points, and "red_baseline_sigma": the
        prior sigmas of their coefficients c_k ~ N(0, s_k^2), a number or [K_b], each > 0 or inf (absent: flat).  A column
        of ones is how the constant is given (lightcurve.trend_columns); no offset_sigma stands next to these keys.  The
        coefficients are marginalised per draw under the correlated noise K: the dataset's term of the log-weight is
        0.5 [y^T K^-1 y - b^T A^-1 b], b = B^T K^-1 y, A = B^T K^-1 B + diag(1 / s_k^2) -- for finite priors
        0.5 y^T (K + B diag(s^2) B^T)^-1 y -- in the Kalman form of ou_system that whitens residuals and columns alike
        (datasets.ou_baseline_system, _numerics.ou_baseline_halfchi2, trxg_chi2_grid_ou_baseline).  The dropped factors
        det K and det(I + diag(s^2) B^T K^-1 B) depend on the dataset alone and are the same for every star: red_sigma and
        every finite s_k scale with the errors.  The keys stand only next to red_sigma / red_timescale and may stand next
        to "t0_grid"; next to offset_sigma, baseline, red_grid or the outlier keys, without the two red keys, with a zero
        column or with columns that are collinear under the noise they are a ValueError.  Grid evaluation only.
        `.dataset_red_baselines` is then a list per scenario of a list per dataset: None for a dataset without the keys,
        else the [K_b] posterior-mean coefficients at the scenario's best draw, in flux units per unit of the column (NaN
        without a finite lnZ; with a t0_grid on its node of largest weight); the whole attribute is None when no dataset
        has the keys.  Not built: red_grid next to a baseline, the outlier keys next to any marginalised term, the fused
        evaluation, the scalar calc_probs path (under the other kernels the columns go under red_kernel_baseline).

        A dataset with red_sigma / red_timescale may name the kernel of that noise: "red_kernel": "ou", None or absent is
        the one exponential term above, with its calls and its bits.  "matern32": red_sigma = s and red_timescale = l, both
        finite and > 0, K = diag(sigma_t^2) + s^2 (1 + sqrt(3) D / l) exp(-sqrt(3) D / l), D = |t_i - t_j| -- smooth sample
        paths, as airmass, seeing and drift are.  "ou2": red_sigma = (s_1, s_2) and red_timescale = (tau_1, tau_2), arrays
        of two, every entry finite and > 0, K = diag(sigma_t^2) + s_1^2 exp(-D / tau_1) + s_2^2 exp(-D / tau_2) -- two time
        scales, minutes and hours.  The dataset's term of the log-weight is 0.5 y^T K^-1 y as before, exact in O(len(time))
        per draw: both processes have a state of dimension two, and the innovation form of their Kalman filter needs
        per-stamp tables A [T][2][2], g [T][2], omega [T] that depend on the dataset alone (datasets.ss2_system,
        _numerics.ss2_halfchi2, trxs_chi2_grid_ss2).  det K depends on the dataset only -- every s scales with the errors
        when a light curve is renormalised to a star -- and is dropped as for the one term.  The stamps must be in
        non-decreasing order; with these two kernels the dataset may stand next to "t0_grid" only: next to offset_sigma,
        baseline, red_grid, red_baseline or the outlier keys, for a red_kernel that is none of the four values, for shapes
        that do not fit the kernel or an entry that is not finite and > 0 (tau = inf stays the one term's business) it is a
        ValueError.  Grid evaluation only: evaluation="fused" raises NotImplementedError.  Nothing new is reported per
        best draw.  Not built: these kernels next to red_grid or the outlier keys, a quasi-periodic (SHO) term,
        more than two exponential terms, the fused evaluation, the scalar calc_probs path.

        A dataset with such a red_kernel may carry a trend as well: "red_kernel_baseline": 1 ... 4 columns B_k
        [K_b][len(time)] (or [len(time)]) aligned with `time`, finite at the kept points -- lightcurve.trend_columns makes
        them; a column of ones is the constant --, and "red_kernel_baseline_sigma": the prior sigmas of their coefficients
        c_k ~ N(0, s_k^2), a number or [K_b], each > 0 or inf (absent: flat).  The coefficients are marginalised per draw
        under the kernel's noise K exactly as red_baseline's are under the one exponential term: the dataset's term of the
        log-weight is 0.5 [y^T K^-1 y - b^T A^-1 b], b = B^T K^-1 y, A = B^T K^-1 B + diag(1 / s_k^2) -- for finite priors
        0.5 y^T (K + B diag(s^2) B^T)^-1 y --, the two-state filter of ss2_system whitening residuals and columns alike
        (datasets.ss2_baseline_system, _numerics.ss2_baseline_halfchi2, trxk_chi2_grid_ss2_baseline).  The dropped factors
        det K and det(I + diag(s^2) B^T K^-1 B) depend on the dataset alone and are the same for every star.  The keys
        stand only next to red_kernel = "matern32" or "ou2" and may stand next to "t0_grid"; next to offset_sigma,
        baseline, red_baseline, red_grid, white_grid or the outlier keys, without such a red_kernel ("red_baseline" next to
        red_kernel stays a ValueError: these are its keys there), with a zero column or with columns that are collinear
        under the noise they are a ValueError.  Grid evaluation only.  `.dataset_red_kernel_baselines` is then a list per
        scenario of a list per dataset: None for a dataset without the keys, else the [K_b] posterior-mean coefficients at
        the scenario's best draw, in flux units per unit of the column (NaN without a finite lnZ; with a t0_grid on its
        node of largest weight); the whole attribute is None when no dataset has the keys.  Not built: red_grid next to a
        baseline, an SHO term, the fused evaluation, the keys next to any other marginalised term, the scalar calc_probs
        path.

        Where the SIZE of a dataset's white noise is not known -- photon-noise errors from a differential-photometry
        pipeline, binned errors that ignore what detrending left --, the dataset may carry "white_grid": 1 to 8 candidates
        (scale k, jitter s, weight) -- lightcurve.white_noise_grid makes a product grid --, k finite and > 0, s finite and
        >= 0 in flux units, the prior weights > 0 (normalised to sum 1; repeated pairs are allowed).  Candidate j has the
        per-point variance v_j[t] = k_j^2 sigma_t^2 + s_j^2, and the pair is integrated out per draw, determinants included:
        with w_j = 1 / v_j, h_j = 0.5 sum_t w_j[t] (flux_t - model_t)^2 and c_j proportional to weight_j prod_t w_j[t]^(1/2),
        sum_j c_j = 1 (datasets.white_mix_system), the dataset's term of the log-weight is -ln sum_j c_j exp(-h_j), in one
        pass over the model grid for all candidates (trxv_chi2_grid_white_mix).  The normaliser
        sum_j weight_j prod_t w_j[t]^(1/2) depends on the dataset only (every s_j scales with the errors under
        renormalisation and the k_j are pure numbers, so the c_j are the same for every star) and is dropped as det K is for
        red_grid: `.probs`, `.FPP` and `.NFPP` are those of the full marginal.  One candidate (1, 0) of weight 1 gives the
        bits of the dataset without the key.  sigma_bar and the secondary-eclipse rule use flux_err as given.  No condition
        on the order of the stamps: a folded light curve may carry the key.  It stands alone or next to "t0_grid"; next to
        offset_sigma, baseline, red_sigma / red_timescale, red_grid, red_kernel, red_baseline or the outlier keys on the
        same dataset it is a ValueError.  Grid evaluation only.  `.dataset_white_noise` is then a list per scenario of a
        list per dataset: None for a dataset without the key, else {"grid": the [J][3] candidates as validated (k, s,
        normalised prior weight, in the units given), "weight": the [J] posterior weights of the candidates at the
        scenario's best draw, softmax_j(ln c_j - h_j) (NaN without a finite lnZ; with a t0_grid on its node of largest
        weight)}; the whole attribute is None when no dataset has the key.  Not built: the key next to an offset, a
        baseline, red noise or the outlier keys, a continuous fit of k or s, per-draw candidate posteriors, the fused
        evaluation, the scalar calc_probs path.

        A dataset with "white_grid" whose normalisation or trend is not known either -- a single-night ground-based curve --
        may carry next to it "white_baseline": an array [K][len(time)] (or [len(time)]) of K <= 4 columns B_k[t] of a linear
        baseline model sum_k c_k B_k[t] -- lightcurve.trend_columns makes them; a column of ones is the constant --, and
        "white_baseline_sigma": the prior sigmas of c_k ~ N(0, s_k^2), a number or one per column, > 0 or inf (absent:
        flat).  The coefficients are integrated out per draw under every candidate, determinants included: with
        A_j = B^T W_j B + diag(1 / s_k^2), b_j = B^T W_j (flux - model) and h_j = 0.5 max(S2_j - b_j^T A_j^-1 b_j, 0) the
        dataset's term is -ln sum_j c_j exp(-h_j), c_j proportional to weight_j prod_t w_j[t]^(1/2) det(A_j)^(-1/2)
        (datasets.white_baseline_system), in one pass over the model grid for all candidates and columns
        (trxb_chi2_grid_white_baseline).  Every finite sigma is in flux units per unit of its column and is renormalised
        with the errors, so det A_j gains the same factor for every candidate and the c_j are the same for every star.  The
        keys stand only next to white_grid (and t0_grid): without it, or next to offset_sigma, baseline, any red key or
        the outlier keys they are a ValueError, as are a sigma without columns, a wrong shape, more than four columns, a
        kept entry that is not finite, a zero column, a bool or a string, or columns that are collinear under a
        candidate's weights.  Grid evaluation only.  `.dataset_white_baselines` is then a list per scenario of a list per
        dataset: None for a dataset without the keys, else {"coef": the [J][K] posterior-mean coefficients under each
        candidate at the scenario's best draw, in the units of the given flux, "mean": [K] their average under the
        candidates' posterior weights (`.dataset_white_noise`'s "weight")} (NaN without a finite lnZ; with a t0_grid on
        its node of largest weight); the whole attribute is None when no dataset has the keys.  Not built: white_grid next
        to the plain offset_sigma / baseline keys, red_grid next to a baseline, the fused evaluation."""
        ds, n_samples, kw, verbose = self._datasets_args(datasets, n_samples, evaluation, calc_probs_kwargs)
        best_offsets = {} if ds.has_offsets else None
        best_baselines = {} if ds.has_baselines else None
        best_red = {} if any(s.red_grid is not None for s in ds.sets) else None
        best_t0 = {} if ds.has_t0_grids else None
        best_outliers = {} if ds.has_outliers else None
        best_gls = {} if ds.has_red_baselines else None
        best_white = {} if ds.has_white_grids else None
        best_lin = {} if ds.has_white_baselines else None
        best_ss2gls = {} if ds.has_red_kernel_baselines else None
        units, rows, n_scen = self._datasets_pass(ds, P_orb, kw, verbose, evaluation, n_samples,
                                                  DATASET_OFFSETS=best_offsets, DATASET_BASELINES=best_baselines,
                                                  DATASET_RED_NOISE=best_red, DATASET_T0=best_t0,
                                                  DATASET_OUTLIERS=best_outliers, DATASET_RED_BASELINES=best_gls,
                                                  DATASET_WHITE_NOISE=best_white, DATASET_WHITE_BASELINES=best_lin,
                                                  DATASET_RED_KERNEL_BASELINES=best_ss2gls)
        self._finish(units, rows, n_scen, layout=sharding.last_layout)
        share = self.stars["fluxratio"].to_numpy()[self.stars["tdepth"].to_numpy() > 0]
        self.sigma_ref = ds.renorm(share[0]).sigma_ref if share.size else ds.sigma_ref

        # (a call's offsets are in its star's normalisation: flux' = (flux - (1 - fr)) / fr, so c = fr c'; and c_k multiplies
        # a column that is left alone, so it scales as the flux does: c = fr c')
        def scaled(u, per):
            return [None if c is None else c * share[u.group[1]] for c in per]

        def blank_coefs(sizes):
            return lambda: [None if m is None else np.full(m, np.nan) for m in sizes]

        table = self._scatter_best(units, best_offsets, lambda: np.full(len(ds), np.nan),
                                   lambda u, c: c * share[u.group[1]])
        self.dataset_offsets = None if table is None else np.array(table).reshape(n_scen, len(ds))
        self.dataset_baselines = self._scatter_best(
            units, best_baselines, blank_coefs([None if s.baseline is None else s.baseline.shape[0] for s in ds.sets]), scaled)
        self.dataset_red_baselines = self._scatter_best(
            units, best_gls, blank_coefs([None if p is None else p[0].shape[0] for p in ds.red_baselines]), scaled)
        self.dataset_red_kernel_baselines = self._scatter_best(
            units, best_ss2gls, blank_coefs([None if p is None else p[0].shape[0] for p in ds.red_kernel_baselines]), scaled)

        # (the weights are pure numbers: the same in every star's normalisation; a white_grid is as validated, in the units
        # given)
        def cand(g, w=None):
            if g is None:
                return None
            return {"grid": g.copy(), "weight": np.full(g.shape[0], np.nan) if w is None else w}
        red_grids = [s.red_grid for s in ds.sets]
        self.dataset_red_noise = self._scatter_best(units, best_red, lambda: [cand(g) for g in red_grids],
                                                    lambda u, per: [cand(g, w) for g, w in zip(red_grids, per)])
        self.dataset_white_noise = self._scatter_best(units, best_white, lambda: [cand(g) for g in ds.white_grids],
                                                      lambda u, per: [cand(g, w) for g, w in zip(ds.white_grids, per)])

        # (shifts are times and the weights pure numbers: the same in every star's normalisation)
        def node(g, w=None):
            if g is None:
                return None
            w = np.full(g.shape[0], np.nan) if w is None else w
            return {"shift": g[:, 0].copy(), "weight": w, "mean": float(np.sum(w * g[:, 0]))}
        self.dataset_t0 = self._scatter_best(units, best_t0, lambda: [node(g) for g in ds.t0_grids],
                                             lambda u, per: [node(g, w) for g, w in zip(ds.t0_grids, per)])

        # (only (flux - model) / sigma enters: the same in every star's normalisation)
        def points(s, o, p=None):
            if o is None:
                return None
            return {"frac": o[0], "scale": o[1], "prob": np.full(s.time.size, np.nan) if p is None else p}
        robust = list(zip(ds.sets, ds.outliers))
        self.dataset_outliers = self._scatter_best(units, best_outliers, lambda: [points(s, o) for s, o in robust],
                                                   lambda u, per: [points(s, o, p) for (s, o), p in zip(robust, per)])

        # (as dataset_baselines: c = fr c')
        def terms(g, p, c=None, fr=1.0):
            if p is None:
                return None
            J, K = g.shape[0], p[0].shape[0]
            if c is None:
                return {"coef": np.full((J, K), np.nan), "mean": np.full(K, np.nan)}
            return {"coef": c["coef"] * fr, "mean": c["mean"] * fr}
        pairs = list(zip(ds.white_grids, ds.white_baselines))
        self.dataset_white_baselines = self._scatter_best(
            units, best_lin, lambda: [terms(g, p) for g, p in pairs],
            lambda u, per: [terms(g, p, c, share[u.group[1]]) for (g, p), c in zip(pairs, per)])
        return

    def _scatter_best(self, units, best, blank, fill):
        """what a DATASET_* switch collected (`best`: {work unit: per branch, what the datasets' terms left}) as a list per
        scenario row: blank() for a row whose unit left nothing or whose lnZ is not finite, else fill(unit, the branch's
        entries); None for a switch that was not opened"""
        if best is None:
            return None
        rows = [blank() for _ in range(len(self.lnZ))]
        for k, u in enumerate(sharding.as_units(units)):
            for i, per in enumerate(best.get(k, ())):
                if np.isfinite(self.lnZ[u.first_row + i]):
                    rows[u.first_row + i] = fill(u, per)
        return rows

    def calc_probs_refined(self, time, flux_0, flux_err_0: float, P_orb, n_adapt: int = 2, N_adapt: int = None,
                           n_samples: int = 0, alpha: float = 0.5, floor: float = 0.1, **calc_probs_kwargs):
        """calc_probs by adaptive importance sampling: n_adapt adaptation passes of N_adapt draws
        each (default: N), then one final pass of N draws that fills the target exactly as calc_probs does -- and, with
        n_samples > 0, `.posterior` as calc_posteriors does.

        Every continuous random input of a draw is the inverse-CDF transform of one uniform, so in the space of those
        uniforms the prior is the constant 1 on the unit cube.  Each lnZ_* call (work unit) keeps a per-dimension
        piecewise-linear map of that cube (a VEGAS grid of 64 bins for each of P, q_companion, R_p, inc, q, ecc and argp;
        the identity at first); an adaptation pass returns the histogram of its evidence's weight over the bins, and
        _numerics.warp_refine(alpha, floor) moves the edges so that the next pass draws mostly where the weight is.  The
        map's Jacobian enters every weight, so any grid gives the same expectation; only the final pass -- whose grids
        are fixed by independent earlier draws -- enters the result: the estimate is unbiased.  Every pass draws from the
        generator's running stream, as consecutive calc_probs calls do.  `.refine_history` holds, per pass, the rows'
        lnZ, ess and w_max_frac.  n_adapt = 0 is calc_probs (calc_posteriors), bit for bit.

        Needs set_sampling("device") -- the numpy modes stage their uniforms, and a staged uniform is never mapped --
        and one rank."""
        from . import fused
        n_adapt, n_samples = int(n_adapt), int(n_samples)
        if n_adapt < 0:
            raise ValueError("n_adapt must be >= 0")
        kw = dict(calc_probs_kwargs)

        def final():
            if n_samples > 0:
                self.calc_posteriors(time, flux_0, flux_err_0, P_orb, n_samples=n_samples, **kw)
            else:
                self.calc_probs(time, flux_0, flux_err_0, P_orb, **kw)

        kw_adapt = dict(kw)
        verbose = kw_adapt.pop("verbose", 1)
        if N_adapt is not None:
            kw_adapt["N"] = int(N_adapt)

        def adapt_pass():
            units, n_scen = self._prepare(time, flux_0, flux_err_0, P_orb, **kw_adapt)
            with fused.switches(WARP_HIST=True):
                rows = sharding.run_units(units, verbose=verbose, as_rows=True)
            hists = {}
            for k, rec in enumerate(rows):
                if rec is None:
                    continue
                hists[k] = rec[:, sharding.last_layout.hist]
                if np.isnan(hists[k][:, 1]).any():        # (a row shorter than the table stays NaN there)
                    raise NotImplementedError("calc_probs_refined needs the library's own chain "
                                              "(set_sampling('device')): this pass returned no weight histograms")
            return units, rows, n_scen, hists

        self._refined("calc_probs_refined", n_adapt, adapt_pass, final, alpha, floor)
        return

    def _refined(self, who, n_adapt, adapt_pass, final, alpha, floor):
        """The loop of calc_probs_refined and calc_probs_datasets_refined.  adapt_pass() runs one adaptation pass under
        fused.WARP_GRIDS and returns (units, rows, n_scen, {work unit: its branches' weight histograms}); every unit's
        grid is refined from its histogram (_numerics.warp_refine) and the pass enters `.refine_history`.  final() is
        the plain call, run under the grids the adaptation left."""
        from . import fused
        from ._numerics import warp_refine

        def snapshot():
            return {"lnZ": np.array(self.lnZ), "ess": np.array(self.ess), "w_max_frac": np.array(self.w_max_frac)}

        if n_adapt == 0:
            final()
            self.refine_history = [snapshot()]
            return
        if not fused.threadable() or not fused.NATIVE:
            raise NotImplementedError("%s needs set_sampling('device'): the numpy sampling modes stage "
                                      "their uniforms, and a staged uniform is never mapped" % who)
        if sharding._dist() is not None:
            raise NotImplementedError("%s on several ranks is not built: the grids would have to follow "
                                      "the schedule" % who)
        grids = {}                       # work unit -> [7][65] edges (kept per (star, call), not per target)
        history = []
        with fused.switches(POSTERIOR_ROWS=0, WARP_GRIDS=grids):
            for _ in range(n_adapt):
                units, rows, n_scen, hists = adapt_pass()
                for k, hist in hists.items():
                    grids[k] = warp_refine(grids.get(k, fused.warp_identity()), hist, alpha=alpha, floor=floor)
                self._finish(units, rows, n_scen, warn=False, layout=sharding.last_layout)
                history.append(snapshot())
            final()
            history.append(snapshot())
        self.refine_history = history
        return

    def calc_probs_datasets_refined(self, datasets, P_orb, n_adapt: int = 2, N_adapt: int = None, n_samples: int = 0,
                                    evaluation: str = "grid", alpha: float = 0.5, floor: float = 0.1,
                                    **calc_probs_kwargs):
        """calc_probs_datasets by adaptive importance sampling: calc_probs_refined's loop on the
        datasets path (section 14).  n_adapt adaptation passes of N_adapt draws each (default: N) evaluate the datasets
        under each work unit's importance map, take the histogram of the evidence's weight over the bins of the draws'
        uniforms from the chi^2/2 values of that pass (trxw_hist_from_halfchi2, fused.DATASET_WARP_HIST) and refine
        the map; best-draw offsets and baselines are not computed in them.  The final pass is calc_probs_datasets under
        the maps the adaptation left: it fills `.probs`, `.FPP`, `.lnZ_err`, `.posterior` (n_samples > 0), `.sigma_ref`,
        `.dataset_offsets`, `.dataset_baselines`, `.dataset_red_noise`, `.dataset_t0`, `.dataset_outliers`, `.dataset_red_baselines`, `.dataset_white_noise`, `.dataset_white_baselines` and `.dataset_red_kernel_baselines` as calc_probs_datasets does, and only it enters the result, so the
        estimate is unbiased.  `.refine_history` holds, per pass, the rows' lnZ, ess and w_max_frac.  n_adapt = 0 is
        calc_probs_datasets, bit for bit.  Both evaluations ("grid", "fused") feed the histogram the same way.

        Needs set_sampling("device") and one rank."""
        n_adapt = int(n_adapt)
        if n_adapt < 0:
            raise ValueError("n_adapt must be >= 0")
        ds, n_samples, kw, verbose = self._datasets_args(datasets, n_samples, evaluation, calc_probs_kwargs)

        def final():
            self.calc_probs_datasets(datasets, P_orb, n_samples=n_samples, evaluation=evaluation, **calc_probs_kwargs)

        kw_adapt = dict(kw)
        if N_adapt is not None:
            kw_adapt["N"] = int(N_adapt)

        def adapt_pass():
            hists = {}
            units, rows, n_scen = self._datasets_pass(ds, P_orb, kw_adapt, verbose, evaluation, DATASET_WARP_HIST=hists)
            return units, rows, n_scen, hists

        self._refined("calc_probs_datasets_refined", n_adapt, adapt_pass, final, alpha, floor)
        return

    def posterior_summary(self, q=(0.16, 0.5, 0.84)):
        """Quantiles of every scenario's posterior samples (calc_posteriors): a DataFrame with one row per scenario
        that has samples -- ID, scenario, prob, then <param>_q<100 q> for every physical column.  The samples are
        equally weighted, so these are plain np.quantile values."""
        self._finish_pending()
        post = self.__dict__.get("posterior")
        stored = self.__dict__.get("posterior_quantiles")
        if post is None and stored is None:
            raise ValueError("no posterior samples: run calc_posteriors first")
        if post is None:
            # (calc_posteriors_many(keep="summary"): the quantiles were taken where the samples were; the samples are gone)
            if tuple(float(x) for x in q) != tuple(self._posterior_q):
                raise ValueError("this target holds the quantiles %r only (calc_posteriors_many(keep='summary')): "
                                 "ask for those, or keep the samples" % (tuple(self._posterior_q),))
            post = stored
        cols = self._probs_columns
        out = []
        for j, p in enumerate(post):
            if p is None:
                continue
            row = {"ID": cols["ID"][j], "scenario": cols["scenario"][j], "prob": cols["prob"][j]}
            for c in _POSTERIOR_PARAMS:
                for qq, v in zip(q, p[c] if post is stored else np.quantile(p[c], q)):
                    row["%s_q%g" % (c, 100 * qq)] = v
            out.append(row)
        return DataFrame(out)

    def _samples(self):
        """`.posterior` of the last calc_posteriors; raises where there are no samples to draw from"""
        self._finish_pending()            # (a table left to its first reader: calc_posteriors_many on several ranks)
        post = self.__dict__.get("posterior")
        if post is None and self.__dict__.get("posterior_quantiles") is not None:
            raise ValueError("this target holds quantiles only (calc_posteriors_many(keep='summary')): the samples are "
                             "gone -- run calc_posteriors_many(keep='samples') to draw from them")
        if post is None:
            raise ValueError("no posterior samples: run calc_posteriors first")
        return post

    def _mixture_picks(self, post, n, rng=None):
        """n (scenario row, sample index) picks from the model-averaged posterior: a scenario in proportion to its
        `prob`, then one of its (equally weighted) samples -- the picks of posterior_samples and of fit_bands'
        model average (the same rng gives both the same picks)."""
        rng = np.random.default_rng() if rng is None else rng
        have = np.array([p is not None for p in post])
        w = np.where(have, np.nan_to_num(np.asarray(self._probs_columns["prob"], dtype=np.float64)), 0.0)
        if not w.sum() > 0:
            raise ValueError("no scenario with posterior samples carries probability")
        which = rng.choice(len(post), size=int(n), p=w / w.sum())
        sample = np.zeros(int(n), dtype=np.int64)
        for j in np.unique(which):
            sel = which == j
            sample[sel] = rng.integers(0, len(post[j]["lnw"]), size=int(sel.sum()))
        return which, sample

    def posterior_samples(self, n, rng=None):
        """n draws from the model-averaged posterior: a scenario in proportion to its `prob`, then one of its
        (equally weighted) samples.  DataFrame of n rows: `scenario`, `ID`, and the physical columns.  Scenarios
        without samples contribute nothing (their probability is zero or was dropped).  Host side, numpy only."""
        post = self._samples()
        cols = self._probs_columns
        which, sample = self._mixture_picks(post, n, rng)
        out = {"scenario": np.asarray(cols["scenario"])[which], "ID": np.asarray(cols["ID"])[which]}
        for c in _POSTERIOR_PARAMS:
            out[c] = np.empty(int(n))
        for j in np.unique(which):
            sel = which == j
            for c in _POSTERIOR_PARAMS:
                out[c][sel] = np.asarray(post[j][c])[sample[sel]]
        return DataFrame(out)

    def calc_probs_runs(self, time, flux_0, flux_err_0: float, P_orb, n_runs: int = 20, **calc_probs_kwargs):
        """n_runs independent calc_probs of this target in ONE sharded pass: the mean and the scatter of FPP and NFPP that
        the reference's tutorial asks for before a result is quoted (its loop of `.calc_probs()` calls), with the
        streams, launch chains, host threads and ranks seeing the units of all runs at once.

        calc_probs_kwargs: the other arguments of calc_probs (verbose defaults to 0 here).  On one rank, one host thread
        and without sharding.per_unit_seed, run r is the r-th of n_runs consecutive calc_probs calls from the same seed,
        bit for bit.  Returns a dict of numpy arrays: FPP, NFPP, FPP_err, NFPP_err [n_runs]; lnZ, prob [n_runs][n_scen];
        FPP_mean, FPP_std, NFPP_mean, NFPP_std (np.std, ddof = 0).  Afterwards the target holds the table of the last
        run, as the loop leaves it."""
        n_runs = int(n_runs)
        if n_runs < 1:
            raise ValueError("n_runs must be >= 1")
        from . import fused
        if fused.POSTERIOR_ROWS:
            raise NotImplementedError("posterior rows are not available in calc_probs_runs (repeated runs with posteriors "
                                      "are not built): use calc_posteriors, or calc_posteriors_many for a batch")
        kw = dict(calc_probs_kwargs)
        verbose = kw.pop("verbose", 0)
        prepared = [self._prepare(time, flux_0, flux_err_0, P_orb, job=r, **kw) for r in range(n_runs)]
        flat = [u for units, _ in prepared for u in units]
        results = sharding.run_units(flat, verbose=verbose, as_rows=True)
        keys = ("FPP", "NFPP", "FPP_err", "NFPP_err")
        out = {k: np.empty(n_runs) for k in keys}
        lnZ, prob = [], []
        at = 0
        for r, (units, n_scen) in enumerate(prepared):
            self._finish(units, results[at:at + len(units)], n_scen, layout=sharding.last_layout)
            at += len(units)
            for k in keys:
                out[k][r] = getattr(self, k)
            lnZ.append(self.lnZ)
            prob.append(self._probs_columns["prob"])
        out["lnZ"], out["prob"] = np.array(lnZ), np.array(prob)
        for k in ("FPP", "NFPP"):
            out[k + "_mean"] = float(np.mean(out[k]))
            out[k + "_std"] = float(np.std(out[k]))
        return out

    def _prepare(self, time, flux_0, flux_err_0, P_orb, contrast_curve_file=None, filt="TESS",
                 N=1000000, parallel=False, drop_scenario=[], flatpriors=False, exptime=0.00139,
                 nsamples=20, molusc_file=None, job=0):
        """Work units of one calc_probs (triceratops.py:673-735: NaN filter, star filter, table
        sizes) and the number of table rows.  job: index of this target in a calc_probs_many batch."""
        if not isinstance(time, Datasets):      # (calc_probs_datasets has validated and filtered its light curves)
            time = np.asarray(time, dtype=np.float64)
            flux_0 = np.asarray(flux_0, dtype=np.float64)
            keep = ~np.isnan(time) & ~np.isnan(flux_0)
            time, flux_0 = time[keep], flux_0[keep]
        # (the stars that can host the signal, triceratops.py:712; as a row mask over the table's own columns --
        # a filtered copy of the DataFrame costs more than everything else in here)
        # (the numeric columns in ONE conversion: eleven `stars[c].to_numpy()` are 30 us of pandas per target, the whole
        # table as one float64 block 7 -- 1.3 ms of a 64-target step, on every rank; a table with a non-numeric column
        # -- string IDs -- takes the columns one by one as before)
        try:
            block = self.stars.to_numpy(dtype=np.float64)
            loc = self.stars.columns.get_loc

            def column(c):
                return block[:, loc(c)]
        except (ValueError, TypeError):
            def column(c):
                return self.stars[c].to_numpy()
        keep = column("tdepth") > 0
        filtered = (keep, self.stars, column)
        n_scen = 3 * int(keep.sum()) + 12
        needs_field = not all(k in drop_scenario for k in ("DTP", "DEB", "BTP", "BEB"))
        if self.trilegal_fname is None and needs_field:
            raise ValueError("trilegal_fname is required for the D and B scenarios (the TRILEGAL "
                             "web query is outside the accelerated path); pass it to target(...) "
                             "or drop DTP, DEB, BTP and BEB")
        units, _ok = self._units(filtered, flux_0, flux_err_0, time, P_orb, contrast_curve_file,
                                 filt, N, parallel, drop_scenario, flatpriors, exptime, nsamples,
                                 molusc_file, job)
        return units, n_scen

    def _finish(self, units, results, n_scen, warn=True, layout=None):
        """Scenario table, normalised probabilities, FPP and NFPP from the per-unit results
        (triceratops.py:1430-1485).  Plain arrays here; the `.probs` DataFrame of the reference is put
        together when it is first read (a batch of 64 targets spent as long building 64 DataFrames nobody
        had asked for yet as waiting for the GPU).  warn = False: the caller has already raised the
        reference's RuntimeWarnings for these evidences (_defer_finish).  layout: the sharding.RowLayout of the pass
        that made `results` (sharding.last_layout; default: rows without posterior columns)."""
        self.__dict__["_pending_finish"] = None
        layout = layout or sharding.RowLayout()
        summary_q = layout.summary_q
        targets = np.zeros(n_scen, dtype=np.dtype("i8"))
        star_num = np.zeros(n_scen, dtype=np.dtype("i8"))
        scenarios = np.zeros(n_scen, dtype=np.dtype('U6'))
        best = {c: np.zeros(n_scen) for c in _COLS}
        lnZ = np.zeros(n_scen)
        rec_tab = None
        lnM2 = np.full(n_scen, np.nan)               # the evidences' moments (sharding.MOMENT_COLS), NaN = unknown
        extras = [None] * n_scen                     # calc_posteriors: every row's samples (summary mode: quantiles)
        lnWmax = np.full(n_scen, np.nan)
        n_draws = np.full(n_scen, np.nan)            # N of each row's lnZ_* call (units of target._units)
        for u, res in zip(sharding.as_units(units), results):
            j0, names, snum, ID = u.first_row, u.names, u.star_num, u.ID
            if u.draws is not None:
                n_draws[j0:j0 + len(names)] = u.draws
            if isinstance(res, np.ndarray):
                # (sharding.run_units(as_rows=True): the unit's rows in `layout` -- or, made by hand, a leading part of it)
                if rec_tab is None:
                    rec_tab = np.zeros((n_scen, len(sharding.RECORD_COLS)))
                nb = len(names)
                rec_tab[j0:j0 + nb] = res[:, layout.record]
                targets[j0:j0 + nb], star_num[j0:j0 + nb] = ID, snum
                scenarios[j0:j0 + nb] = names
                lnZ[j0:j0 + nb] = res[:, layout.lnZ]
                if res.shape[1] >= layout.moments.stop:
                    lnM2[j0:j0 + nb], lnWmax[j0:j0 + nb] = res[:, layout.moments].T
                if layout.post_rows and res.shape[1] >= layout.extra.stop:
                    for i in range(nb):
                        extras[j0 + i] = layout.decode(res[i])
                continue
            for off, name in enumerate(names):
                j = j0 + off
                targets[j], star_num[j], scenarios[j] = ID, snum, name
                if res is None:
                    lnZ[j] = -np.inf
                    continue
                r = res[off]
                for c in _COLS:
                    best[c][j] = r[c]
                lnZ[j] = r["lnZ"]
                extras[j] = r.get(layout.extra_key or "posterior") if isinstance(r, dict) else None
        if rec_tab is not None:
            for i, c in enumerate(sharding.RECORD_COLS[:-1]):
                best[c] = best[c] + rec_tab[:, i]         # (rows of dict-valued or dropped units stay as filled above)

        relative_probs, status = _normalize_probabilities(lnZ)
        if warn:
            self._warn_status(status, stacklevel=4)
        self.FPP_degenerate = status in ('anomaly', 'all_neginf')

        self._probs_columns = {
            "ID": targets, "scenario": scenarios, "M_s": best["M_s"], "R_s": best["R_s"],
            "P_orb": best["P_orb"], "inc": best["inc"], "b": best["b"], "ecc": best["ecc"],
            "w": best["argp"], "R_p": best["R_p"], "M_EB": best["M_EB"], "R_EB": best["R_EB"],
            "prob": relative_probs}
        self._probs = None
        self.lnZ = lnZ
        self.posterior = extras if summary_q is None else None
        self.posterior_quantiles = extras if summary_q is not None else None
        self._posterior_q = None if summary_q is None else tuple(float(x) for x in summary_q)
        self.star_num = star_num
        self.u1 = best["u1"]
        self.u2 = best["u2"]
        self.fluxratio_EB = best["fluxratio_EB"]
        self.fluxratio_comp = best["fluxratio_comp"]
        prob = relative_probs
        self.FPP = 1 - (prob[0] + prob[3] + prob[9])
        self.NFPP = np.sum(prob[15:]) if len(prob) > 15 else 0.0
        # what the Monte-Carlo error of this table is made from; the error attributes below are
        # computed when one of them is first read, like .probs (a 64-target step reads none of them)
        self._mc_inputs = (lnZ, lnM2, lnWmax, n_draws, status)
        self._mc = None
        return

    def _mc_attr(self, name):
        d = self.__dict__
        inputs = d.get("_mc_inputs")
        if inputs is None:
            # (no table yet, or a deferred one: target.__getattr__ fills it and reads again)
            raise AttributeError("'%s' object has no attribute '%s'" % (type(self).__name__, name))
        if d.get("_mc") is None:
            lnZ, lnM2, lnWmax, n_draws, status = inputs
            mc = _mc_errors(lnZ, lnM2, n_draws, status)
            mc["w_max_frac"] = np.exp(lnWmax)
            d["_mc"] = mc
        return d["_mc"][name]

    # The Monte-Carlo error of the last calc_probs table: per scenario row the effective sample size ess (0 where
    # lnZ = -inf), the standard error of lnZ (NaN where lnZ is not finite) and the largest draw's share of the evidence;
    # per target the delta-method errors of FPP and NFPP.  NaN where the run gave no moments.
    ess = property(lambda self: self._mc_attr("ess"))
    lnZ_err = property(lambda self: self._mc_attr("lnZ_err"))
    w_max_frac = property(lambda self: self._mc_attr("w_max_frac"))
    FPP_err = property(lambda self: self._mc_attr("FPP_err"))
    NFPP_err = property(lambda self: self._mc_attr("NFPP_err"))

    @staticmethod
    def _warn_status(status, stacklevel):
        """the reference's RuntimeWarnings for degenerate evidences (triceratops.py:1466-1478)"""
        if status == 'anomaly':
            warnings.warn(
                "Unexpected NaN or +inf in scenario log-evidences. This indicates a numerical "
                "anomaly unrelated to geometric exclusions. Inspect self.lnZ for diagnostics.",
                RuntimeWarning, stacklevel=stacklevel)
        elif status == 'all_neginf':
            warnings.warn(
                "All scenario log-evidences are -inf: every MC draw was geometrically invalid. "
                "FPP=1.0 reflects a failed computation, not a confident false positive. "
                "Inspect self.lnZ for diagnostics.",
                RuntimeWarning, stacklevel=stacklevel)

    # what _finish sets: a target whose table is still to be filled (calc_probs_many on several ranks) has none of them
    _RESULTS = ("lnZ", "star_num", "u1", "u2", "fluxratio_EB", "fluxratio_comp", "FPP", "NFPP", "FPP_degenerate",
                "_probs_columns", "_probs", "ess", "lnZ_err", "w_max_frac", "FPP_err", "NFPP_err", "_mc_inputs", "_mc",
                "posterior", "posterior_quantiles", "_posterior_q")

    def _defer_finish(self, units, results, n_scen, layout=None):
        """The table of this target is filled when one of its results is first read (calc_probs_many on several
        ranks: the targets another rank evaluated).  What is kept is DATA only -- per unit (first row, names, star
        number, ID) and a copy of its own records -- not the units' closures over light curves and star tables nor
        views into the whole batch's gathered table: the target pickles and copies like any other (advisor, round 5;
        __getstate__ fills the table first), and holds on to nothing of the batch.  The reference's RuntimeWarnings
        for degenerate evidences are raised HERE, where calc_probs_many was called, not at some later read."""
        d = self.__dict__
        for name in self._RESULTS:
            d.pop(name, None)                # (results of an earlier calc_probs must not be read as this one's)
        # (the units with their thunks dropped: the other fields are plain data, and the error attributes need the draws)
        slim = [u._replace(thunk=None) for u in sharding.as_units(units)]
        kept = [None if r is None else (np.array(r, copy=True) if isinstance(r, np.ndarray) else r) for r in results]
        layout = layout or sharding.RowLayout()
        d["_pending_finish"] = (slim, kept, n_scen, layout)
        lnz = np.full(n_scen, 0.0)
        for u, r in zip(slim, kept):
            mine = slice(u.first_row, u.first_row + len(u.names))
            if r is None:
                lnz[mine] = -np.inf
            elif isinstance(r, np.ndarray):
                lnz[mine] = r[:, layout.lnZ]
            else:
                lnz[mine] = [x["lnZ"] for x in r]
        if not np.all(np.isfinite(lnz)):      # (the common case costs one pass over ~20 numbers)
            self._warn_status(_normalize_probabilities(lnz)[1], stacklevel=4)

    def _finish_pending(self):
        d = object.__getattribute__(self, "__dict__")
        pend = d.get("_pending_finish")
        if pend is not None:
            d["_pending_finish"] = None
            self._finish(*pend[:3], warn=False, layout=pend[3])

    def __getattr__(self, name):
        # (only reached when normal lookup fails)
        d = object.__getattribute__(self, "__dict__")
        if d.get("_pending_finish") is not None and name in type(self)._RESULTS:
            self._finish_pending()
            return object.__getattribute__(self, name)
        raise AttributeError("'%s' object has no attribute '%s'" % (type(self).__name__, name))

    def __getstate__(self):
        # (pickle, copy.copy and copy.deepcopy all come through here: a table still to be filled is filled first)
        self._finish_pending()
        return self.__dict__

    @property
    def probs(self):
        """the scenario table of the last calc_probs (triceratops.py:1449-1463)"""
        if getattr(self, "_probs", None) is None:
            if getattr(self, "_probs_columns", None) is None:
                raise AttributeError("'target' object has no attribute 'probs'")
            self._probs = DataFrame(self._probs_columns)
        return self._probs

    @probs.setter
    def probs(self, value):
        self._probs = value

    # -----------------------------------------------------------------------------------
    def fit_curves(self, time, flux_0, flux_err_0: float, n_model: int = 100,
                   exptime: float = 0.00139, nsamples: int = 20):
        """Best-fit model light curve of every scenario of the last calc_probs: the data half of
        the reference's plot_fits (triceratops.py:1502-1597).

        Returns (model_time, curves): model_time = linspace(min(time), max(time), n_model) and one
        dict per row of .probs {ID, scenario, flux, flux_err, model}; flux/flux_err are the data
        renormalised to that scenario's host star, model is all ones for a skipped scenario.  All
        rows of one kind (TP / EB, companion-is-host or not) go to the GPU as one parameter block,
        with the reference's scalar-path radius-ratio rule (likelihoods.py:63-66, 122-131)."""
        time = np.asarray(time, dtype=np.float64)
        flux_0 = np.asarray(flux_0, dtype=np.float64)
        live = (self.probs["ID"] != 0).values       # rows calc_probs never reached keep ID 0
        df = self.probs[live]
        star_num, u1, u2 = self.star_num[live], self.u1[live], self.u2[live]
        fr_EB, fr_comp = self.fluxratio_EB[live], self.fluxratio_comp[live]
        model_time = np.linspace(np.min(time), np.max(time), n_model)
        star_ids = self.stars["ID"].astype(str).values
        models = np.ones((len(df), n_model))
        groups = {}
        for k in range(len(df)):
            if df["M_s"].values[k] == 0.0 or not np.isfinite(df["M_s"].values[k]):
                continue
            groups.setdefault((k % 3 == 0, bool(star_num[k] != 1)), []).append(k)
        t_d = _lib.dev(model_time)
        for (is_tp, comp), rows in groups.items():
            r = np.array(rows)
            model, flags, block = _model_block(is_tp, comp, {
                "M_s": df["M_s"].values[r], "M_EB": df["M_EB"].values[r], "P_orb": df["P_orb"].values[r],
                "inc": df["inc"].values[r], "R_s": df["R_s"].values[r], "u1": u1[r], "u2": u2[r],
                "ecc": df["ecc"].values[r], "argp": df["w"].values[r], "fluxratio_comp": fr_comp[r],
                "R_p": df["R_p"].values[r], "R_EB": df["R_EB"].values[r], "fluxratio_EB": fr_EB[r]})
            grid, _ = _lib.flux_grid(model, flags, t_d, _lib.dev(block), exptime, nsamples, want_secdepth=False)
            models[r] = grid.cpu().numpy()
        curves = []
        for k in range(len(df)):
            idx = np.argwhere(star_ids == str(df["ID"].values[k]))[0, 0]
            flux, flux_err = renorm_flux(flux_0, flux_err_0, self.stars["fluxratio"].values[idx])
            curves.append({"ID": df["ID"].values[k], "scenario": df["scenario"].values[k],
                           "flux": flux, "flux_err": flux_err, "model": models[k]})
        return model_time, curves

    def fit_bands(self, time, flux_0, flux_err_0: float, n_model: int = 100, q=(0.16, 0.5, 0.84),
                  exptime: float = 0.00139, nsamples: int = 20, model_average: int = 0, rng=None):
        """Posterior-predictive light-curve bands of every scenario of the last calc_posteriors (or
        calc_posteriors_many(keep="samples")): the model curve of EVERY posterior sample, reduced on the device to its
        pointwise quantiles `q`.  The companion of fit_curves, which gives the best draw's curve.

        Returns (model_time, bands): model_time as in fit_curves, and one dict per row of .probs {ID, scenario, flux,
        flux_err -- as fit_curves returns them --, q, band, n_samples}: band is the [len(q)][n_model] array
        np.quantile(curves of the row's samples, q, axis=0) in the normalisation of that scenario's host star, or None
        for a row without samples (n_samples = 0).  The parameter blocks are fit_curves' with every column taken from
        the samples; all samples of all rows of one kind (TP / EB, companion-is-host or not) go to the GPU as one block.

        model_average = n > 0 appends the band of the mixture of the scenarios in proportion to `prob` (scenario
        "model average", the target's ID, flux_0 and flux_err_0 as given): the quantiles over the curves of the n
        (scenario, sample) picks posterior_samples(n, rng) makes from the same rng, each curve taken back to the TARGET's
        normalisation, 1 - fluxratio_host (1 - curve).  That entry also names its picks: "rows" (the rows of .probs) and
        "samples" (the index into that row's samples)."""
        import torch
        from . import fused
        post = self._samples()
        if all(p is None for p in post):
            raise ValueError("no scenario with posterior samples carries probability")
        q = tuple(float(x) for x in np.atleast_1d(q))
        if not 1 <= len(q) <= _lib.QUANTILES_MAX or not all(0.0 <= x <= 1.0 for x in q):
            raise ValueError("q must hold 1 to %d quantile levels in [0, 1]" % _lib.QUANTILES_MAX)
        model_average = int(model_average)
        if not 0 <= model_average <= fused.POST_MAX_ROWS:
            raise ValueError("model_average must lie in [0, %d]" % fused.POST_MAX_ROWS)
        time = np.asarray(time, dtype=np.float64)
        flux_0 = np.asarray(flux_0, dtype=np.float64)
        live = np.flatnonzero((self.probs["ID"] != 0).values)       # rows calc_probs never reached keep ID 0
        df = self.probs.iloc[live]
        star_num = self.star_num[live]
        model_time = np.linspace(np.min(time), np.max(time), n_model)
        star_ids = self.stars["ID"].astype(str).values
        share = [self.stars["fluxratio"].values[np.argwhere(star_ids == str(ID))[0, 0]] for ID in df["ID"].values]
        # the samples of every row, grouped as fit_curves groups the rows; the groups' grids are consecutive row ranges
        # of ONE device grid, so that the mixture's gather list addresses them all
        groups, n_of = {}, np.zeros(len(df), dtype=np.int64)
        for k, j in enumerate(live):
            if post[j] is not None:
                n_of[k] = len(post[j]["lnw"])
                groups.setdefault((k % 3 == 0, bool(star_num[k] != 1)), []).append(k)
        first = np.zeros(len(df), dtype=np.int64)        # grid row of a row's sample 0
        t_d = _lib.dev(model_time)
        grid = torch.empty((int(n_of.sum()), n_model), dtype=torch.float64, device=t_d.device)
        at = 0
        for (is_tp, comp), rows in groups.items():
            model, flags, block = _model_block(is_tp, comp, {
                c: np.concatenate([np.asarray(post[live[k]][c], dtype=np.float64) for k in rows]) for c in _COLS})
            n = block.shape[1]
            _lib.flux_grid(model, flags, t_d, _lib.dev(block), exptime, nsamples, want_secdepth=False, out=grid[at:at + n])
            for k in rows:
                first[k], at = at, at + n_of[k]
        have = np.flatnonzero(n_of)
        bands_d = torch.empty((len(have) + (model_average > 0), len(q), n_model), dtype=torch.float64, device=t_d.device)
        for i, k in enumerate(have):
            bands_d[i] = _lib.grid_quantiles(grid[first[k]:first[k] + n_of[k]], q)
        if model_average:
            which, sample = self._mixture_picks(post, model_average, rng)
            at_live = {j: k for k, j in enumerate(live)}
            rows = np.array([first[at_live[j]] for j in which], dtype=np.int64) + sample
            scale = np.array([share[at_live[j]] for j in which], dtype=np.float64)
            bands_d[-1] = _lib.grid_quantiles(grid, q, rows_d=torch.as_tensor(rows).to(grid.device), scale_d=_lib.dev(scale))
        bands_h = bands_d.cpu().numpy()
        slot = {k: i for i, k in enumerate(have)}
        bands = []
        for k in range(len(df)):
            flux, flux_err = renorm_flux(flux_0, flux_err_0, share[k])
            bands.append({"ID": df["ID"].values[k], "scenario": df["scenario"].values[k], "flux": flux,
                          "flux_err": flux_err, "q": q, "band": bands_h[slot[k]] if k in slot else None,
                          "n_samples": int(n_of[k])})
        if model_average:
            bands.append({"ID": self.ID, "scenario": "model average", "flux": flux_0, "flux_err": flux_err_0, "q": q,
                          "band": bands_h[-1], "n_samples": model_average, "rows": which, "samples": sample})
        return model_time, bands


def calc_probs_many(jobs, verbose: int = 0):
    """calc_probs for several targets at once (BASELINE config 4: many TOIs over the GPUs of a node).

    jobs: sequence of (target, kwargs) with kwargs the calc_probs arguments of that target
    (time, flux_0, flux_err_0, P_orb, ...).  The (TOI, star, lnZ_* call) units of ALL jobs form one
    list, dealt to the ranks by size (N x n_time x scenario cost) and finished with the same single
    all_gather as one calc_probs; every target then gets its own table, FPP and NFPP.  On one GPU
    without per-unit seeding this is the jobs' calc_probs calls one after the other on one random
    stream."""
    from . import fused
    if fused.POSTERIOR_ROWS:
        raise NotImplementedError("posterior rows are not available in calc_probs_many: use calc_posteriors_many "
                                  "(or target.calc_posteriors)")
    return _probs_many(jobs, verbose)


def calc_posteriors_many(jobs, n_samples: int = 1000, keep: str = "samples", q=(0.16, 0.5, 0.84), verbose: int = 0):
    """calc_probs_many with posterior samples: the same pass over the same `jobs` -- from the same seed every table,
    `.lnZ`, `.FPP`, `.NFPP` and error attribute is bit for bit calc_probs_many's -- in which every lnZ_* call also draws
    n_samples of its draws in proportion to their weight in the evidence, inside the launch chains and under the same
    sharding.  Every target ends as target.calc_posteriors leaves it.

    keep="samples": `.posterior` holds the samples of every scenario row (posterior_summary, posterior_samples).  On
    several ranks the samples ride in the pass's one all_gather: 16 n_samples doubles per scenario row.
    keep="summary": the rank that evaluated a row reduces its samples to the quantiles `q` of the 14 physical columns
    (np.quantile, as posterior_summary takes them) before the gather, which then carries 14 len(q) doubles per row.
    The targets hold `.posterior_quantiles` -- per scenario row a dict column -> [len(q)] array, or None -- and
    `.posterior = None`; posterior_summary(q) returns the same DataFrame as from the samples, for this q only."""
    from . import fused
    n_samples = int(n_samples)
    if not 1 <= n_samples <= fused.POST_MAX_ROWS:
        raise ValueError("n_samples must lie in [1, %d]" % fused.POST_MAX_ROWS)
    if keep not in ("samples", "summary"):
        raise ValueError("keep must be 'samples' or 'summary', not %r" % (keep,))
    summary_q = None
    if keep == "summary":
        summary_q = tuple(float(x) for x in q)
        if not summary_q or not all(0.0 <= x <= 1.0 for x in summary_q):
            raise ValueError("q must be a non-empty sequence of quantile levels in [0, 1]")
    with fused.switches(POSTERIOR_ROWS=n_samples, POSTERIOR_SUMMARY=summary_q):
        out = _probs_many(jobs, verbose)
    for tg in out:
        if tg.__dict__.get("_pending_finish") is not None:
            continue                     # (another rank's target: its table is filled when it is first read)
        have = tg.posterior if summary_q is None else tg.posterior_quantiles
        if all(p is None for p in have) and np.isfinite(tg.lnZ).any():
            raise NotImplementedError("calc_posteriors_many needs the device paths (set_sampling('device') or "
                                      "'numpy-device'): this sampling mode returns no posterior rows")
    return out


def _probs_many(jobs, verbose):
    """the pass of calc_probs_many / calc_posteriors_many"""
    import time as _time
    t0 = _time.perf_counter()
    prepared = []
    for job, (tg, kw) in enumerate(jobs):
        kw = dict(kw)
        kw.pop("verbose", None)
        prepared.append((tg,) + tg._prepare(job=job, **kw))
    flat = [u for _, units, _ in prepared for u in units]
    t1 = _time.perf_counter()
    # (one rank: a target's table is filled as soon as its last record is in, while the GPU works on the later targets)
    finished = set()
    t_fin = [0.0]

    def job_done(job, res):
        t_a = _time.perf_counter()
        tg, units, n_scen = prepared[job]
        tg._finish(units, res, n_scen, layout=sharding.last_layout)
        finished.add(job)
        t_fin[0] += _time.perf_counter() - t_a

    results = sharding.run_units(flat, verbose=verbose, as_rows=True, job_done=job_done)
    t2 = _time.perf_counter()
    at = 0
    # Several ranks: every rank holds every record after the all_gather, and a rank fills the tables of the targets it
    # evaluated itself at once; the others' are filled when one of their results is first read (target.__getattr__) --
    # filling all 64 tables of a batch on each of eight ranks was a quarter of a rank's host path.
    many_ranks, layout = sharding._dist() is not None, sharding.last_layout
    for job, (tg, units, n_scen) in enumerate(prepared):
        if job not in finished:
            if many_ranks and job not in sharding.last_own_jobs:
                tg._defer_finish(units, results[at:at + len(units)], n_scen, layout)
            else:
                tg._finish(units, results[at:at + len(units)], n_scen, layout=layout)
        at += len(units)
    # every rank lists the units of all targets (cheap: no argument is built before a unit's owner calls it)
    # and fills every target's table from the gathered records; both are a few ms for 64 targets
    sharding.timing["prepare_s"] = t1 - t0
    sharding.timing["finish_s"] = _time.perf_counter() - t2 + t_fin[0]
    return [tg for tg, _ in jobs]
