"""Several light curves with per-point flux errors: the input of target.calc_probs_datasets.

A dataset is one light curve with its own cadence: `time`, `flux`, `flux_err` (one number or one per point),
`exptime` and `nsamples`, and optionally `offset_sigma`: the standard deviation of a Gaussian prior on a constant
baseline offset of that light curve, marginalised per draw (inf: a flat prior).  This module is host side and numpy only: validation, the reference noise sigma_bar and the
per-star renormalisation.  A `Datasets` object is what the lnZ_* functions receive in place of `time` (with
flux = None and sigma = sigma_bar); only the device sampling modes evaluate it (fused._Scenario).
"""
import math
from typing import NamedTuple

import numpy as np

from .funcs import renorm_flux

MAX_DATASETS = 16
DEFAULT_EXPTIME, DEFAULT_NSAMPLES = 0.00139, 20


class Dataset(NamedTuple):
    time: np.ndarray          # [T] float64, no NaN
    flux: np.ndarray          # [T]
    flux_err: np.ndarray      # [T], finite and > 0
    exptime: float
    nsamples: int
    offset_sigma: float = None    # prior sigma of a constant baseline offset (inf: flat); None: no offset


def _offset_sigma(i, value):
    """a dataset's "offset_sigma": None, or a float > 0 (inf allowed)"""
    if value is None:
        return None
    if isinstance(value, (bool, str, bytes)) or not isinstance(value, (int, float, np.integer, np.floating)):
        raise ValueError("dataset %d: offset_sigma must be None, a number > 0 or inf (got %r)" % (i, value))
    value = float(value)
    if not value > 0:              # (also NaN)
        raise ValueError("dataset %d: offset_sigma must be None, a number > 0 or inf (got %r)" % (i, value))
    return value


def validate(datasets):
    """A list of 1 ... MAX_DATASETS dicts {time, flux, flux_err[, exptime, nsamples, offset_sigma]} -> a list of Dataset.  Points
    with a NaN time or flux are dropped together with their error; a scalar flux_err is broadcast.  ValueError for an
    empty list, too many datasets, mismatched lengths, an error that is not finite or not positive, a dataset
    without points, or an offset_sigma that is not None, a number > 0 or inf."""
    if isinstance(datasets, dict) or not hasattr(datasets, "__len__"):
        raise ValueError("datasets must be a list of dicts with the keys time, flux, flux_err")
    if len(datasets) == 0:
        raise ValueError("datasets is empty: give at least one light curve")
    if len(datasets) > MAX_DATASETS:
        raise ValueError("at most %d datasets (got %d)" % (MAX_DATASETS, len(datasets)))
    out = []
    for i, d in enumerate(datasets):
        unknown = set(d) - {"time", "flux", "flux_err", "exptime", "nsamples", "offset_sigma"}
        if unknown:
            raise ValueError("dataset %d: unknown key(s) %s" % (i, sorted(unknown)))
        for k in ("time", "flux", "flux_err"):
            if k not in d:
                raise ValueError("dataset %d has no '%s'" % (i, k))
        time = np.atleast_1d(np.asarray(d["time"], dtype=np.float64))
        flux = np.atleast_1d(np.asarray(d["flux"], dtype=np.float64))
        err = np.asarray(d["flux_err"], dtype=np.float64)
        if time.ndim != 1 or flux.shape != time.shape:
            raise ValueError("dataset %d: time and flux must be 1-d arrays of one length (got %s and %s)"
                             % (i, time.shape, flux.shape))
        if err.ndim == 0:
            err = np.full(time.shape, float(err))
        elif err.shape != time.shape:
            raise ValueError("dataset %d: flux_err must be a number or an array of len(time) = %d (got shape %s)"
                             % (i, time.size, err.shape))
        keep = ~np.isnan(time) & ~np.isnan(flux)
        time, flux, err = time[keep], flux[keep], err[keep]
        if time.size == 0:
            raise ValueError("dataset %d has no points left after dropping NaN" % i)
        if not np.all(np.isfinite(err) & (err > 0)):
            raise ValueError("dataset %d: every flux_err must be finite and > 0" % i)
        nsamples = int(d.get("nsamples", DEFAULT_NSAMPLES))
        if nsamples < 1:
            raise ValueError("dataset %d: nsamples must be >= 1" % i)
        out.append(Dataset(np.ascontiguousarray(time), np.ascontiguousarray(flux), np.ascontiguousarray(err),
                           float(d.get("exptime", DEFAULT_EXPTIME)), nsamples,
                           _offset_sigma(i, d.get("offset_sigma"))))
    return out


def sigma_ref(sets):
    """sigma_bar = (mean over all points of all datasets of 1 / sigma_t^2)^(-1/2): sigma itself where all errors are
    equal, and unchanged when a light curve is split into several datasets (the sums run over the points)"""
    return sigma_bar([s.flux_err for s in sets])


def sigma_bar(errs):
    """sigma_ref of a list of error arrays; where all entries are equal, that entry exactly (no rounding of the mean)"""
    lo, hi = min(float(np.min(e)) for e in errs), max(float(np.max(e)) for e in errs)
    if lo == hi:
        return lo
    # (math.fsum: the correctly rounded sum, so the order of the points -- how a light curve is split -- cannot enter)
    total = math.fsum(float(x) for e in errs for x in 1.0 / (np.asarray(e) * np.asarray(e)))
    count = sum(np.size(e) for e in errs)
    return float((total / count) ** -0.5)


class Datasets:
    """validated datasets in one star's normalisation, and their sigma_bar"""

    def __init__(self, sets):
        self.sets = tuple(sets)
        self.sigma_ref = sigma_ref(self.sets)

    def __len__(self):
        return len(self.sets)

    @property
    def has_offsets(self):
        return any(s.offset_sigma is not None for s in self.sets)

    @property
    def size(self):
        """points of all datasets together"""
        return sum(s.time.size for s in self.sets)

    def renorm(self, star_fluxratio):
        """funcs.renorm_flux on every dataset, elementwise on flux and flux_err; sigma_bar is taken afterwards.  A finite
        offset_sigma is an error in flux units and is divided by the flux ratio as the errors are: s^2 sum(1 / err^2) --
        and with it the factor of the marginal that the evidence drops -- is the same for every
        star."""
        out = []
        for s in self.sets:
            flux, err = renorm_flux(s.flux, s.flux_err, star_fluxratio)
            off = s.offset_sigma
            if off is not None and math.isfinite(off):
                off = off / star_fluxratio
            out.append(s._replace(flux=np.ascontiguousarray(flux), flux_err=np.ascontiguousarray(err), offset_sigma=off))
        return Datasets(out)
