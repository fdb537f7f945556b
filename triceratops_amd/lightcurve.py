"""Light-curve preparation in front of calc_probs: fold, trim and bin.

The reference has no code for this step: its notebooks hand it to lightkurve
(examples/TSCIII_tutorial.ipynb cell 5: `TessLightCurve(time, flux).bin(time_bin_size=...)` on the
points with |t| < 0.4 d; examples/example.ipynb folds with `lc.fold`).  lightkurve is not a
dependency here, so the same three operations are provided on plain numpy arrays; calc_probs
takes their output directly (it drops the NaN of empty bins itself, triceratops.py:707-709).
Bin edges follow lightkurve 2.x's fixed-width binning [recollection -- lightkurve is not in this
image]: bins of `time_bin_size` start at the first time stamp, each bin reports its centre and the
nan-mean of its fluxes, an empty bin reports NaN.
"""
import math

import numpy as np


def fold(time, period: float, epoch_time: float):
    """Days from the nearest transit midpoint, in [-period/2, period/2), sorted; returns
    (folded_time, order) so that flux[order] lines up with folded_time."""
    time = np.asarray(time, dtype=np.float64)
    phase = np.mod(time - epoch_time + 0.5 * period, period) - 0.5 * period
    order = np.argsort(phase, kind="stable")
    return phase[order], order


def trim(time, flux, half_width: float):
    """The points within `half_width` days of the transit midpoint."""
    time, flux = np.asarray(time, dtype=np.float64), np.asarray(flux, dtype=np.float64)
    keep = np.abs(time) < half_width
    return time[keep], flux[keep]


def bin_lightcurve(time, flux, time_bin_size: float = None, n_bins: int = None):
    """Fixed-width bins starting at min(time).  Give the width, or a bin count (the width is then
    the time span / n_bins).  Returns (bin centres, mean flux per bin, points per bin); empty bins
    hold NaN."""
    time, flux = np.asarray(time, dtype=np.float64), np.asarray(flux, dtype=np.float64)
    if time.size == 0:
        return np.empty(0), np.empty(0), np.empty(0, dtype=np.int64)
    if (time_bin_size is None) == (n_bins is None):
        raise ValueError("give exactly one of time_bin_size and n_bins")
    t0, span = np.min(time), np.max(time) - np.min(time)
    if time_bin_size is None:
        time_bin_size = span / n_bins if span > 0 else 1.0
    if not time_bin_size > 0:
        raise ValueError("time_bin_size must be positive")
    if n_bins is None:
        n_bins = int(np.floor(span / time_bin_size)) + 1
    idx = np.minimum(((time - t0) / time_bin_size).astype(np.int64), n_bins - 1)
    ok = ~np.isnan(flux)
    count = np.bincount(idx[ok], minlength=n_bins)
    total = np.bincount(idx[ok], weights=flux[ok], minlength=n_bins)
    mean = np.full(n_bins, np.nan)
    np.divide(total, count, out=mean, where=count > 0)
    centres = t0 + (np.arange(n_bins) + 0.5) * time_bin_size
    return centres, mean, count


def prepare(time, flux, half_width: float = 0.4, n_bins: int = 200, n_sigma: int = 50):
    """The tutorial's preparation in one call: trim to |t| < half_width, bin to `n_bins` bins of
    width 2 max|t| / n_bins, drop empty bins, and estimate the per-point uncertainty as the
    standard deviation of the first `n_sigma` (out-of-transit) binned points.
    Returns (time, flux, sigma) ready for calc_probs."""
    t, y = trim(time, flux, half_width)
    if t.size == 0:
        raise ValueError("no points within %g d of the transit midpoint" % half_width)
    tb, yb, _ = bin_lightcurve(t, y, time_bin_size=2 * np.max(t) / n_bins)
    keep = ~np.isnan(yb)
    tb, yb = tb[keep], yb[keep]
    return tb, yb, float(np.std(yb[:n_sigma]))


def polynomial_baseline(time, order: int):
    """[order][T] columns of a polynomial baseline for a dataset's "baseline" key: column p - 1 is u^p, p = 1 ... order,
    u = (t - mid) / half-span over the finite times, so u spans [-1, 1].  The constant term is not among them: it is the
    dataset's offset_sigma.  A NaN time gives NaN entries (dropped with the point)."""
    time = np.asarray(time, dtype=np.float64)
    order = int(order)
    if time.ndim != 1 or order < 1:
        raise ValueError("polynomial_baseline needs a 1-d time array and order >= 1")
    fin = time[np.isfinite(time)]
    if fin.size == 0 or np.max(fin) == np.min(fin):
        raise ValueError("polynomial_baseline needs at least two different finite times")
    lo, hi = float(np.min(fin)), float(np.max(fin))
    u = (time - 0.5 * (lo + hi)) / (0.5 * (hi - lo))
    return np.stack([u ** p for p in range(1, order + 1)])


def trend_columns(time, order: int, constant: bool = True):
    """[order + 1][T] columns u^0 ... u^order of a polynomial trend for a dataset's "red_baseline" key (constant=False:
    [order][T], u^1 ... u^order), u as in polynomial_baseline.  The column of ones is how the constant is given there: no
    offset_sigma stands next to red_baseline.  order = 0 (with the constant): the ones alone.  A NaN time gives NaN entries
    (dropped with the point), also in the constant."""
    time = np.asarray(time, dtype=np.float64)
    order = int(order)
    if time.ndim != 1 or order < 0 or (order == 0 and not constant):
        raise ValueError("trend_columns needs a 1-d time array and order >= 0 (>= 1 without the constant)")
    cols = polynomial_baseline(time, order) if order > 0 else np.empty((0, time.size))
    if constant:
        cols = np.concatenate([np.where(np.isnan(time), np.nan, 1.0)[None, :], cols])
    return np.ascontiguousarray(cols)


def red_noise_grid(sigmas, timescales, weights=None):
    """The product grid of candidate red-noise amplitudes and time scales as a dataset's "red_grid": a float64 array
    [len(sigmas) * len(timescales)][3] of rows (s_r, tau, weight), sigmas-major.  weights: None (equal), or an array
    [len(sigmas)][len(timescales)] of prior weights > 0; they are normalised to sum 1.  datasets.validate checks the
    values and the number of candidates (datasets.MAX_RED_CANDIDATES)."""
    s = np.atleast_1d(np.asarray(sigmas, dtype=np.float64))
    tau = np.atleast_1d(np.asarray(timescales, dtype=np.float64))
    if s.ndim != 1 or tau.ndim != 1 or s.size == 0 or tau.size == 0:
        raise ValueError("sigmas and timescales must be non-empty 1-d sequences")
    w = np.ones((s.size, tau.size)) if weights is None else np.asarray(weights, dtype=np.float64)
    if w.shape != (s.size, tau.size):
        raise ValueError("weights must have the shape (len(sigmas), len(timescales)) = %s (got %s)"
                         % ((s.size, tau.size), w.shape))
    if not np.all(np.isfinite(w) & (w > 0)):
        raise ValueError("every weight must be finite and > 0")
    ss, tt = np.meshgrid(s, tau, indexing="ij")
    return np.ascontiguousarray(np.stack([ss.ravel(), tt.ravel(), w.ravel() / w.sum()], axis=1))


def white_noise_grid(scales, jitters=(0.0,), weights=None):
    """The product grid of candidate error scales and jitters as a dataset's "white_grid": a float64 array
    [len(scales) * len(jitters)][3] of rows (scale k, jitter s, weight), scales-major: candidate (k, s) has the per-point
    variance k^2 flux_err^2 + s^2.  weights: None (equal), or an array [len(scales)][len(jitters)] of prior weights > 0; they
    are normalised to sum 1.  datasets.validate checks the values and the number of candidates
    (datasets.MAX_WHITE_CANDIDATES)."""
    k = np.atleast_1d(np.asarray(scales, dtype=np.float64))
    s = np.atleast_1d(np.asarray(jitters, dtype=np.float64))
    if k.ndim != 1 or s.ndim != 1 or k.size == 0 or s.size == 0:
        raise ValueError("scales and jitters must be non-empty 1-d sequences")
    w = np.ones((k.size, s.size)) if weights is None else np.asarray(weights, dtype=np.float64)
    if w.shape != (k.size, s.size):
        raise ValueError("weights must have the shape (len(scales), len(jitters)) = %s (got %s)"
                         % ((k.size, s.size), w.shape))
    if not np.all(np.isfinite(w) & (w > 0)):
        raise ValueError("every weight must be finite and > 0")
    kk, ss = np.meshgrid(k, s, indexing="ij")
    return np.ascontiguousarray(np.stack([kk.ravel(), ss.ravel(), w.ravel() / w.sum()], axis=1))


def t0_shift_grid(sigma, n: int = 5, span: float = 3.0):
    """A Gaussian prior on a dataset's transit-time shift as its "t0_grid": a float64 array [n][2] of rows (shift, weight),
    n odd, the shifts equally spaced over -span * sigma ... +span * sigma (the middle one exactly 0, the others mirror
    images), the weights proportional to exp(-0.5 (shift / sigma)^2) and normalised to sum 1.  sigma: the propagated
    ephemeris error sqrt(sigma_T0^2 + E^2 sigma_P^2), in the units of `time`.  n = 1: the single node 0."""
    sigma, span, n = float(sigma), float(span), int(n)
    if not (sigma > 0 and math.isfinite(sigma)) or not (span > 0 and math.isfinite(span)):
        raise ValueError("sigma and span must be finite and > 0")
    if n < 1 or n % 2 == 0:
        raise ValueError("n must be odd and >= 1 (got %d): the middle node is no shift" % n)
    half = n // 2
    k = np.arange(-half, half + 1, dtype=np.float64)
    u = k * (span / half) if half else k                          # (shift / sigma; symmetric in bits)
    w = np.exp(-0.5 * u * u)
    return np.ascontiguousarray(np.stack([u * sigma, w / math.fsum(w.tolist())], axis=1))


def prepare_dataset(time, flux, half_width: float = 0.4, n_bins: int = 200, n_sigma: int = 50,
                    exptime: float = 0.00139, nsamples: int = 20, offset_sigma: float = None,
                    baseline_order: int = 0, baseline_sigma=None, red_sigma: float = None, red_timescale: float = None,
                    red_grid=None, t0_grid=None, outlier_frac: float = None, outlier_scale: float = None,
                    red_baseline_order: int = None, red_baseline_sigma=None, red_kernel: str = None, white_grid=None,
                    red_kernel_baseline_order: int = None, red_kernel_baseline_sigma=None,
                    white_baseline_order: int = None, white_baseline_sigma=None):
    """prepare() for target.calc_probs_datasets: the same trimming and binning, but one error per bin.  Returns the dict
    {"time", "flux", "flux_err", "exptime", "nsamples", "offset_sigma", "baseline", "baseline_sigma"} of one dataset;
    empty bins are dropped.
    offset_sigma (None: no offset; a number > 0 or inf) is passed through: the prior of the dataset's baseline offset.
    baseline_order > 0: "baseline" = polynomial_baseline(kept bins' times, baseline_order), with baseline_sigma (a number
    or one per column; None: flat) passed through; 0: both keys are None.
    red_sigma, red_timescale (both or neither): the dataset's correlated noise, passed through as the keys of those names
    when given; red_kernel ("ou", "matern32" or "ou2": the kernel of that noise, the last with two amplitudes and two time
    scales) is passed through as the key "red_kernel" when given.  red_grid (red_noise_grid's result, or any list of (s_r, tau, weight)): candidates of that noise to
    marginalise, passed through as the key "red_grid" when given.  t0_grid (t0_shift_grid's result, or any list of (shift,
    weight)): nodes of a transit-time shift to marginalise, passed through as the key "t0_grid" when given.
    outlier_frac, outlier_scale (both or neither): the outlier-tolerant likelihood of the dataset's points, passed through
    as the keys of those names when given.
    red_baseline_order (None: no such key; >= 0): "red_baseline" = trend_columns(kept bins' times, red_baseline_order), the
    trend marginalised under the dataset's red_sigma / red_timescale, with red_baseline_sigma (a number or one per column;
    None: flat) passed through.
    white_grid (white_noise_grid's result, or any list of (scale, jitter, weight)): candidates of the size of the white noise
    to marginalise, passed through as the key "white_grid" when given.
    white_baseline_order (None: no such key; >= 0): "white_baseline" = trend_columns(kept bins' times, white_baseline_order),
    the trend marginalised under every candidate of white_grid, with white_baseline_sigma (a number or one per column;
    None: flat) passed through.
    red_kernel_baseline_order (None: no such key; >= 0): "red_kernel_baseline" = trend_columns(kept bins' times,
    red_kernel_baseline_order), the trend marginalised under the dataset's red_kernel = "matern32" or "ou2" noise, with
    red_kernel_baseline_sigma (a number or one per column; None: flat) passed through (keywords: they stand before the
    white_baseline pair in the signature).

    flux_err of a bin = s / sqrt(points in the bin), s the per-point scatter: s^2 is the mean over the first `n_sigma`
    (out-of-transit) bins of count x (bin flux - their mean)^2 -- a bin mean of c points scatters with s^2 / c.  With
    the same count in every bin all errors equal prepare()'s sigma."""
    t, y = trim(time, flux, half_width)
    if t.size == 0:
        raise ValueError("no points within %g d of the transit midpoint" % half_width)
    tb, yb, count = bin_lightcurve(t, y, time_bin_size=2 * np.max(t) / n_bins)
    keep = ~np.isnan(yb)
    tb, yb, count = tb[keep], yb[keep], count[keep]
    head = yb[:n_sigma]
    scatter = float(np.sqrt(np.mean(count[:n_sigma] * (head - np.mean(head)) ** 2)))
    baseline = polynomial_baseline(tb, baseline_order) if int(baseline_order) > 0 else None
    out = {"time": tb, "flux": yb, "flux_err": scatter / np.sqrt(count), "exptime": float(exptime),
           "nsamples": int(nsamples), "offset_sigma": offset_sigma, "baseline": baseline,
           "baseline_sigma": baseline_sigma}
    if red_sigma is not None or red_timescale is not None:
        out["red_sigma"], out["red_timescale"] = red_sigma, red_timescale
    if red_kernel is not None:
        out["red_kernel"] = red_kernel
    if red_grid is not None:
        out["red_grid"] = red_grid
    if t0_grid is not None:
        out["t0_grid"] = t0_grid
    if outlier_frac is not None or outlier_scale is not None:
        out["outlier_frac"], out["outlier_scale"] = outlier_frac, outlier_scale
    if red_baseline_order is not None:
        out["red_baseline"] = trend_columns(tb, red_baseline_order)
    if red_baseline_sigma is not None:
        out["red_baseline_sigma"] = red_baseline_sigma
    if red_kernel_baseline_order is not None:
        out["red_kernel_baseline"] = trend_columns(tb, red_kernel_baseline_order)
    if red_kernel_baseline_sigma is not None:
        out["red_kernel_baseline_sigma"] = red_kernel_baseline_sigma
    if white_grid is not None:
        out["white_grid"] = white_grid
    if white_baseline_order is not None:
        out["white_baseline"] = trend_columns(tb, white_baseline_order)
    if white_baseline_sigma is not None:
        out["white_baseline_sigma"] = white_baseline_sigma
    return out
