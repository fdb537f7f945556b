"""Several light curves with per-point flux errors: the input of target.calc_probs_datasets.

A dataset is one light curve with its own cadence: `time`, `flux`, `flux_err` (one number or one per point),
`exptime` and `nsamples`, and optionally `offset_sigma`: the standard deviation of a Gaussian prior on a constant
baseline offset of that light curve, marginalised per draw (inf: a flat prior), and `baseline` / `baseline_sigma`: up to
MAX_BASELINE_TERMS columns B_k[t] of a linear baseline model sum_k c_k B_k[t] with priors c_k ~ N(0, s_k^2), marginalised
the same way (baseline_system), or `red_sigma` / `red_timescale`: correlated noise of standard deviation s_r with an
exponential kernel of time scale tau next to the white errors (ou_system) -- with `red_kernel` = "matern32" a Matern-3/2
kernel, with "ou2" two exponential terms (ss2_system) --, or `red_grid`: up to MAX_RED_CANDIDATES
weighted candidates (s_r, tau) of that noise, marginalised per draw (ou_mix_system); and next to any of these `t0_grid`: up
to MAX_T0_NODES weighted shifts of its stamps, marginalised per draw (t0_grids); next to `red_sigma` / `red_timescale` (and
`t0_grid`) alone `red_baseline` / `red_baseline_sigma`: up to MAX_BASELINE_TERMS baseline columns marginalised under that
correlated noise (red_baselines, ou_baseline_system), next to `red_kernel` = "matern32" / "ou2" (and `t0_grid`) alone
`red_kernel_baseline` / `red_kernel_baseline_sigma`: the same under that kernel's noise (red_kernel_baselines,
ss2_baseline_system); or, alone or next to `t0_grid`,
`outlier_frac` / `outlier_scale`: every point is with probability eps an outlier from a Gaussian kappa times wider than its
error, the membership integrated out per point and per draw (outliers, robust_constants); or, alone or next to `t0_grid`,
`white_grid`: up to MAX_WHITE_CANDIDATES weighted candidates (error scale k, jitter s) of the white noise's size,
marginalised per draw (white_grids, white_mix_system), and next to it `white_baseline` / `white_baseline_sigma`: up to
MAX_BASELINE_TERMS baseline columns marginalised under every candidate (white_baselines, white_baseline_system).  This module is host side and numpy only:
validation, the reference noise sigma_bar and the per-star renormalisation.  A `Datasets` object is what the lnZ_*
functions receive in place of `time` (with flux = None and sigma = sigma_bar); only the device sampling modes evaluate it
(fused._Scenario).
"""
import math
from typing import NamedTuple

import numpy as np

from .funcs import renorm_flux

MAX_DATASETS = 16
MAX_BASELINE_TERMS = 4          # terms of a dataset's linear baseline model, the offset_sigma term included
MIN_BASELINE_EIGENVALUE = 1e-6  # of the scaled system matrix: below it the columns count as collinear
MAX_RED_CANDIDATES = 8          # candidate (s_r, tau) pairs of a dataset's red_grid
MAX_T0_NODES = 8                # nodes (shift, weight) of a dataset's t0_grid
MAX_WHITE_CANDIDATES = 8        # candidate (scale, jitter) pairs of a dataset's white_grid
DEFAULT_EXPTIME, DEFAULT_NSAMPLES = 0.00139, 20


class Dataset(NamedTuple):
    time: np.ndarray          # [T] float64, no NaN
    flux: np.ndarray          # [T]
    flux_err: np.ndarray      # [T], finite and > 0
    exptime: float
    nsamples: int
    offset_sigma: float = None    # prior sigma of a constant baseline offset (inf: flat); None: no offset
    baseline: np.ndarray = None         # [K_b][T] columns of the linear baseline model, finite; None: none
    baseline_sigma: np.ndarray = None   # [K_b] prior sigmas of their coefficients (inf: flat); None without baseline
    red_grid: np.ndarray = None         # [J][3] candidates (s_r, tau, weight) of the correlated noise, weights sum to 1; None
    red_sigma: float = None       # standard deviation of the correlated (Ornstein-Uhlenbeck) noise, flux units; None: white
    red_timescale: float = None   # its time scale, in the units of `time` (inf allowed); None without red_sigma

    # The kernel of the correlated noise: None, the one exponential term of ou_system.  It is no field -- the fields are
    # what a Dataset of today's keys compares by -- but the record's type: validate returns a Matern32Dataset or an
    # Ou2Dataset for the other two kernels, and _replace (Datasets.renorm) keeps the type.
    red_kernel = None


class Matern32Dataset(Dataset):
    """a Dataset whose correlated noise is a Matern-3/2 term: red_sigma = s, red_timescale = l, both finite floats"""
    __slots__ = ()
    red_kernel = "matern32"


class Ou2Dataset(Dataset):
    """a Dataset whose correlated noise is two exponential terms: red_sigma = (s_1, s_2), red_timescale = (tau_1, tau_2),
    float64 arrays of two, all finite"""
    __slots__ = ()
    red_kernel = "ou2"


RED_KERNELS = {"matern32": Matern32Dataset, "ou2": Ou2Dataset}


class BaselineSystem(NamedTuple):
    """the linear system of a dataset's marginalised baseline terms (baseline_system)"""
    terms: tuple              # per term ("offset" | "baseline", index among the dataset's columns or None, prior sigma)
    D: np.ndarray             # [K] D_k = sum_t w_t B_k[t]^2
    A: np.ndarray             # [K][K] A~ = D^(-1/2) (B^T W B + diag(1 / s_k^2)) D^(-1/2)
    M: np.ndarray             # [K][K] A~^(-1), symmetric
    g: np.ndarray             # [K][T] g_k[t] = w_t B_k[t] / sqrt(D_k)
    lambda_min: float         # smallest eigenvalue of A~

    @property
    def minv(self):
        """M's upper triangle packed by rows: the `minv` of trx_chi2_grid_baseline"""
        return np.ascontiguousarray(self.M[np.triu_indices(self.M.shape[0])])


def linear_system(w, columns, sigmas):
    """BaselineSystem of the columns B [K][T] with prior sigmas [K] (inf: flat) under the weights w [T]; `terms` is left
    empty.  D_k by math.fsum; the off-diagonal of A~ in float64, its diagonal 1 + 1 / (s_k^2 D_k).  ValueError for a column
    whose D_k is 0 (or not finite); a singular A~ gives lambda_min <= 0 and M = None."""
    w = np.asarray(w, dtype=np.float64)
    B = np.atleast_2d(np.asarray(columns, dtype=np.float64))
    s = np.broadcast_to(np.asarray(sigmas, dtype=np.float64), (B.shape[0],))
    D = np.array([math.fsum((w * b * b).tolist()) for b in B])
    if not np.all(np.isfinite(D) & (D > 0)):
        raise ValueError("column %d is zero at every point" % int(np.flatnonzero(~(np.isfinite(D) & (D > 0)))[0]))
    g = (w * B) / np.sqrt(D)[:, None]
    A = (g * (1.0 / w)) @ g.T
    A = 0.5 * (A + A.T)
    with np.errstate(divide="ignore"):
        A[np.diag_indices_from(A)] = 1.0 + 1.0 / (s * s * D)          # (1 / inf^2 = 0: the flat prior)
    lam = float(np.linalg.eigvalsh(A)[0])
    M = None
    if lam > 0:
        try:
            M = np.linalg.inv(A)
            M = 0.5 * (M + M.T)
        except np.linalg.LinAlgError:
            M = None
    return BaselineSystem((), D, A, M, np.ascontiguousarray(g), lam)


def baseline_system(dataset):
    """The BaselineSystem of a Dataset's marginalised terms, or None when it has none: the ones column with offset_sigma
    first when offset_sigma is set, then the `baseline` columns with their baseline_sigma -- the one place that fixes the
    order of the terms, for the device path (fused._Scenario) and for the numpy statement (_numerics.baseline_halfchi2)."""
    cols, sig, terms = [], [], []
    if dataset.offset_sigma is not None:
        cols.append(np.ones(dataset.time.size))
        sig.append(dataset.offset_sigma)
        terms.append(("offset", None, float(dataset.offset_sigma)))
    if dataset.baseline is not None:
        for k, (b, s) in enumerate(zip(dataset.baseline, dataset.baseline_sigma)):
            cols.append(b)
            sig.append(s)
            terms.append(("baseline", k, float(s)))
    if not cols:
        return None
    w = 1.0 / (dataset.flux_err * dataset.flux_err)
    return linear_system(w, np.stack(cols), np.array(sig, dtype=np.float64))._replace(terms=tuple(terms))


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


def _baseline(i, value, sigma, n_given, keep, name="baseline"):
    """a dataset's "baseline" and "baseline_sigma" -> ([K_b][T kept] columns, [K_b] sigmas), or (None, None); name: the
    key the messages speak of ("red_baseline": the same rules for the columns under correlated noise)"""
    if value is None:
        if sigma is not None:
            raise ValueError("dataset %d: %s_sigma without %s" % (i, name, name))
        return None, None
    try:
        B = np.asarray(value, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("dataset %d: %s must be an array [K][len(time)] or [len(time)]" % (i, name)) from None
    if B.ndim == 1:
        B = B[None, :]
    if B.ndim != 2 or B.shape[0] < 1 or B.shape[1] != n_given:
        raise ValueError("dataset %d: %s must be an array [K][len(time)] or [len(time)], len(time) = %d (got shape %s)"
                         % (i, name, n_given, np.shape(value)))
    B = B[:, keep]
    if not np.all(np.isfinite(B)):
        raise ValueError("dataset %d: every %s entry of a kept point must be finite" % (i, name))
    msg = "dataset %d: %s_sigma must be a number or %d numbers, each > 0 or inf (got %r)" % (i, name, B.shape[0], sigma)
    if sigma is None:
        s = np.full(B.shape[0], np.inf)
    else:
        if isinstance(sigma, (bool, str, bytes)):
            raise ValueError(msg)
        try:
            s = np.asarray(sigma, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(msg) from None
        if s.ndim == 0:
            s = np.full(B.shape[0], float(s))
        if s.shape != (B.shape[0],) or not np.all(s > 0):            # (also NaN)
            raise ValueError(msg)
    return np.ascontiguousarray(B), np.ascontiguousarray(s)


def _red_noise(i, sigma, timescale, time, others):
    """a dataset's "red_sigma" and "red_timescale" -> (s_r, tau) or (None, None); time: the kept stamps; others: whether
    the dataset marginalises an offset or a baseline as well"""
    if sigma is None and timescale is None:
        return None, None
    if sigma is None or timescale is None:
        raise ValueError("dataset %d: red_sigma and red_timescale are given together or not at all" % i)
    for name, value in (("red_sigma", sigma), ("red_timescale", timescale)):
        if isinstance(value, (bool, str, bytes)) or not isinstance(value, (int, float, np.integer, np.floating)):
            raise ValueError("dataset %d: %s must be a number > 0 (got %r)" % (i, name, value))
    sigma, timescale = float(sigma), float(timescale)
    if not (sigma > 0 and math.isfinite(sigma)):              # (also NaN)
        raise ValueError("dataset %d: red_sigma must be a finite number > 0 (got %r)" % (i, sigma))
    if not timescale > 0:
        raise ValueError("dataset %d: red_timescale must be a number > 0 or inf (got %r)" % (i, timescale))
    if others:
        raise ValueError("dataset %d: red_sigma together with offset_sigma or baseline is not built (a generalised "
                         "least-squares problem): give the correlated noise or the marginalised terms" % i)
    if np.any(np.diff(time) < 0):
        raise ValueError("dataset %d: red_sigma needs time in non-decreasing order: the noise model is a process in "
                         "time and follows the stamps as given (a folded light curve is not sorted silently)" % i)
    return sigma, timescale


def _red_kernel(i, value):
    """a dataset's "red_kernel" -> None (absent, None or "ou": the one exponential term), "matern32" or "ou2" (the others)"""
    if value is None or (isinstance(value, str) and value == "ou"):
        return None
    if not isinstance(value, str) or value not in RED_KERNELS:
        raise ValueError("dataset %d: red_kernel must be None, 'ou', 'matern32' or 'ou2' (got %r)" % (i, value))
    return value


def _red_terms(i, kernel, sigma, timescale, time, others):
    """a dataset's "red_sigma" and "red_timescale" under red_kernel = "matern32" (two finite numbers > 0) or "ou2" (two
    arrays of two, every entry finite and > 0) -> (sigma, timescale) as floats or contiguous float64 arrays; time: the kept
    stamps; others: the names of the keys of the dataset that do not stand next to these kernels"""
    n = {"matern32": 0, "ou2": 2}[kernel]
    want = "a finite number > 0" if n == 0 else "two finite numbers > 0"
    out = []
    for name, value in (("red_sigma", sigma), ("red_timescale", timescale)):
        msg = "dataset %d: %s must be %s with red_kernel = %r (got %r)" % (i, name, want, kernel, value)
        if value is None or isinstance(value, (bool, np.bool_, str, bytes)):
            raise ValueError(msg)
        try:
            if not isinstance(value, np.ndarray) or value.dtype.kind not in "iuf":
                # (a bool or a string among the entries would convert silently)
                if any(isinstance(x, (bool, np.bool_, str, bytes)) for x in np.asarray(value, dtype=object).ravel()):
                    raise TypeError
            v = np.array(value, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(msg) from None
        if v.shape != ((n,) if n else ()) or not np.all(np.isfinite(v) & (v > 0)):       # (also NaN)
            raise ValueError(msg)
        out.append(np.ascontiguousarray(v) if n else float(v))
    if others:
        raise ValueError("dataset %d: red_kernel = %r together with %s is not built: the kernel stands next to red_sigma / "
                         "red_timescale and t0_grid alone (baseline columns marginalised under it go under "
                         "red_kernel_baseline / red_kernel_baseline_sigma)" % (i, kernel, ", ".join(others)))
    if np.any(np.diff(time) < 0):
        raise ValueError("dataset %d: red_sigma needs time in non-decreasing order: the noise model is a process in "
                         "time and follows the stamps as given (a folded light curve is not sorted silently)" % i)
    return out[0], out[1]


def _red_grid(i, value, time, others):
    """a dataset's "red_grid" -> [J][3] float64 rows (s_r, tau, weight), the weights normalised to sum 1, or None; time:
    the kept stamps; others: whether the dataset has red_sigma / red_timescale, an offset or a baseline as well"""
    if value is None:
        return None
    msg = ("dataset %d: red_grid must be 1 ... %d triples (s_r, tau, weight): s_r finite and > 0, tau > 0 or inf, weight "
           "finite and > 0 (got %r)" % (i, MAX_RED_CANDIDATES, value))
    if isinstance(value, (bool, str, bytes)):
        raise ValueError(msg)
    try:
        g = np.array(value, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(msg) from None
    if g.ndim != 2 or g.shape[1] != 3 or not 1 <= g.shape[0] <= MAX_RED_CANDIDATES:
        raise ValueError(msg)
    s_r, tau, weight = g[:, 0], g[:, 1], g[:, 2]
    if not (np.all(np.isfinite(s_r) & (s_r > 0)) and np.all(tau > 0) and np.all(np.isfinite(weight) & (weight > 0))):
        raise ValueError(msg)                                     # (also NaN)
    if others:
        raise ValueError("dataset %d: red_grid together with red_sigma / red_timescale, offset_sigma or baseline is not "
                         "built: give the candidates alone (a single pair is a red_grid of one row)" % i)
    if np.any(np.diff(time) < 0):
        raise ValueError("dataset %d: red_grid needs time in non-decreasing order: the noise model is a process in "
                         "time and follows the stamps as given (a folded light curve is not sorted silently)" % i)
    total = math.fsum(weight.tolist())
    if not (math.isfinite(total) and total > 0):
        raise ValueError(msg)
    g[:, 2] = weight / total
    return np.ascontiguousarray(g)


def _t0_grid(i, value):
    """a dataset's "t0_grid" -> [J][2] float64 rows (shift, weight), the weights normalised to sum 1, or None"""
    if value is None:
        return None
    msg = ("dataset %d: t0_grid must be 1 ... %d pairs (shift, weight): the shifts finite and all different, the weights "
           "finite and > 0 (got %r)" % (i, MAX_T0_NODES, value))
    if isinstance(value, (bool, str, bytes)):
        raise ValueError(msg)
    try:
        if not isinstance(value, np.ndarray) or value.dtype.kind not in "iuf":
            # (a bool or a string among the entries would convert silently)
            if any(isinstance(x, (bool, np.bool_, str, bytes)) for x in np.asarray(value, dtype=object).ravel()):
                raise TypeError
        g = np.array(value, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(msg) from None
    if g.ndim != 2 or g.shape[1] != 2 or not 1 <= g.shape[0] <= MAX_T0_NODES:
        raise ValueError(msg)
    shift, weight = g[:, 0], g[:, 1]
    if not (np.all(np.isfinite(shift)) and np.all(np.isfinite(weight) & (weight > 0))):
        raise ValueError(msg)                                     # (also NaN)
    if np.unique(shift).size != shift.size:
        raise ValueError(msg)
    total = math.fsum(weight.tolist())
    if not (math.isfinite(total) and total > 0):
        raise ValueError(msg)
    g[:, 1] = weight / total
    return np.ascontiguousarray(g)


def t0_grids(dicts, sets):
    """The "t0_grid" keys of the dicts that validate() turned into `sets`: per dataset None, or a contiguous float64 [J][2]
    array of J = 1 ... MAX_T0_NODES rows (shift_j, weight_j) -- shifts in the units of `time`, finite and all different;
    weights finite and > 0, normalised to sum 1 (math.fsum).  The dataset's term of the log-weight, h_j on the stamps
    time + shift_j, becomes -ln sum_j weight_j exp(-h_j) (_numerics.t0_mix_halfchi2).  The key stands next to any other key
    of the dataset: a shift leaves the stamp differences, the index-aligned baseline columns and the determinants as they
    are.  ValueError for a wrong shape, too many rows, a value that is not finite, repeated shifts, a weight <= 0, a bool
    or a string.  Dataset itself has no field for the key: the grids travel in Datasets.t0_grids."""
    if len(dicts) != len(sets):
        raise ValueError("t0_grids: %d dicts for %d datasets" % (len(dicts), len(sets)))
    return [_t0_grid(i, d.get("t0_grid")) for i, d in enumerate(dicts)]


OUTLIER_KEYS = ("outlier_frac", "outlier_scale")


def _outliers(i, d, dataset):
    """a dataset's "outlier_frac" and "outlier_scale" -> (frac, scale) as Python floats, or None; dataset: the validated
    Dataset of the same dict (what else it marginalises)"""
    frac, scale = d.get("outlier_frac"), d.get("outlier_scale")
    if frac is None and scale is None:
        return None
    if frac is None or scale is None:
        raise ValueError("dataset %d: outlier_frac and outlier_scale are given together or not at all" % i)
    for name, value in (("outlier_frac", frac), ("outlier_scale", scale)):
        if isinstance(value, (bool, np.bool_, str, bytes)) or not isinstance(value, (int, float, np.integer, np.floating)):
            raise ValueError("dataset %d: %s must be a number (got %r)" % (i, name, value))
    frac, scale = float(frac), float(scale)
    if not 0.0 < frac <= 0.5:                                     # (also NaN)
        raise ValueError("dataset %d: outlier_frac must lie in (0, 0.5] (got %r)" % (i, frac))
    if not (scale > 1.0 and math.isfinite(scale)):                # (also NaN)
        raise ValueError("dataset %d: outlier_scale must be a finite number > 1 (got %r)" % (i, scale))
    if (dataset.offset_sigma is not None or dataset.baseline is not None or dataset.red_sigma is not None
            or dataset.red_grid is not None):
        raise ValueError("dataset %d: outlier_frac / outlier_scale together with offset_sigma, baseline, red_sigma / "
                         "red_timescale or red_grid is not built: the mixture has no closed form next to a marginalised "
                         "linear term or a correlated residual" % i)
    return frac, scale


def outliers(dicts, sets):
    """The "outlier_frac" / "outlier_scale" keys of the dicts that validate() turned into `sets`: per dataset None, or the
    tuple (frac, scale) of Python floats -- both keys or neither; 0 < frac <= 0.5: the prior probability eps that a point is
    an outlier; scale finite and > 1: the factor kappa by which an outlier's Gaussian is wider than the point's flux_err.
    The dataset's term of the log-weight, 0.5 sum_t w_t d_t^2, becomes sum_t -ln[(1 - eps) e^(-a_t) + (eps / kappa)
    e^(-a_t / kappa^2)], a_t = 0.5 w_t d_t^2 (_numerics.robust_halfchi2 on robust_constants).  The keys stand alone or next to
    t0_grid; next to offset_sigma, baseline, red_sigma / red_timescale or red_grid they are a ValueError, as is a bool, a
    string, an array, a NaN or an inf.  Dataset itself has no field for the keys: the pairs travel in Datasets.outliers."""
    if len(dicts) != len(sets):
        raise ValueError("outliers: %d dicts for %d datasets" % (len(dicts), len(sets)))
    return [_outliers(i, d, s) for i, (d, s) in enumerate(zip(dicts, sets))]


WHITE_GRID_NEIGHBOURS = ("offset_sigma", "baseline", "baseline_sigma", "red_sigma", "red_timescale", "red_grid", "red_kernel",
                         "red_baseline", "red_baseline_sigma") + OUTLIER_KEYS


def _white_grid(i, d):
    """a dataset's "white_grid" -> [J][3] float64 rows (scale k, jitter s, weight), the weights normalised to sum 1, or
    None; d: the dataset's dict (what else it asks for)"""
    value = d.get("white_grid")
    if value is None:
        return None
    msg = ("dataset %d: white_grid must be 1 ... %d triples (scale, jitter, weight): scale finite and > 0, jitter finite and "
           ">= 0, weight finite and > 0 (got %r)" % (i, MAX_WHITE_CANDIDATES, value))
    if isinstance(value, (bool, str, bytes)):
        raise ValueError(msg)
    try:
        if not isinstance(value, np.ndarray) or value.dtype.kind not in "iuf":
            # (a bool or a string among the entries would convert silently)
            if any(isinstance(x, (bool, np.bool_, str, bytes)) for x in np.asarray(value, dtype=object).ravel()):
                raise TypeError
        g = np.array(value, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(msg) from None
    if g.ndim != 2 or g.shape[1] != 3 or not 1 <= g.shape[0] <= MAX_WHITE_CANDIDATES:
        raise ValueError(msg)
    scale, jitter, weight = g[:, 0], g[:, 1], g[:, 2]
    if not (np.all(np.isfinite(scale) & (scale > 0)) and np.all(np.isfinite(jitter) & (jitter >= 0))
            and np.all(np.isfinite(weight) & (weight > 0))):
        raise ValueError(msg)                                     # (also NaN)
    others = [k for k in WHITE_GRID_NEIGHBOURS if d.get(k) is not None]
    if others:
        raise ValueError("dataset %d: white_grid together with %s is not built: the candidates stand alone or next to t0_grid "
                         "(baseline columns marginalised under every candidate go under white_baseline / white_baseline_sigma)"
                         % (i, ", ".join(others)))
    total = math.fsum(weight.tolist())
    if not (math.isfinite(total) and total > 0):
        raise ValueError(msg)
    g[:, 2] = weight / total
    return np.ascontiguousarray(g)


def white_grids(dicts, sets):
    """The "white_grid" keys of the dicts that validate() turned into `sets`: per dataset None, or a contiguous float64
    [J][3] array of J = 1 ... MAX_WHITE_CANDIDATES rows (k_j, s_j, weight_j) -- an error scale k finite and > 0, a jitter s
    finite and >= 0 in flux units, a prior weight finite and > 0, normalised to sum 1 (math.fsum); repeated pairs are
    allowed.  Candidate j has the per-point variance k_j^2 flux_err_t^2 + s_j^2, and the dataset's term of the log-weight
    becomes -ln sum_j c_j exp(-h_j) (_numerics.white_mix_halfchi2 on white_mix_system).  No condition on the order of the
    stamps.  The key stands alone, next to t0_grid or with white_baseline / white_baseline_sigma (white_baselines); next to offset_sigma, baseline, red_sigma / red_timescale, red_grid,
    red_kernel, red_baseline / red_baseline_sigma or the outlier keys it is a ValueError, as is a wrong shape, too many
    rows, a value that is not finite, a scale <= 0, a jitter < 0, a weight <= 0, a bool or a string.  Dataset itself has no
    field for the key: the grids travel in Datasets.white_grids."""
    if len(dicts) != len(sets):
        raise ValueError("white_grids: %d dicts for %d datasets" % (len(dicts), len(sets)))
    return [_white_grid(i, d) for i, d in enumerate(dicts)]


def white_mix_system(dataset, grid):
    """(w [J][T], lnc [J]), float64: the per-point weights of every candidate (k_j, s_j, pi_j) of a dataset's white_grid
    [J][3] and the candidates' log-weights,
        w_j[t] = 1 / (k_j^2 flux_err_t^2 + s_j^2),
        lnc_j = ln pi_j + 0.5 sum_t ln w_j[t] - logsumexp_j(the same),
    so that sum_j exp(lnc_j) = 1 and the dataset's term of the log-weight is -ln sum_j exp(lnc_j - h_j),
    h_j = 0.5 sum_t w_j[t] y_t^2 (_numerics.white_mix_halfchi2, trxv_chi2_grid_white_mix) -- the one place that forms them,
    for the device path (fused._Dataset) and for the numpy statement.  The candidate (1, 0) has the bits of
    1 / (flux_err * flux_err), a power-of-two k those of the same errors scaled.  The sums are math.fsum's; the normaliser
    that is dropped, sum_j pi_j prod_t w_j[t]^(1/2), depends on the dataset alone."""
    err = np.asarray(dataset.flux_err, dtype=np.float64)
    grid = np.asarray(grid, dtype=np.float64)
    w, terms = [], []
    for k_j, s_j, weight in grid:
        k_j, s_j = float(k_j), float(s_j)
        w_j = 1.0 / ((k_j * k_j) * (err * err) + s_j * s_j)
        w.append(w_j)
        terms.append([math.log(weight)] + (0.5 * np.log(w_j)).tolist())
    # (the raw values are large -- half a log-determinant --, their differences are not: the difference to the largest is
    # one correctly rounded sum over both candidates' terms, so the spacing of the raw values does not enter)
    top = [-v for v in max(terms, key=math.fsum)]
    diff = [math.fsum(t + top) for t in terms]
    norm = math.log(math.fsum(math.exp(v) for v in diff))
    lnc = np.array([v - norm for v in diff])
    return np.ascontiguousarray(np.stack(w)), lnc


WHITE_BASELINE_KEYS = ("white_baseline", "white_baseline_sigma")


class WhiteBaselineSystem(NamedTuple):
    """the candidates' weights of a dataset's white_grid and, per candidate, the linear system of its baseline columns
    under those weights (white_baseline_system)"""
    w: np.ndarray             # [J][T] w_j[t] = 1 / (k_j^2 flux_err_t^2 + s_j^2), as white_mix_system forms them
    B: np.ndarray             # [K][T] the columns as given
    minv: np.ndarray          # [J][K (K + 1) / 2] A_j^-1, upper triangle packed by rows, in the units of b_jk = sum w_j B_k y
    lnc: np.ndarray           # [J] ln pi_j + 0.5 sum_t ln w_j[t] - 0.5 ln det A_j, less their log-sum-exp
    lambda_min: np.ndarray    # [J] smallest eigenvalue of the unit-diagonal scaling A~_j of A_j
    D: np.ndarray             # [J][K] D_jk = sum_t w_j[t] B_k[t]^2
    M: tuple                  # per candidate [K][K] A~_j^-1 (None where A~_j is singular)


def white_baseline_system(dataset, grid, B, sigmas):
    """WhiteBaselineSystem of the columns B [K][T] with prior sigmas [K] (inf: flat) under every candidate (k_j, s_j, pi_j)
    of a dataset's white_grid [J][3] -- the one place that forms them, for the device path (fused._Dataset) and for the
    numpy statement (_numerics.white_baseline_halfchi2).  Per candidate linear_system(w_j, B, sigmas) gives D_j, the
    unit-diagonal A~_j = D_j^(-1/2) A_j D_j^(-1/2), A_j = B^T W_j B + diag(1 / s_k^2), and M_j = A~_j^-1; then
        A_j^-1 = D_j^(-1/2) M_j D_j^(-1/2),      ln det A_j = ln det A~_j + sum_k ln D_jk,
        lnc_j = ln pi_j + 0.5 sum_t ln w_j[t] - 0.5 ln det A_j - logsumexp_j(the same),
    so that the dataset's term of the log-weight is -ln sum_j exp(lnc_j - h_j), h_j = 0.5 max(S2_j - b_j^T A_j^-1 b_j, 0).  For
    finite priors that is -ln sum_j pi_j N(y; 0, diag(1 / w_j) + B diag(s^2) B^T) up to a constant of the dataset: det(I +
    diag(s^2) B^T W_j B) = det A_j prod_k s_k^2.  The lnc are formed as white_mix_system forms them: the difference to the
    largest is one math.fsum over both candidates' terms.  ValueError for a column whose D_jk is 0 (or not finite); a
    singular A~_j gives lambda_min[j] <= 0, M[j] = None and NaN in minv[j] and lnc."""
    B = np.ascontiguousarray(np.atleast_2d(np.asarray(B, dtype=np.float64)))
    K = B.shape[0]
    w, _ = white_mix_system(dataset, grid)
    grid = np.asarray(grid, dtype=np.float64)
    iu = np.triu_indices(K)
    minv, lam, Ds, Ms, terms = [], [], [], [], []
    for w_j, (_, _, weight) in zip(w, grid):
        system = linear_system(w_j, B, sigmas)
        lam.append(system.lambda_min)
        Ds.append(system.D)
        Ms.append(system.M)
        if system.M is None:
            minv.append(np.full(iu[0].size, np.nan))
            terms.append([math.nan])
            continue
        rs = 1.0 / np.sqrt(system.D)
        minv.append((system.M * rs[:, None] * rs[None, :])[iu])
        sign, lndet = np.linalg.slogdet(system.A)
        terms.append([math.log(weight)] + (0.5 * np.log(w_j)).tolist() + [-0.5 * float(lndet)]
                     + (-0.5 * np.log(system.D)).tolist())
    if any(M is None for M in Ms):
        lnc = np.full(len(terms), np.nan)
    else:
        top = [-v for v in max(terms, key=math.fsum)]
        diff = [math.fsum(t + top) for t in terms]
        norm = math.log(math.fsum(math.exp(v) for v in diff))
        lnc = np.array([v - norm for v in diff])
    return WhiteBaselineSystem(w, B, np.ascontiguousarray(np.stack(minv)), lnc, np.array(lam), np.stack(Ds), tuple(Ms))


def _white_baseline(i, d, dataset):
    """a dataset's "white_baseline" and "white_baseline_sigma" -> ([K_b][T kept] columns, [K_b] sigmas), or None; dataset:
    the validated Dataset of the same dict (its errors)"""
    value, sigma = d.get("white_baseline"), d.get("white_baseline_sigma")
    if isinstance(value, (bool, np.bool_, str, bytes)):
        raise ValueError("dataset %d: white_baseline must be an array [K][len(time)] or [len(time)] (got %r)" % (i, value))
    time = np.atleast_1d(np.asarray(d["time"], dtype=np.float64))
    keep = ~np.isnan(time) & ~np.isnan(np.atleast_1d(np.asarray(d["flux"], dtype=np.float64)))
    B, s = _baseline(i, value, sigma, time.size, keep, name="white_baseline")
    if B is None:
        return None
    if B.shape[0] > MAX_BASELINE_TERMS:
        raise ValueError("dataset %d: at most %d white_baseline columns (got %d)" % (i, MAX_BASELINE_TERMS, B.shape[0]))
    others = [k for k in WHITE_GRID_NEIGHBOURS if d.get(k) is not None]
    if others:
        raise ValueError("dataset %d: white_baseline together with %s is not built: the columns stand next to white_grid (and "
                         "t0_grid) alone; a column of ones is the constant" % (i, ", ".join(others)))
    grid = _white_grid(i, d)
    if grid is None:
        raise ValueError("dataset %d: white_baseline needs white_grid: with the errors as given give the columns as "
                         "baseline" % i)
    try:
        system = white_baseline_system(dataset, grid, B, s)
    except ValueError as e:
        raise ValueError("dataset %d: white_baseline term %s" % (i, e)) from None
    if not np.all(system.lambda_min >= MIN_BASELINE_EIGENVALUE):
        raise ValueError("dataset %d: the white_baseline terms are collinear under a candidate's weights (smallest "
                         "eigenvalue of the scaled system %.3g < %g): drop a column, or give finite priors"
                         % (i, float(np.min(system.lambda_min)), MIN_BASELINE_EIGENVALUE))
    return B, s


def white_baselines(dicts, sets):
    """The "white_baseline" / "white_baseline_sigma" keys of the dicts that validate() turned into `sets`: per dataset None,
    or the pair (B, sigmas) -- B a contiguous float64 [K_b][kept points] array of K_b = 1 ... MAX_BASELINE_TERMS columns of a
    linear baseline model sum_k c_k B_k[t], aligned with `time` (entries of NaN-dropped points dropped with them, every
    kept entry finite), sigmas [K_b] the prior sigmas of c_k ~ N(0, s_k^2), each > 0 or inf (absent: flat) -- marginalised
    per draw under every candidate of the dataset's white_grid, determinants included: its term of the log-weight becomes
    -ln sum_j exp(lnc_j - h_j), h_j = 0.5 [S2_j - b_j^T A_j^-1 b_j] (_numerics.white_baseline_halfchi2 on
    white_baseline_system).  A column of ones is how the constant is given.  The keys stand only next to white_grid, and may
    stand next to t0_grid (the columns follow the points); ValueError without white_grid, next to offset_sigma, baseline,
    any red key or outlier_frac / outlier_scale, for a sigma without columns, a wrong shape, more than MAX_BASELINE_TERMS
    columns, a kept entry that is not finite, a zero column, a bool or a string, or columns that are collinear under a
    candidate's weights (smallest eigenvalue of a scaled system < MIN_BASELINE_EIGENVALUE).  Dataset itself has no field
    for the keys: the pairs travel in Datasets.white_baselines."""
    if len(dicts) != len(sets):
        raise ValueError("white_baselines: %d dicts for %d datasets" % (len(dicts), len(sets)))
    return [_white_baseline(i, d, s) for i, (d, s) in enumerate(zip(dicts, sets))]


RED_BASELINE_KEYS = ("red_baseline", "red_baseline_sigma")


class OuBaselineSystem(NamedTuple):
    """the noise tables of a dataset and the linear system of its baseline columns under that noise (ou_baseline_system)"""
    alpha: np.ndarray         # [T] of ou_system
    beta: np.ndarray          # [T]
    omega: np.ndarray         # [T]
    c: np.ndarray             # [K][T] c_k[n] = omega_n z[B_k]_n / sqrt(D_k), z[x] the innovations of x
    D: np.ndarray             # [K] D_k = sum_n omega_n z[B_k]_n^2 = B_k^T K^-1 B_k
    A: np.ndarray             # [K][K] A~ = D^(-1/2) (B^T K^-1 B + diag(1 / s_k^2)) D^(-1/2)
    M: np.ndarray             # [K][K] A~^(-1), symmetric; None where A~ is singular
    lambda_min: float         # smallest eigenvalue of A~

    @property
    def minv(self):
        """M's upper triangle packed by rows: the `minv` of trxg_chi2_grid_ou_baseline"""
        return np.ascontiguousarray(self.M[np.triu_indices(self.M.shape[0])])


def ou_baseline_system(dataset, B, sigmas):
    """OuBaselineSystem of the columns B [K][T] with prior sigmas [K] (inf: flat) under the noise of a Dataset with
    red_sigma / red_timescale -- the one place that forms them, for the device path (fused._Dataset) and for the numpy
    statement (_numerics.ou_baseline_halfchi2).  The Kalman recurrence of ou_system whitens the columns as it whitens the
    residuals: with z[x]_n = x_n - g_n (_numerics.ou_innovations), B_k^T K^-1 B_l = sum_n omega_n z[B_k]_n z[B_l]_n, so the
    scaled system is linear_system's on the weights omega and the columns z[B_k].  ValueError for a column whose D_k is 0
    (or not finite); a singular A~ gives lambda_min <= 0 and M = None."""
    from ._numerics import ou_innovations
    alpha, beta, omega = ou_system(dataset)
    Z = ou_innovations(np.atleast_2d(np.asarray(B, dtype=np.float64)), alpha, beta, np.float64)
    system = linear_system(omega, Z, sigmas)
    return OuBaselineSystem(alpha, beta, omega, system.g, system.D, system.A, system.M, system.lambda_min)


def _red_baseline(i, d, dataset):
    """a dataset's "red_baseline" and "red_baseline_sigma" -> ([K_b][T kept] columns, [K_b] sigmas), or None; dataset: the
    validated Dataset of the same dict (its noise, and what else it marginalises)"""
    value, sigma = d.get("red_baseline"), d.get("red_baseline_sigma")
    time = np.atleast_1d(np.asarray(d["time"], dtype=np.float64))
    keep = ~np.isnan(time) & ~np.isnan(np.atleast_1d(np.asarray(d["flux"], dtype=np.float64)))
    B, s = _baseline(i, value, sigma, time.size, keep, name="red_baseline")
    if B is None:
        return None
    if B.shape[0] > MAX_BASELINE_TERMS:
        raise ValueError("dataset %d: at most %d red_baseline columns (got %d)" % (i, MAX_BASELINE_TERMS, B.shape[0]))
    if (dataset.offset_sigma is not None or dataset.baseline is not None or dataset.red_grid is not None
            or d.get("outlier_frac") is not None or d.get("outlier_scale") is not None):
        raise ValueError("dataset %d: red_baseline together with offset_sigma, baseline, red_grid or outlier_frac / "
                         "outlier_scale is not built: the columns stand next to red_sigma / red_timescale (and t0_grid) "
                         "alone; a column of ones is the constant" % i)
    if dataset.red_sigma is None:
        raise ValueError("dataset %d: red_baseline needs red_sigma / red_timescale: under white noise give the columns as "
                         "baseline" % i)
    try:
        system = ou_baseline_system(dataset, B, s)
    except ValueError as e:
        raise ValueError("dataset %d: red_baseline term %s" % (i, e)) from None
    if not system.lambda_min >= MIN_BASELINE_EIGENVALUE:
        raise ValueError("dataset %d: the red_baseline terms are collinear under the dataset's noise (smallest eigenvalue of "
                         "the scaled system %.3g < %g): drop a column, or give finite priors"
                         % (i, system.lambda_min, MIN_BASELINE_EIGENVALUE))
    return B, s


def red_baselines(dicts, sets):
    """The "red_baseline" / "red_baseline_sigma" keys of the dicts that validate() turned into `sets`: per dataset None, or
    the pair (B, sigmas) -- B a contiguous float64 [K_b][kept points] array of K_b = 1 ... MAX_BASELINE_TERMS columns of a
    linear baseline model sum_k c_k B_k[t], aligned with `time` (entries of NaN-dropped points dropped with them, every
    kept entry finite), sigmas [K_b] the prior sigmas of c_k ~ N(0, s_k^2), each > 0 or inf (absent: flat) -- marginalised
    per draw under the dataset's correlated noise: its term of the log-weight becomes 0.5 [y^T K^-1 y - b^T A^-1 b]
    (_numerics.ou_baseline_halfchi2 on ou_baseline_system).  A column of ones is how the constant is given.  The keys stand
    only next to red_sigma / red_timescale, and may stand next to t0_grid (the columns follow the points); ValueError next
    to offset_sigma, baseline, red_grid or outlier_frac / outlier_scale, without the two red keys, for a sigma without
    columns, a wrong shape, more than MAX_BASELINE_TERMS columns, a kept entry that is not finite, a zero column, or
    columns that are collinear under the noise (smallest eigenvalue of the scaled system < MIN_BASELINE_EIGENVALUE).
    Dataset itself has no field for the keys: the pairs travel in Datasets.red_baselines."""
    if len(dicts) != len(sets):
        raise ValueError("red_baselines: %d dicts for %d datasets" % (len(dicts), len(sets)))
    return [_red_baseline(i, d, s) for i, (d, s) in enumerate(zip(dicts, sets))]


RED_KERNEL_BASELINE_KEYS = ("red_kernel_baseline", "red_kernel_baseline_sigma")


class Ss2BaselineSystem(NamedTuple):
    """the noise tables of a dataset with red_kernel "matern32" or "ou2" and the linear system of its baseline columns
    under that noise (ss2_baseline_system)"""
    A: np.ndarray             # [T][2][2] of ss2_system
    g: np.ndarray             # [T][2]
    omega: np.ndarray         # [T]
    c: np.ndarray             # [K][T] c_k[n] = omega_n z[B_k]_n / sqrt(D_k), z[x] the innovations of x
    D: np.ndarray             # [K] D_k = sum_n omega_n z[B_k]_n^2 = B_k^T K^-1 B_k
    Atilde: np.ndarray        # [K][K] A~ = D^(-1/2) (B^T K^-1 B + diag(1 / s_k^2)) D^(-1/2)
    M: np.ndarray             # [K][K] A~^(-1), symmetric; None where A~ is singular
    lambda_min: float         # smallest eigenvalue of A~

    @property
    def minv(self):
        """M's upper triangle packed by rows: the `minv` of trxk_chi2_grid_ss2_baseline"""
        return np.ascontiguousarray(self.M[np.triu_indices(self.M.shape[0])])


def ss2_baseline_system(dataset, B, sigmas):
    """Ss2BaselineSystem of the columns B [K][T] with prior sigmas [K] (inf: flat) under the noise of a Dataset with
    red_kernel "matern32" or "ou2" -- the one place that forms them, for the device path (fused._Dataset) and for the numpy
    statement (_numerics.ss2_baseline_halfchi2).  The two-state filter of ss2_system whitens the columns exactly as the
    recurrence of ou_system does: with z[x]_n = x_n - u_(n-1)[0] (_numerics.ss2_innovations), which is linear in x,
    B_k^T K^-1 B_l = sum_n omega_n z[B_k]_n z[B_l]_n, so the scaled system is linear_system's on the weights omega and the
    columns z[B_k].  ValueError for a column whose D_k is 0 (or not finite); a singular A~ gives lambda_min <= 0 and
    M = None."""
    from ._numerics import ss2_innovations
    A, g, omega = ss2_system(dataset)
    Z = ss2_innovations(np.atleast_2d(np.asarray(B, dtype=np.float64)), A, g, np.float64)
    system = linear_system(omega, Z, sigmas)
    return Ss2BaselineSystem(A, g, omega, system.g, system.D, system.A, system.M, system.lambda_min)


def _red_kernel_baseline(i, d, dataset):
    """a dataset's "red_kernel_baseline" and "red_kernel_baseline_sigma" -> ([K_b][T kept] columns, [K_b] sigmas), or None;
    dataset: the validated Dataset of the same dict (its noise, and what else it marginalises)"""
    value, sigma = d.get("red_kernel_baseline"), d.get("red_kernel_baseline_sigma")
    if isinstance(value, (bool, np.bool_, str, bytes)):
        raise ValueError("dataset %d: red_kernel_baseline must be an array [K][len(time)] or [len(time)] (got %r)"
                         % (i, value))
    time = np.atleast_1d(np.asarray(d["time"], dtype=np.float64))
    keep = ~np.isnan(time) & ~np.isnan(np.atleast_1d(np.asarray(d["flux"], dtype=np.float64)))
    B, s = _baseline(i, value, sigma, time.size, keep, name="red_kernel_baseline")
    if B is None:
        return None
    if B.shape[0] > MAX_BASELINE_TERMS:
        raise ValueError("dataset %d: at most %d red_kernel_baseline columns (got %d)" % (i, MAX_BASELINE_TERMS, B.shape[0]))
    others = [k for k in ("offset_sigma", "baseline", "baseline_sigma", "red_baseline", "red_baseline_sigma", "red_grid",
                          "white_grid") + WHITE_BASELINE_KEYS + OUTLIER_KEYS if d.get(k) is not None]
    if others:
        raise ValueError("dataset %d: red_kernel_baseline together with %s is not built: the columns stand next to "
                         "red_kernel = 'matern32' or 'ou2' with its red_sigma / red_timescale (and t0_grid) alone; a column "
                         "of ones is the constant" % (i, ", ".join(others)))
    if dataset.red_kernel not in RED_KERNELS:
        raise ValueError("dataset %d: red_kernel_baseline needs red_kernel = 'matern32' or 'ou2': under the one exponential "
                         "term give the columns as red_baseline, under white noise as baseline" % i)
    try:
        system = ss2_baseline_system(dataset, B, s)
    except ValueError as e:
        raise ValueError("dataset %d: red_kernel_baseline term %s" % (i, e)) from None
    if not system.lambda_min >= MIN_BASELINE_EIGENVALUE:
        raise ValueError("dataset %d: the red_kernel_baseline terms are collinear under the dataset's noise (smallest "
                         "eigenvalue of the scaled system %.3g < %g): drop a column, or give finite priors"
                         % (i, system.lambda_min, MIN_BASELINE_EIGENVALUE))
    return B, s


def red_kernel_baselines(dicts, sets):
    """The "red_kernel_baseline" / "red_kernel_baseline_sigma" keys of the dicts that validate() turned into `sets`: per
    dataset None, or the pair (B, sigmas) -- B a contiguous float64 [K_b][kept points] array of K_b = 1 ...
    MAX_BASELINE_TERMS columns of a linear baseline model sum_k c_k B_k[t], aligned with `time` (entries of NaN-dropped
    points dropped with them, every kept entry finite), sigmas [K_b] the prior sigmas of c_k ~ N(0, s_k^2), each > 0 or inf
    (absent: flat) -- marginalised per draw under the dataset's Matern-3/2 or two-term noise: its term of the log-weight
    becomes 0.5 [y^T K^-1 y - b^T A^-1 b] (_numerics.ss2_baseline_halfchi2 on ss2_baseline_system).  A column of ones is
    how the constant is given.  The keys stand only next to red_kernel = "matern32" or "ou2", and may stand next to t0_grid
    (the columns follow the points); ValueError next to offset_sigma, baseline, red_baseline, red_grid, white_grid or
    outlier_frac / outlier_scale, without such a red_kernel, for a sigma without columns, a wrong shape, more than
    MAX_BASELINE_TERMS columns, a kept entry that is not finite, a zero column, a bool or a string, or columns that are
    collinear under the noise (smallest eigenvalue of the scaled system < MIN_BASELINE_EIGENVALUE).  Dataset itself has no
    field for the keys: the pairs travel in Datasets.red_kernel_baselines."""
    if len(dicts) != len(sets):
        raise ValueError("red_kernel_baselines: %d dicts for %d datasets" % (len(dicts), len(sets)))
    return [_red_kernel_baseline(i, d, s) for i, (d, s) in enumerate(zip(dicts, sets))]


def robust_constants(frac, scale):
    """(c0, c1, k2) of a dataset's outlier mixture: c0 = -log1p(-eps) >= 0, c1 = ln kappa - ln eps > 0, k2 = 1 / kappa^2 --
    the one place that forms them, for the device path (fused._Dataset) and for the numpy statement
    (_numerics.robust_halfchi2).  Pure numbers: the same in every star's normalisation."""
    frac, scale = float(frac), float(scale)
    return -math.log1p(-frac), math.log(scale) - math.log(frac), 1.0 / (scale * scale)


def ou_system(dataset):
    """(alpha, beta, omega), float64 [T] each: the Kalman form of a Dataset's noise covariance
    K = diag(flux_err^2) + red_sigma^2 exp(-|t_i - t_j| / red_timescale), stamps in time order -- the one place that forms
    them, for the device path (fused._Dataset) and for the numpy statement (_numerics.ou_halfchi2).  With P_0 = s_r^2 and
    phi_n = exp(-(t_n - t_(n-1)) / tau):
        D_n = P_n + sigma_n^2,  kappa_n = P_n / D_n,  omega_n = 1 / D_n,
        alpha_n = phi_n (1 - kappa_(n-1)),  beta_n = phi_n kappa_(n-1)   (alpha_0 = beta_0 = 0),
        P_n = phi_n^2 (1 - kappa_(n-1)) P_(n-1) + s_r^2 (1 - phi_n^2)    (1 - phi^2 as -expm1(-2 dt / tau)),
    so that 0.5 y^T K^-1 y = 0.5 sum_n omega_n (y_n - g_n)^2, g_0 = 0, g_n = alpha_n g_(n-1) + beta_n y_(n-1)."""
    t, var = dataset.time, dataset.flux_err * dataset.flux_err
    s2, tau = float(dataset.red_sigma) ** 2, float(dataset.red_timescale)
    T = t.size
    alpha, beta, omega = np.zeros(T), np.zeros(T), np.zeros(T)
    P, kappa = s2, 0.0
    for n in range(T):
        if n > 0:
            dt = float(t[n] - t[n - 1])
            phi = math.exp(-dt / tau)
            alpha[n] = phi * (1.0 - kappa)
            beta[n] = phi * kappa
            P = phi * phi * (1.0 - kappa) * P + s2 * -math.expm1(-2.0 * dt / tau)
        D = P + float(var[n])
        kappa = P / D
        omega[n] = 1.0 / D
    return alpha, beta, omega


def ss2_system(dataset):
    """(A [T][2][2], g [T][2], omega [T]), float64: the Kalman form of the noise covariance of a Dataset with red_kernel =
    "matern32" or "ou2", K = diag(flux_err^2) + k(|t_i - t_j|), stamps in time order -- the one place that forms them, for the
    device path (fused._Dataset) and for the numpy statement (_numerics.ss2_halfchi2).  The process has a state of dimension
    two, written in a basis whose first component is what is observed, with the stationary covariance Pinf and the
    transition Phi(dt):
        matern32, k = s^2 (1 + lam dt) exp(-lam dt), lam = sqrt(3) / l, state (x, x' / lam):
            Pinf = s^2 I,   Phi = exp(-lam dt) [[1 + lam dt, lam dt], [-lam dt, 1 - lam dt]];
        ou2, k = s_1^2 exp(-dt / tau_1) + s_2^2 exp(-dt / tau_2), state (x_1 + x_2, x_2), a_i = exp(-dt / tau_i):
            Pinf = [[s_1^2 + s_2^2, s_2^2], [s_2^2, s_2^2]],   Phi = [[a_1, a_2 - a_1], [0, a_2]].
    The covariance recursion with the observation vector e_0 = (1, 0), from P_0 = Pinf:
        S_n = P_n[0][0] + sigma_n^2,  k_n = P_n[:, 0] / S_n,  omega_n = 1 / S_n,  P_n+ = P_n - S_n k_n k_n^T,
        P_(n+1) = Phi P_n+ Phi^T + Q,  Q = Pinf - Phi Pinf Phi^T,  Phi = Phi(t_(n+1) - t_n),
        A_n = Phi (I - k_n e_0^T),  g_n = Phi k_n     (both zero for the last stamp),
    so that 0.5 y^T K^-1 y = 0.5 sum_n omega_n z_n^2, z_n = y_n - u_(n-1)[0], u_(-1) = 0, u_n = A_n u_(n-1) + g_n y_n, and
    ln det K = sum_n ln S_n.  Q is formed without the subtraction of near-equal matrices where a closed form allows it:
    for ou2 from 1 - a_i^2 = -expm1(-2 dt / tau_i), as ou_system forms it."""
    kernel = dataset.red_kernel
    if kernel not in RED_KERNELS:
        raise ValueError("ss2_system: a dataset with red_kernel 'matern32' or 'ou2' (got %r)" % (kernel,))
    t, var = dataset.time, dataset.flux_err * dataset.flux_err
    T = t.size
    if kernel == "matern32":
        s2, lam = float(dataset.red_sigma) ** 2, math.sqrt(3.0) / float(dataset.red_timescale)
        p00, p01, p11 = s2, 0.0, s2

        def step(dt):
            x = lam * dt
            e = math.exp(-x)
            if e == 0.0:                                          # (also x = inf: no 0 * inf below)
                return (0.0, 0.0, 0.0, 0.0), (s2, 0.0, s2)
            e2 = math.exp(-2.0 * x)
            # Q = s^2 (I - Phi Phi^T), Phi Phi^T = exp(-2 x) [[1 + 2 x + 2 x^2, -2 x^2], [-2 x^2, 1 - 2 x + 2 x^2]]
            q00 = s2 * (-math.expm1(-2.0 * x) - e2 * (2.0 * x + 2.0 * x * x))
            q01 = s2 * (e2 * 2.0 * x * x)
            q11 = s2 * (-math.expm1(-2.0 * x) - e2 * (2.0 * x * x - 2.0 * x))
            return (e * (1.0 + x), e * x, -(e * x), e * (1.0 - x)), (q00, q01, q11)
    else:
        s1, s2_ = (float(v) ** 2 for v in dataset.red_sigma)
        tau1, tau2 = (float(v) for v in dataset.red_timescale)
        p00, p01, p11 = s1 + s2_, s2_, s2_

        def step(dt):
            a1, a2 = math.exp(-dt / tau1), math.exp(-dt / tau2)
            q1, q2 = s1 * -math.expm1(-2.0 * dt / tau1), s2_ * -math.expm1(-2.0 * dt / tau2)
            return (a1, a2 - a1, 0.0, a2), (q1 + q2, q2, q2)
    A, g, omega = np.zeros((T, 2, 2)), np.zeros((T, 2)), np.zeros(T)
    for n in range(T):
        S = p00 + float(var[n])
        k0, k1 = p00 / S, p01 / S
        omega[n] = 1.0 / S
        if n == T - 1:
            break
        (f00, f01, f10, f11), (q00, q01, q11) = step(float(t[n + 1] - t[n]))
        A[n] = ((f00 * (1.0 - k0) - f01 * k1, f01), (f10 * (1.0 - k0) - f11 * k1, f11))
        g[n] = (f00 * k0 + f01 * k1, f10 * k0 + f11 * k1)
        # P+ = P - S k k^T, then Phi P+ Phi^T + Q
        u00, u01, u11 = (1.0 - k0) * p00, (1.0 - k0) * p01, p11 - p01 * k1
        m00, m01 = f00 * u00 + f01 * u01, f00 * u01 + f01 * u11
        m10, m11 = f10 * u00 + f11 * u01, f10 * u01 + f11 * u11
        p00 = m00 * f00 + m01 * f01 + q00
        p01 = m00 * f10 + m01 * f11 + q01
        p11 = m10 * f10 + m11 * f11 + q11
    return A, g, omega


def ou_mix_system(dataset):
    """(alpha [J][T], beta [J][T], omega [J][T], lnc [J]), float64: ou_system of every candidate (s_j, tau_j, pi_j) of a
    Dataset's red_grid, and the candidates' log-weights
        lnc_j = ln pi_j + 0.5 sum_n ln omega_j[n] - logsumexp_j(the same),     ln det K_j = -sum_n ln omega_j[n],
    so that sum_j exp(lnc_j) = 1 and the dataset's term of the log-weight is -ln sum_j exp(lnc_j - h_j), h_j = 0.5 y^T K_j^-1 y
    (_numerics.ou_mix_halfchi2, trxm_chi2_grid_ou_mix).  The sums are math.fsum's; the normaliser that is dropped,
    sum_j pi_j |K_j|^(-1/2), depends on the dataset alone."""
    grid = dataset.red_grid
    tables, raw = [], []
    for s_r, tau, weight in grid:
        abw = ou_system(dataset._replace(red_grid=None, red_sigma=float(s_r), red_timescale=float(tau)))
        tables.append(abw)
        raw.append(math.log(weight) + 0.5 * math.fsum(np.log(abw[2]).tolist()))
    # (the raw values are large -- half a log-determinant --, their differences are not: normalise the differences)
    top = max(raw)
    diff = [v - top for v in raw]
    norm = math.log(math.fsum(math.exp(v) for v in diff))
    lnc = np.array([v - norm for v in diff])
    alpha, beta, omega = (np.ascontiguousarray(np.stack([t[k] for t in tables])) for k in range(3))
    return alpha, beta, omega, lnc


def _check_baseline(i, dataset):
    """the limits of a dataset's baseline terms: their number and the conditioning of the scaled system"""
    n_terms = (dataset.offset_sigma is not None) + (0 if dataset.baseline is None else dataset.baseline.shape[0])
    if dataset.baseline is None:
        return
    if n_terms > MAX_BASELINE_TERMS:
        raise ValueError("dataset %d: at most %d baseline terms, offset_sigma included (got %d)"
                         % (i, MAX_BASELINE_TERMS, n_terms))
    try:
        system = baseline_system(dataset)
    except ValueError as e:
        raise ValueError("dataset %d: baseline term %s" % (i, e)) from None
    if not system.lambda_min >= MIN_BASELINE_EIGENVALUE:
        raise ValueError("dataset %d: the baseline terms are collinear (smallest eigenvalue of the scaled system %.3g < %g):"
                         " drop a column, or a constant column next to offset_sigma, or give finite priors"
                         % (i, system.lambda_min, MIN_BASELINE_EIGENVALUE))


def validate(datasets):
    """A list of 1 ... MAX_DATASETS dicts {time, flux, flux_err[, exptime, nsamples, offset_sigma, baseline,
    baseline_sigma, red_sigma, red_timescale, red_kernel, red_grid, t0_grid, outlier_frac, outlier_scale, red_baseline,
    red_baseline_sigma, white_grid, white_baseline, white_baseline_sigma, red_kernel_baseline, red_kernel_baseline_sigma]} -> a list of Dataset ("red_kernel" = "matern32" / "ou2" gives a Matern32Dataset / an Ou2Dataset: the
    same fields, red_sigma and red_timescale two finite numbers / two arrays of two finite entries, all > 0; "t0_grid"
    is allowed here and read by t0_grids, "outlier_frac" / "outlier_scale" are checked here and returned by outliers,
    "red_baseline" / "red_baseline_sigma" are checked here and returned by red_baselines, "white_grid" is checked here and
    returned by white_grids: no field of Dataset holds them).  Points with a NaN time or flux are dropped together with their error and their
    baseline entries; a scalar flux_err is broadcast.  ValueError for an empty list, too many datasets, mismatched
    lengths, an error that is not finite or not positive, a dataset without points, an offset_sigma that is not None, a
    number > 0 or inf, a baseline that is not [K][len(time)] and finite at the kept points, a baseline_sigma that is not
    > 0 or inf per column (or has no baseline), more than MAX_BASELINE_TERMS terms, or collinear terms; for red_sigma
    without red_timescale or the reverse, a red_sigma that is not a finite number > 0, a red_timescale that is not > 0 or
    inf, either of them next to offset_sigma or baseline, or with kept stamps that are not in non-decreasing order; for a
    red_grid that is not 1 ... MAX_RED_CANDIDATES triples (s_r finite > 0, tau > 0 or inf, weight finite > 0; the weights are
    normalised to sum 1, repeated pairs are allowed), that stands next to red_sigma / red_timescale, offset_sigma or
    baseline, or whose kept stamps are not in non-decreasing order; for outlier_frac without outlier_scale or the reverse, an
    outlier_frac outside (0, 0.5], an outlier_scale that is not a finite number > 1, or either of them next to
    offset_sigma, baseline, red_sigma / red_timescale or red_grid; for a red_kernel that is not None, "ou", "matern32" or
    "ou2", and with the last two for a red_sigma or red_timescale of the wrong shape or with an entry that is not finite and
    > 0, for stamps out of order, or for offset_sigma, baseline, red_grid, red_baseline or the outlier keys next to them; and
    for what red_baselines, white_grids, white_baselines and red_kernel_baselines list ("red_kernel_baseline" /
    "red_kernel_baseline_sigma" are checked here and returned by red_kernel_baselines)."""
    if isinstance(datasets, dict) or not hasattr(datasets, "__len__"):
        raise ValueError("datasets must be a list of dicts with the keys time, flux, flux_err")
    if len(datasets) == 0:
        raise ValueError("datasets is empty: give at least one light curve")
    if len(datasets) > MAX_DATASETS:
        raise ValueError("at most %d datasets (got %d)" % (MAX_DATASETS, len(datasets)))
    out = []
    for i, d in enumerate(datasets):
        unknown = set(d) - {"time", "flux", "flux_err", "exptime", "nsamples", "offset_sigma", "baseline", "baseline_sigma",
                            "red_sigma", "red_timescale", "red_grid", "t0_grid", "outlier_frac", "outlier_scale",
                            "red_baseline", "red_baseline_sigma", "red_kernel", "white_grid"} - set(WHITE_BASELINE_KEYS) \
            - set(RED_KERNEL_BASELINE_KEYS)
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
        n_given = time.size
        time, flux, err = time[keep], flux[keep], err[keep]
        if time.size == 0:
            raise ValueError("dataset %d has no points left after dropping NaN" % i)
        if not np.all(np.isfinite(err) & (err > 0)):
            raise ValueError("dataset %d: every flux_err must be finite and > 0" % i)
        nsamples = int(d.get("nsamples", DEFAULT_NSAMPLES))
        if nsamples < 1:
            raise ValueError("dataset %d: nsamples must be >= 1" % i)
        baseline, baseline_sigma = _baseline(i, d.get("baseline"), d.get("baseline_sigma"), n_given, keep)
        offset_sigma = _offset_sigma(i, d.get("offset_sigma"))
        red_kernel = _red_kernel(i, d.get("red_kernel"))
        if red_kernel is None:
            red_sigma, red_timescale = _red_noise(i, d.get("red_sigma"), d.get("red_timescale"), time,
                                                  offset_sigma is not None or baseline is not None)
        else:
            others = [k for k in ("offset_sigma", "baseline", "red_grid", "red_baseline", "red_baseline_sigma") + OUTLIER_KEYS
                      if d.get(k) is not None]
            red_sigma, red_timescale = _red_terms(i, red_kernel, d.get("red_sigma"), d.get("red_timescale"), time, others)
        red_grid = _red_grid(i, d.get("red_grid"), time,
                             offset_sigma is not None or baseline is not None or red_sigma is not None)
        record = Dataset if red_kernel is None else RED_KERNELS[red_kernel]
        out.append(record(np.ascontiguousarray(time), np.ascontiguousarray(flux), np.ascontiguousarray(err),
                          float(d.get("exptime", DEFAULT_EXPTIME)), nsamples,
                          offset_sigma, baseline, baseline_sigma, red_grid, red_sigma, red_timescale))
        _check_baseline(i, out[-1])
        _red_baseline(i, d, out[-1])
        _red_kernel_baseline(i, d, out[-1])
        _outliers(i, d, out[-1])
        _white_grid(i, d)
        _white_baseline(i, d, out[-1])
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
    """validated datasets in one star's normalisation, their sigma_bar, and per dataset None or its transit-time shift
    grid (t0_grids), None or its outlier pair (frac, scale) (outliers), None or the pair (columns, sigmas) of its
    baseline under correlated noise (red_baselines), None or its grid of white-noise candidates (white_grids) and None or
    the pair (columns, sigmas) of its baseline under those candidates (white_baselines), and None or the pair (columns,
    sigmas) of its baseline under Matern-3/2 or two-term noise (red_kernel_baselines: a keyword)"""

    def __init__(self, sets, t0_grids=None, outliers=None, red_baselines=None, white_grids=None, red_kernel_baselines=None,
                 white_baselines=None):
        self.sets = tuple(sets)
        self.sigma_ref = sigma_ref(self.sets)
        for name, what, seq in (("t0_grids", "grids", t0_grids), ("outliers", "pairs", outliers),
                                ("red_baselines", "pairs", red_baselines), ("white_grids", "grids", white_grids),
                                ("white_baselines", "pairs", white_baselines),
                                ("red_kernel_baselines", "pairs", red_kernel_baselines)):
            seq = (None,) * len(self.sets) if seq is None else tuple(seq)
            if len(seq) != len(self.sets):
                raise ValueError("%s: %d %s for %d datasets" % (name, len(seq), what, len(self.sets)))
            setattr(self, name, seq)

    def __len__(self):
        return len(self.sets)

    @property
    def has_offsets(self):
        return any(s.offset_sigma is not None for s in self.sets)

    @property
    def has_baselines(self):
        return any(s.baseline is not None for s in self.sets)

    @property
    def has_red_noise(self):
        return any(s.red_sigma is not None or s.red_grid is not None for s in self.sets)

    @property
    def has_t0_grids(self):
        return any(g is not None for g in self.t0_grids)

    @property
    def has_outliers(self):
        return any(o is not None for o in self.outliers)

    @property
    def has_red_baselines(self):
        return any(b is not None for b in self.red_baselines)

    @property
    def has_white_grids(self):
        return any(g is not None for g in self.white_grids)

    @property
    def has_white_baselines(self):
        return any(b is not None for b in self.white_baselines)

    @property
    def has_red_kernel_baselines(self):
        return any(b is not None for b in self.red_kernel_baselines)

    @property
    def size(self):
        """points of all datasets together"""
        return sum(s.time.size for s in self.sets)

    def renorm(self, star_fluxratio):
        """funcs.renorm_flux on every dataset, elementwise on flux and flux_err; sigma_bar is taken afterwards.  A finite
        offset_sigma is an error in flux units and is divided by the flux ratio as the errors are: s^2 sum(1 / err^2) --
        and with it the factor of the marginal that the evidence drops -- is the same for every
        star.  So is every finite baseline_sigma (flux units per unit of its column); the columns are left alone: the scaled
        system matrix of baseline_system is then the same for every star.  A red_sigma is in flux units too and is divided
        the same way: alpha and beta of ou_system do not change, omega scales with the square of the flux ratio, and the
        determinant ratio that the evidence drops is the same for every star.  The s_r column of a red_grid is divided
        likewise: every candidate's determinant gains the same factor, so the lnc of ou_mix_system do not change.  The t0_grids are times and
        pure weights: carried through as they are.  So are the outlier pairs: only z_t = d_t / sigma_t enters the mixture,
        and renorm_flux leaves it alone.  A finite sigma of a red_baselines pair is in flux units per unit of its column
        and is divided by the flux ratio; the columns are left alone: with red_sigma and the errors scaled alike, D_k of
        ou_baseline_system scales with the square of the flux ratio, s_k^2 D_k and the scaled system matrix are the same
        for every star, and so is the determinant that the evidence drops.  The jitter column of a white_grids grid is in
        flux units and is divided by the flux ratio, the scales are pure numbers: every candidate's weights gain the
        square of the flux ratio, so the lnc of white_mix_system do not change.  A finite sigma of a white_baselines pair is
        divided by the flux ratio as a red_baselines pair's is: every A_j of white_baseline_system gains the square of the
        flux ratio, det A_j its K-th power for every candidate alike, and the lnc do not change.  A finite sigma of a
        red_kernel_baselines pair is divided by the flux ratio as well: A and g of ss2_system do not change, omega and D_k of
        ss2_baseline_system scale with the square of the flux ratio, so s_k^2 D_k, the scaled system matrix and the
        determinant that the evidence drops are the same for every star."""
        out = []
        for s in self.sets:
            flux, err = renorm_flux(s.flux, s.flux_err, star_fluxratio)
            off = s.offset_sigma
            if off is not None and math.isfinite(off):
                off = off / star_fluxratio
            bsig = s.baseline_sigma
            if bsig is not None:
                bsig = np.where(np.isfinite(bsig), bsig / star_fluxratio, bsig)
            red = s.red_sigma
            if red is not None:
                red = red / star_fluxratio
            grid = s.red_grid
            if grid is not None:
                grid = grid.copy()
                grid[:, 0] = grid[:, 0] / star_fluxratio
            out.append(s._replace(flux=np.ascontiguousarray(flux), flux_err=np.ascontiguousarray(err), offset_sigma=off,
                                  baseline_sigma=bsig, red_sigma=red, red_grid=grid))

        def pairs(seq):
            """the finite sigmas of (columns, sigmas) pairs divided by the flux ratio"""
            return [None if p is None else (p[0], np.where(np.isfinite(p[1]), p[1] / star_fluxratio, p[1])) for p in seq]
        white = []
        for g in self.white_grids:
            if g is not None:
                g = g.copy()
                g[:, 1] = g[:, 1] / star_fluxratio
            white.append(g)
        return Datasets(out, self.t0_grids, self.outliers, pairs(self.red_baselines), white,
                        white_baselines=pairs(self.white_baselines), red_kernel_baselines=pairs(self.red_kernel_baselines))
