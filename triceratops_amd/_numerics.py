"""Numerically stable reductions used by the marginal likelihoods.

Same call surface as the reference's triceratops/_numerics.py:
  _log_mean_exp(logw, *, N_total)   (_numerics.py:12-51)  -> HIP kernel trx_log_mean_exp
  _normalize_probabilities(lnZ)     (_numerics.py:54-76)  -> host arithmetic over the 18-75
                                                             scenario evidences
"""
import math

import numpy as np
import torch

from . import _lib


def _log_mean_exp(logw, *, N_total: int) -> float:
    """log(mean(exp(logw))) over N_total draws, evaluated on the GPU.

    -inf and NaN entries carry zero weight but count in the denominator; any +inf gives +inf;
    no finite entry gives -inf; N_total must equal len(logw) (ValueError otherwise, exactly like
    the reference guard at _numerics.py:40-45).  `logw` may be a numpy array or a CUDA tensor.
    """
    size = logw.numel() if isinstance(logw, torch.Tensor) else np.size(logw)
    if N_total != size:
        raise ValueError(
            f"N_total ({N_total}) must equal len(logw) ({size}). "
            "Passing len(lnL[finite]) instead of len(lnL) would silently "
            "overestimate evidence for scenarios with geometric exclusions."
        )
    d = _lib.dev(logw).reshape(-1)
    return float(_lib.log_mean_exp(d, N_total).cpu()[0])


def _normalize_probabilities(lnZ):
    """Scenario probabilities exp(lnZ - logsumexp(lnZ)) and a status string:
    'ok', 'all_neginf' (every evidence is -inf) or 'anomaly' (a NaN or +inf is present);
    the two degenerate cases return all-zero probabilities."""
    lnZ = np.asarray(lnZ, dtype=np.float64)
    if np.any(np.isnan(lnZ)) or np.any(np.isposinf(lnZ)):
        return np.zeros(len(lnZ)), 'anomaly'
    if np.all(np.isneginf(lnZ)):
        return np.zeros(len(lnZ)), 'all_neginf'
    top = np.max(lnZ)
    with np.errstate(divide="ignore"):
        lse = np.log(np.sum(np.exp(lnZ - top))) + top
    return np.exp(lnZ - lse), 'ok'


# rows of the scenario table whose evidences make up 1 - FPP (TP, PTP, DTP: triceratops.py:1483) and the first row of
# the nearby stars' scenarios (NFPP, :1484)
_FPP_ROWS = (0, 3, 9)
_NFPP_FIRST = 15


def _mc_errors(lnZ, lnM2, N, status):
    """Monte-Carlo standard errors of a calc_probs table from the moments of its evidences.

    lnZ, lnM2 [n_scen]: log mean weight and log mean squared weight of each scenario's N draws (lnM2 NaN = unknown);
    N: draws per scenario; status: _normalize_probabilities' status of lnZ.  Returns a dict of
      ess       (sum w)^2 / sum w^2 = N exp(2 lnZ - lnM2) per row; 0 where lnZ = -inf
      lnZ_err   sqrt(1 / ess - 1 / N) per row (the delta method's standard error of log(mean w)); NaN where lnZ is
                not finite
      FPP_err, NFPP_err   the delta method through FPP = B / (A + B) (A = the TP, PTP and DTP evidences, B = the rest)
                and NFPP = C / (C + D) (C = the nearby stars' rows), the evidences taken as independent: the two branches
                of one binary call share draws with disjoint masks (covariance -Z1 Z2 / N, a relative -1/N), left out.
                NaN when the status is not 'ok' or a contributing row's error is unknown.
    """
    lnZ = np.asarray(lnZ, dtype=np.float64)
    lnM2 = np.asarray(lnM2, dtype=np.float64)
    N = np.asarray(N, dtype=np.float64)
    fin = np.isfinite(lnZ)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        ess = np.where(fin, N * np.exp(2.0 * lnZ - lnM2), np.where(lnZ == -np.inf, 0.0, np.nan))
        lnZ_err = np.where(fin, np.sqrt(np.maximum(1.0 / ess - 1.0 / N, 0.0)), np.nan)
    out = {"ess": ess, "lnZ_err": lnZ_err, "FPP_err": np.nan, "NFPP_err": np.nan}
    if status != 'ok':
        return out
    # Z_i = exp(lnZ_i - max lnZ) (a common scale: the ratios do not see it), V_i = Z_i^2 lnZ_err_i^2 (0 where Z_i = 0)
    Z = np.exp(lnZ - lnZ.max())
    V = np.where(fin, Z * Z * lnZ_err * lnZ_err, 0.0)

    def ratio_err(in_a):
        # (both sides summed on their own: B = sum - A would lose B, and V_B go negative, when A holds nearly all)
        A, B, VA, VB = Z[in_a].sum(), Z[~in_a].sum(), V[in_a].sum(), V[~in_a].sum()
        return float(np.sqrt((A * A * VB + B * B * VA) / (A + B) ** 4))

    in_a = np.zeros(lnZ.shape, dtype=bool)
    in_a[[i for i in _FPP_ROWS if i < lnZ.size]] = True
    out["FPP_err"] = ratio_err(in_a)
    in_c = np.zeros(lnZ.shape, dtype=bool)
    in_c[_NFPP_FIRST:] = True
    out["NFPP_err"] = ratio_err(in_c)
    return out


# ---- adaptive importance map of the draw kernel's uniforms (trx_draw_args.warp) ----------------
WARP_DIMS, WARP_BINS = _lib.WARP_DIMS, _lib.WARP_BINS


def offset_halfchi2(resid, w, offset_sigma):
    """chi^2/2 of a light curve's residuals with a constant offset c ~ N(0, offset_sigma^2) marginalised (DESIGN.md
    section 14), float64 on the host: the statement of what trx_chi2_grid_offset computes per row.
        -ln int exp(-0.5 sum_t w_t (r_t - c)^2) N(c; 0, s^2) dc = h + 0.5 ln(1 + s^2 S0),
        h = 0.5 (S2 - S1^2 / (S0 + 1 / s^2)),   S0 = sum w, S1 = sum w r, S2 = sum w r^2.
    Returns h -- the factor (1 + s^2 S0)^(-1/2) depends on the dataset only and is dropped -- never below 0.
    resid: [..., T]; w: [T]; offset_sigma: > 0, inf for the flat prior (1 / s^2 = 0); None: no offset, 0.5 S2."""
    resid = np.asarray(resid, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    S2 = np.sum(w * resid * resid, axis=-1)
    if offset_sigma is None:
        return 0.5 * S2
    S0 = math.fsum(w.tolist())
    S1 = np.sum(w * resid, axis=-1)
    prec = 0.0 if math.isinf(offset_sigma) else 1.0 / (float(offset_sigma) * float(offset_sigma))
    return np.maximum(0.5 * (S2 - S1 * S1 / (S0 + prec)), 0.0)


def baseline_halfchi2(resid, w, basis, sigmas=None):
    """chi^2/2 of a light curve's residuals with a linear baseline sum_k c_k B_k[t], c_k ~ N(0, s_k^2) independent,
    marginalised, float64 on the host: the statement of what trx_chi2_grid_baseline computes per row.
        -ln int exp(-0.5 sum_t w_t (r_t - sum_k c_k B_k[t])^2) prod_k N(c_k; 0, s_k^2) dc
            = h + 0.5 ln det(I + diag(s^2) B^T W B),
        h = 0.5 (S2 - b^T A^-1 b),   S2 = sum w r^2,   b_k = sum w B_k r,   A = B^T W B + diag(1 / s_k^2),
    evaluated in the scaled form of datasets.linear_system (D_k = sum w B_k^2, A~ = D^(-1/2) A D^(-1/2), M = A~^-1,
    b~_k = b_k / sqrt(D_k)): h = 0.5 (S2 - b~^T M b~).  Returns h -- the determinant depends on the dataset only and is
    dropped -- never below 0.  resid: [..., T]; w: [T]; basis: [K][T] or [T], None: no baseline, 0.5 S2; sigmas: a number
    or [K], each > 0 or inf (flat: 1 / s^2 = 0), None: all flat.  ValueError for a zero column or a singular system."""
    from .datasets import linear_system
    resid = np.asarray(resid, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    S2 = np.sum(w * resid * resid, axis=-1)
    if basis is None:
        return 0.5 * S2
    system = linear_system(w, basis, np.inf if sigmas is None else sigmas)
    if system.M is None:
        raise ValueError("the baseline system is singular (smallest eigenvalue %g)" % system.lambda_min)
    b = resid @ system.g.T
    q = np.einsum("...i,ij,...j->...", b, system.M, b)
    return np.maximum(0.5 * (S2 - q), 0.0)


def ou_halfchi2(y, alpha, beta, omega, dtype=np.float64):
    """chi^2/2 of a light curve's residuals under white plus exponential (Ornstein-Uhlenbeck) noise (DESIGN.md section
    14), on the host: the statement of what trxn_chi2_grid_ou computes per row,
        g_0 = 0,  g_n = alpha_n g_(n-1) + beta_n y_(n-1),   h = 0.5 sum_n omega_n (y_n - g_n)^2 = 0.5 y^T K^-1 y,
    alpha, beta, omega [T] from datasets.ou_system; the determinant of K depends on the dataset only and is dropped.
    y: [..., T] residuals.  A sequential loop over T, vectorised over the rows, in `dtype` (np.longdouble: the tests'
    reference)."""
    y = np.asarray(y, dtype=dtype)
    alpha, beta, omega = (np.asarray(v, dtype=dtype) for v in (alpha, beta, omega))
    g = np.zeros(y.shape[:-1], dtype=dtype)
    h = np.zeros(y.shape[:-1], dtype=dtype)
    for n in range(y.shape[-1]):
        if n > 0:
            g = alpha[n] * g + beta[n] * y[..., n - 1]
        z = y[..., n] - g
        h = h + omega[n] * z * z
    return h * dtype(0.5)


def ss2_halfchi2(y, A, g, omega, dtype=np.float64):
    """chi^2/2 of a light curve's residuals under white noise plus a process with a two-dimensional state -- a Matern-3/2
    term, two exponential terms -- (DESIGN.md section 14), on the host: the statement of what trxs_chi2_grid_ss2 computes
    per row,
        u_(-1) = 0,  z_n = y_n - u_(n-1)[0],  u_n = A_n u_(n-1) + g_n y_n,   h = 0.5 sum_n omega_n z_n^2 = 0.5 y^T K^-1 y,
    A [T][2][2], g [T][2], omega [T] from datasets.ss2_system; the determinant of K depends on the dataset only and is
    dropped.  y: [..., T] residuals.  A sequential loop over T, vectorised over the rows, in `dtype` (np.longdouble: the
    tests' reference)."""
    y = np.asarray(y, dtype=dtype)
    T = y.shape[-1]
    A = np.asarray(A, dtype=dtype).reshape(T, 2, 2)
    g = np.asarray(g, dtype=dtype).reshape(T, 2)
    omega = np.asarray(omega, dtype=dtype).reshape(T)
    u0 = np.zeros(y.shape[:-1], dtype=dtype)
    u1 = np.zeros(y.shape[:-1], dtype=dtype)
    h = np.zeros(y.shape[:-1], dtype=dtype)
    for n in range(T):
        yn = y[..., n]
        z = yn - u0
        h = h + omega[n] * z * z
        u0, u1 = (A[n, 0, 0] * u0 + A[n, 0, 1] * u1 + g[n, 0] * yn,
                  A[n, 1, 0] * u0 + A[n, 1, 1] * u1 + g[n, 1] * yn)
    return h * dtype(0.5)


def ou_innovations(x, alpha, beta, dtype=np.float64):
    """The innovations of x [..., T] under the Kalman recurrence of datasets.ou_system: z_n = x_n - g_n, g_0 = 0,
    g_n = alpha_n g_(n-1) + beta_n x_(n-1) -- what ou_halfchi2 squares, and what whitens a baseline column as it whitens
    the residuals: x^T K^-1 x' = sum_n omega_n z[x]_n z[x']_n.  In `dtype`, the operations of ou_halfchi2 in its order."""
    x = np.asarray(x, dtype=dtype)
    alpha, beta = np.asarray(alpha, dtype=dtype), np.asarray(beta, dtype=dtype)
    z = np.empty(x.shape, dtype=dtype)
    g = np.zeros(x.shape[:-1], dtype=dtype)
    for n in range(x.shape[-1]):
        if n > 0:
            g = alpha[n] * g + beta[n] * x[..., n - 1]
        z[..., n] = x[..., n] - g
    return z


def ou_baseline_halfchi2(y, system, dtype=np.float64, return_coef=False):
    """chi^2/2 of a light curve's residuals with a linear baseline sum_k c_k B_k[t], c_k ~ N(0, s_k^2) independent,
    marginalised under white plus exponential noise K, on the host: the statement of what
    trxg_chi2_grid_ou_baseline computes per row,
        h = 0.5 [y^T K^-1 y - b^T A^-1 b],   b = B^T K^-1 y,   A = B^T K^-1 B + diag(1 / s_k^2),
    (for finite priors 0.5 y^T (K + B diag(s^2) B^T)^-1 y) in the innovations z = ou_innovations(y) and the scaled form of
    `system` (datasets.ou_baseline_system: omega, c, M):
        S2 = sum_n omega_n z_n^2,   b~_k = sum_n c_k[n] z_n,   h = 0.5 max(S2 - b~^T M b~, 0).
    The factors det K and det(I + diag(s^2) B^T K^-1 B) depend on the dataset alone and are dropped.  y: [..., T]
    residuals; in `dtype` (np.longdouble: the tests' reference).  S2 is summed as ou_halfchi2 sums it: M = 0 gives its
    bits.  return_coef: (h, coef~ [..., K]), coef~ = M b~ the scaled posterior-mean coefficients, c_k = coef~_k / sqrt(D_k)."""
    z = ou_innovations(y, system.alpha, system.beta, dtype)
    omega = np.asarray(system.omega, dtype=dtype)
    c = np.asarray(system.c, dtype=dtype)
    M = np.asarray(system.M, dtype=dtype)
    S2 = np.zeros(z.shape[:-1], dtype=dtype)
    for n in range(z.shape[-1]):                                  # (ou_halfchi2's order: its bits at M = 0)
        zn = z[..., n]
        S2 = S2 + omega[n] * zn * zn
    b = z @ c.T
    coef = b @ M                                                  # (M is symmetric)
    q = np.sum(b * coef, axis=-1)
    with np.errstate(invalid="ignore"):
        tot = S2 - q
        h = np.where(tot < 0, dtype(0.0), tot) * dtype(0.5)       # (a NaN stays a NaN)
    h = np.asarray(h, dtype=dtype)
    return (h, coef) if return_coef else h


def ss2_innovations(x, A, g, dtype=np.float64):
    """The innovations of x [..., T] under the Kalman recurrence of datasets.ss2_system: z_n = x_n - u_(n-1)[0], u_(-1) = 0,
    u_n = A_n u_(n-1) + g_n x_n -- what ss2_halfchi2 squares, and what whitens a baseline column as it whitens the
    residuals: x^T K^-1 x' = sum_n omega_n z[x]_n z[x']_n.  In `dtype`, the operations of ss2_halfchi2 in its order."""
    x = np.asarray(x, dtype=dtype)
    T = x.shape[-1]
    A = np.asarray(A, dtype=dtype).reshape(T, 2, 2)
    g = np.asarray(g, dtype=dtype).reshape(T, 2)
    z = np.empty(x.shape, dtype=dtype)
    u0 = np.zeros(x.shape[:-1], dtype=dtype)
    u1 = np.zeros(x.shape[:-1], dtype=dtype)
    for n in range(T):
        xn = x[..., n]
        z[..., n] = xn - u0
        u0, u1 = (A[n, 0, 0] * u0 + A[n, 0, 1] * u1 + g[n, 0] * xn,
                  A[n, 1, 0] * u0 + A[n, 1, 1] * u1 + g[n, 1] * xn)
    return z


def ss2_baseline_halfchi2(y, system, dtype=np.float64, return_coef=False):
    """ou_baseline_halfchi2 for noise with a two-dimensional state -- a Matern-3/2 term, two exponential terms -- (DESIGN.md
    section 14), on the host: the statement of what trxk_chi2_grid_ss2_baseline computes per row,
        h = 0.5 [y^T K^-1 y - b^T A^-1 b],   b = B^T K^-1 y,   A = B^T K^-1 B + diag(1 / s_k^2),
    (for finite priors 0.5 y^T (K + B diag(s^2) B^T)^-1 y) in the innovations z = ss2_innovations(y) and the scaled form of
    `system` (datasets.ss2_baseline_system: A, g, omega, c, M):
        S2 = sum_n omega_n z_n^2,   b~_k = sum_n c_k[n] z_n,   h = 0.5 max(S2 - b~^T M b~, 0).
    The factors det K and det(I + diag(s^2) B^T K^-1 B) depend on the dataset alone and are dropped.  y: [..., T]
    residuals; in `dtype` (np.longdouble: the tests' reference).  S2 is summed as ss2_halfchi2 sums it: M = 0 gives its
    bits.  return_coef: (h, coef~ [..., K]), coef~ = M b~ the scaled posterior-mean coefficients, c_k = coef~_k / sqrt(D_k)."""
    z = ss2_innovations(y, system.A, system.g, dtype)
    omega = np.asarray(system.omega, dtype=dtype).reshape(-1)
    c = np.asarray(system.c, dtype=dtype)
    M = np.asarray(system.M, dtype=dtype)
    S2 = np.zeros(z.shape[:-1], dtype=dtype)
    for n in range(z.shape[-1]):                                  # (ss2_halfchi2's order: its bits at M = 0)
        zn = z[..., n]
        S2 = S2 + omega[n] * zn * zn
    b = z @ c.T
    coef = b @ M                                                  # (M is symmetric)
    q = np.sum(b * coef, axis=-1)
    with np.errstate(invalid="ignore"):
        tot = S2 - q
        h = np.where(tot < 0, dtype(0.0), tot) * dtype(0.5)       # (a NaN stays a NaN)
    h = np.asarray(h, dtype=dtype)
    return (h, coef) if return_coef else h


def ou_mix_halfchi2(y, alpha, beta, omega, lnc, dtype=np.float64, return_candidates=False):
    """A dataset's term of the log-weight with the amplitude and time scale of its correlated noise marginalised over J
    candidates, on the host: the statement of what trxm_chi2_grid_ou_mix computes per row,
        h_j = ou_halfchi2(y, alpha[j], beta[j], omega[j]),  a_j = h_j - lnc_j,  m = min_j a_j,
        T = m - ln sum_j exp(m - a_j) = -ln sum_j exp(lnc_j - h_j),   stored as 0 where rounding drives it below,
    alpha, beta, omega [J][T] and lnc [J] from datasets.ou_mix_system; the terms are summed in ascending j.  y: [..., T]
    residuals.  In `dtype` (np.longdouble: the tests' reference).  J = 1 with lnc = 0 gives ou_halfchi2's bits.
    return_candidates: (T, h [..., J])."""
    lnc = np.asarray(lnc, dtype=dtype)
    h = np.stack([ou_halfchi2(y, alpha[j], beta[j], omega[j], dtype=dtype) for j in range(lnc.size)], axis=-1)
    a = h - lnc
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        m = np.fmin.reduce(a, axis=-1)
        s = np.zeros(m.shape, dtype=dtype)
        for j in range(lnc.size):
            s = s + np.exp(m - a[..., j])
        t = np.where(m < np.inf, m - np.log(s), m)                # (every candidate +inf, or a NaN row: no inf - inf)
        t = np.where(t < 0, dtype(0.0), t)                        # (a NaN stays a NaN)
    t = np.asarray(t, dtype=dtype)
    return (t, h) if return_candidates else t


def white_mix_halfchi2(y, w, lnc, dtype=np.float64, return_candidates=False):
    """A dataset's term of the log-weight with the size of its white noise marginalised over J candidates (DESIGN.md section
    14), on the host: the statement of what trxv_chi2_grid_white_mix computes per row,
        h_j = 0.5 sum_t w_j[t] y_t^2,  a_j = h_j - lnc_j,  m = min_j a_j,
        T = m - ln sum_j exp(m - a_j) = -ln sum_j exp(lnc_j - h_j),   stored as 0 where rounding drives it below,
    w [J][T] and lnc [J] from datasets.white_mix_system; the terms are summed in ascending j.  y: [..., T] residuals.  In
    `dtype` (np.longdouble: the tests' reference).  J = 1 with lnc = 0 gives the plain weighted chi^2/2,
    0.5 * sum(w[0] * y * y).  return_candidates: (T, h [..., J])."""
    y = np.asarray(y, dtype=dtype)
    w = np.atleast_2d(np.asarray(w, dtype=dtype))
    lnc = np.asarray(lnc, dtype=dtype)
    assert w.shape[0] == lnc.size and lnc.ndim == 1
    h = np.stack([dtype(0.5) * np.sum(w[j] * y * y, axis=-1) for j in range(lnc.size)], axis=-1)
    a = h - lnc
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        m = np.fmin.reduce(a, axis=-1)
        s = np.zeros(m.shape, dtype=dtype)
        for j in range(lnc.size):
            s = s + np.exp(m - a[..., j])
        t = np.where(m < np.inf, m - np.log(s), m)                # (every candidate +inf, or a NaN row: no inf - inf)
        t = np.where(t < 0, dtype(0.0), t)                        # (a NaN stays a NaN)
    t = np.asarray(t, dtype=dtype)
    return (t, h) if return_candidates else t


def white_baseline_halfchi2(y, system, dtype=np.float64, return_candidates=False, return_coef=False):
    """A dataset's term of the log-weight with the size of its white noise marginalised over J candidates and K baseline
    columns marginalised under every candidate, on the host: the statement of what
    trxb_chi2_grid_white_baseline computes per row,
        S2_j = sum_t w_j[t] y_t^2,   b_jk = sum_t w_j[t] B_k[t] y_t,   coef_j = A_j^-1 b_j,
        h_j = 0.5 max(S2_j - b_j . coef_j, 0),   a_j = h_j - lnc_j,  m = min_j a_j,
        T = m - ln sum_j exp(m - a_j) = -ln sum_j exp(lnc_j - h_j),   stored as 0 where rounding drives it below,
    `system` from datasets.white_baseline_system (w [J][T], B [K][T], minv [J][K (K + 1) / 2] the packed A_j^-1, lnc [J]); the
    terms are summed in ascending j.  y: [..., T] residuals.  In `dtype` (np.longdouble: the tests' reference).  minv = 0
    gives white_mix_halfchi2 on (w, lnc).  Returns T, then with return_candidates h [..., J], then with return_coef
    coef [..., J, K], the posterior-mean coefficients under each candidate."""
    y = np.asarray(y, dtype=dtype)
    w = np.atleast_2d(np.asarray(system.w, dtype=dtype))
    B = np.atleast_2d(np.asarray(system.B, dtype=dtype))
    lnc = np.asarray(system.lnc, dtype=dtype)
    J, K = w.shape[0], B.shape[0]
    packed = np.asarray(system.minv, dtype=dtype).reshape(J, -1)
    iu = np.triu_indices(K)
    hs, coefs = [], []
    for j in range(J):
        Ainv = np.zeros((K, K), dtype=dtype)
        Ainv[iu] = packed[j]
        Ainv = Ainv + np.triu(Ainv, 1).T
        u = w[j] * y
        S2 = np.sum(u * y, axis=-1)
        b = u @ B.T
        coef = b @ Ainv                                           # (A_j^-1 is symmetric)
        with np.errstate(invalid="ignore"):
            tot = S2 - np.sum(b * coef, axis=-1)
            hs.append(np.where(tot < 0, dtype(0.0), tot) * dtype(0.5))        # (a NaN stays a NaN)
        coefs.append(coef)
    h = np.stack(hs, axis=-1)
    a = h - lnc
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        m = np.fmin.reduce(a, axis=-1)
        s = np.zeros(m.shape, dtype=dtype)
        for j in range(J):
            s = s + np.exp(m - a[..., j])
        t = np.where(m < np.inf, m - np.log(s), m)                # (every candidate +inf, or a NaN row: no inf - inf)
        t = np.where(t < 0, dtype(0.0), t)                        # (a NaN stays a NaN)
    out = (np.asarray(t, dtype=dtype),)
    if return_candidates:
        out += (h,)
    if return_coef:
        out += (np.stack(coefs, axis=-2),)
    return out if len(out) > 1 else out[0]


def t0_mix_halfchi2(h, lnpi):
    """A dataset's term of the log-weight with a transit-time shift marginalised over J nodes, on the
    host: the statement of what trxt_softmin_rows computes per row,
        a_j = h_j - lnpi_j,  m = min_j a_j,  T = m - ln sum_j exp(m - a_j) = -ln sum_j exp(lnpi_j - h_j),
    stored as 0 where rounding drives it below; m = +inf (every node excluded) or NaN is stored as it is.  h: [J][n] (or
    [J]), node j's term on the stamps time + shift_j; lnpi: [J] log prior weights (-inf: a node switched off).  The minimum
    and the sum run in ascending j.  In h's dtype (np.longdouble: the tests' reference).  J = 1 with lnpi = 0 returns
    h[0]'s bits."""
    h = np.asarray(h)
    dtype = h.dtype.type
    lnpi = np.asarray(lnpi, dtype=dtype)
    assert h.shape[0] == lnpi.size and lnpi.ndim == 1
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        a = [h[j] - lnpi[j] for j in range(lnpi.size)]
        m = a[0]
        for j in range(1, lnpi.size):
            m = np.fmin(m, a[j])
        s = np.zeros(np.shape(m), dtype=dtype)
        for j in range(lnpi.size):
            s = s + np.exp(m - a[j])
        t = np.where(m < np.inf, m - np.log(s), m)                # (every node +inf, or a NaN row: no inf - inf)
        t = np.where(t < 0, dtype(0.0), t)                        # (a NaN stays a NaN)
    return np.asarray(t, dtype=dtype)


def _robust_terms(resid, inv_var, c0, c1, k2):
    """(A, B) of robust_halfchi2, in resid's dtype"""
    d = np.asarray(resid)
    dtype = d.dtype.type if d.dtype.kind == "f" else np.float64
    d = np.asarray(d, dtype=dtype)
    w = np.asarray(inv_var, dtype=dtype)
    a = (dtype(0.5) * (w * d)) * d
    return a + dtype(c0), a * dtype(k2) + dtype(c1)


def robust_halfchi2(resid, inv_var, c0, c1, k2):
    """A dataset's term of the log-weight under the outlier mixture, on the host: the statement of
    what trxr_chi2_grid_robust computes per row.  With d = resid [..., T] (flux - model), w = inv_var [T] and the constants
    of datasets.robust_constants,
        a_t = 0.5 w_t d_t^2,  A_t = a_t + c0,  B_t = a_t k2 + c1,  lo_t = min(A_t, B_t),
        h = sum_t (lo_t - log1p(exp(-|A_t - B_t|)))  =  sum_t -ln[(1 - eps) e^(-a_t) + (eps / kappa) e^(-a_t / kappa^2)],
    stored as 0 where rounding drives the total below; a NaN stays a NaN.  Not halved: the terms are log-weights already.
    In resid's dtype (np.longdouble: the tests' reference)."""
    with np.errstate(invalid="ignore", over="ignore"):
        A, B = _robust_terms(resid, inv_var, c0, c1, k2)
        lo = np.minimum(A, B)
        h = np.sum(lo - np.log1p(np.exp(-np.abs(A - B))), axis=-1)
        h = np.where(h < 0, A.dtype.type(0.0), h)                 # (a NaN stays a NaN)
    return np.asarray(h, dtype=A.dtype)


def robust_responsibility(resid, inv_var, c0, c1, k2):
    """The posterior probability that each point is an outlier under robust_halfchi2's mixture, given the residuals:
    p_t = 1 / (1 + exp(B_t - A_t)), in resid's shape and dtype."""
    with np.errstate(invalid="ignore", over="ignore"):
        A, B = _robust_terms(resid, inv_var, c0, c1, k2)
        return np.asarray(1.0 / (1.0 + np.exp(B - A)), dtype=A.dtype)


def warp_identity():
    """the identity grid: [WARP_DIMS][WARP_BINS + 1] edges b / 64 (the map returns its input, ln J = 0, exactly)"""
    return np.tile(np.arange(WARP_BINS + 1) / WARP_BINS, (WARP_DIMS, 1))


def warp_apply(edges, y):
    """The kernel's map in numpy: edges [WARP_BINS + 1] of one slot, y uniforms in [0, 1) ->
    u = e[b] + (y 64 - b) (e[b + 1] - e[b]) with b = min(int(y 64), 63), kept below 1."""
    e = np.asarray(edges, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    s = y * WARP_BINS
    b = np.minimum(s.astype(np.int64), WARP_BINS - 1)
    u = e[b] + (s - b) * (e[b + 1] - e[b])
    return np.minimum(u, np.nextafter(1.0, 0.0))


def warp_lnj(edges, y):
    """ln of the map's Jacobian at y: log(64 (e[b + 1] - e[b]))"""
    e = np.asarray(edges, dtype=np.float64)
    b = np.minimum((np.asarray(y, dtype=np.float64) * WARP_BINS).astype(np.int64), WARP_BINS - 1)
    return np.log(WARP_BINS * (e[b + 1] - e[b]))


def warp_hist_bins(hist):
    """Branch blocks of trx_scenario_args.warp_hist -- [branches][TRX_WARP_BRANCH] 64-bit words (word 0 = X as a
    double's bits), or the same as doubles with X as a value (the row columns of sharding.run_units) -- combined into
    one [WARP_DIMS][WARP_BINS] array of weight: branch b counts with exp(X_b - max X); a branch without rows: not at
    all."""
    h = np.atleast_2d(np.asarray(hist))
    if h.dtype.kind in "ui":
        X = np.ascontiguousarray(h[:, 0]).astype(np.uint64).view(np.float64)
        h = h.astype(np.float64)
    else:
        h = h.astype(np.float64)
        X = h[:, 0]
    live = (h[:, 1] > 0) & np.isfinite(X)
    out = np.zeros((WARP_DIMS, WARP_BINS))
    if not live.any():
        return out
    top = X[live].max()
    for b in np.nonzero(live)[0]:
        out += np.exp(X[b] - top) * h[b, 8:8 + WARP_DIMS * WARP_BINS].reshape(WARP_DIMS, WARP_BINS)
    return out


def warp_refine(edges, hist, alpha=0.5, floor=0.1):
    """One refinement of an importance grid (the VEGAS rule, Lepage 1978 / 2021, per dimension).

    edges [WARP_DIMS][WARP_BINS + 1]: the grid the histogram was taken under; hist: what warp_hist_bins takes, or the
    [WARP_DIMS][WARP_BINS] array it returns.  Bin k of row d holds the evidence's weight of the draws whose uniform fell
    into the k-th bin of the grid -- the weights carry the grid's Jacobian, so this is the posterior's mass between
    edges k and k + 1.  Per dimension: normalise, smooth (d- + 6 d + d+) / 8, damp ((1 - d) / ln(1 / d)) ** alpha,
    resplit into WARP_BINS bins of equal damped weight, then mix with the identity -- F(u) = (1 - floor) F_grid(u) +
    floor u, new edges F^-1(b / 64) -- so that the proposal's density 1 / (64 width) is at least `floor` everywhere (a
    bounded weight: no region of the prior is starved).  A dimension whose histogram is all zero (the scenario does
    not consume it, or the pass found no weight) keeps its row -- the identity unless an earlier pass moved it; an
    unused dimension would otherwise add pure noise through ln J.  A flat histogram keeps the row as well."""
    edges = np.array(edges, dtype=np.float64)
    d_all = np.asarray(hist, dtype=np.float64) if np.shape(hist) == (WARP_DIMS, WARP_BINS) else warp_hist_bins(hist)
    if not 0.0 <= floor < 1.0:
        raise ValueError("floor must lie in [0, 1)")
    levels = np.arange(WARP_BINS + 1) / WARP_BINS
    out = edges.copy()
    for dim in range(WARP_DIMS):
        d = d_all[dim]
        total = d.sum()
        if not (total > 0 and np.isfinite(total)):
            continue
        d = d / total
        grid = edges[dim]
        if np.ptp(d) > 0:
            sm = np.empty_like(d)
            sm[1:-1] = (d[:-2] + 6.0 * d[1:-1] + d[2:]) / 8.0
            sm[0], sm[-1] = (7.0 * d[0] + d[1]) / 8.0, (d[-2] + 7.0 * d[-1]) / 8.0
            sm = sm / sm.sum()
            with np.errstate(divide="ignore", invalid="ignore"):
                damp = np.where((sm > 0) & (sm < 1), ((1.0 - sm) / -np.log(sm)) ** alpha, np.where(sm >= 1, 1.0, 0.0))
            damp = np.maximum(damp, 1e-30 * damp.max())           # (a strictly increasing cumulative sum)
            cum = np.concatenate([[0.0], np.cumsum(damp)])
            cum /= cum[-1]
            grid = np.interp(levels, cum, edges[dim])
            grid[0], grid[-1] = 0.0, 1.0
        # F at the grid's knots: b / 64 + floor (u - b / 64); piecewise linear between them, inverted at b / 64
        F = levels + floor * (grid - levels)
        new = np.interp(levels, F, grid)
        new[0], new[-1] = 0.0, 1.0
        out[dim] = new
    return out
