"""Numerically stable reductions used by the marginal likelihoods.

Same call surface as the reference's triceratops/_numerics.py:
  _log_mean_exp(logw, *, N_total)   (_numerics.py:12-51)  -> HIP kernel trx_log_mean_exp
  _normalize_probabilities(lnZ)     (_numerics.py:54-76)  -> host arithmetic over the 18-75
                                                             scenario evidences
"""
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
