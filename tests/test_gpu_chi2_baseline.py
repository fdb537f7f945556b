"""chi2_rows_kernel<STAGE, Chi2Baseline<K>> (trx_chi2_grid_baseline): the weighted row reduction with a
linear baseline model sum_k c_k B_k[t] of the light curve marginalised in closed form,
    h = 0.5 max(S2 - b~^T M b~, 0),  coef = M b~,  S2 = sum w d^2,  b~_k = sum g_k d,  g_k = w B_k / sqrt(D_k),  M = A~^-1.

The yardstick is the same formula in np.longdouble on the grid the device holds, with a longdouble Cholesky solve of A~
(formed in longdouble from the columns the device holds).  Bars, none of them chosen from results:
  |d h| <= 1e-12 x 0.5 S2 x (1 + 4 sqrt(K / lambda_min)) + 1e-12, lambda_min the smallest eigenvalue of the case's A~: each
        sum carries at most n_time x 2^-53 relative error of its absolute terms (1.5e-13 at 1365 stamps), |d b~_k| <=
        eps sqrt(S2) by Cauchy-Schwarz in the scaled columns, and a perturbation d b~ moves the quadratic form by at most
        2 sqrt(S2) |d b~| / sqrt(lambda_min);
  coef_out (scaled coefficients): 1e-12 x sqrt(K S2) / lambda_min + 1e-15 per entry;
  minv = 0: the bits of chi2_grid_weighted (S2 is formed term for term the same way; S2 - 0 = S2).
Shapes: as many stamps as terms and one more, lanes without stamps, one pair a lane (63, 64, 65), odd lengths (every second
row off its 16-byte boundary), both sides of each K's LDS staging limit (1364, 1024, 818, 682 stamps); odd row counts; and
(CAPPED) more rows than the capped grid has waves, so that a wave's trip takes two rows, an odd remainder of them.  Columns u^p, p = 0 .. K - 1; the data shifted by 0, 3 and 100 mean sigma times (1 + u); flat priors
and A~ + I."""
import ctypes
import math

import numpy as np
import pytest
import torch

from test_gpu_reductions import chi2_rows_blocks
from triceratops_amd import _lib, synth
from triceratops_amd.datasets import linear_system

pytestmark = pytest.mark.gpu

KS = [1, 2, 3, 4]
STAGE_MAX = {1: 1364, 2: 1024, 3: 818, 4: 682}
NS = [1, 2, 3, 257]
CAPPED = [(4, 65, 8195), (1, 1364, 5123)]          # (K, n_time, n): 8 blocks a CU; 5 at K = 1's staged limit
SIGMA = 1e-3
INF = float("inf")
LD = np.longdouble
SHIFTS = (0.0, 3.0, 100.0)
_hosts, _cases = {}, {}
_worst = {"h": 0.0, "coef": 0.0}


def _n_times(K):
    return sorted({K, K + 1, 63, 64, 65, 129, 333, STAGE_MAX[K], STAGE_MAX[K] + 1})


def _cholesky_solve(A, b):
    """x with A x = b in the dtype of A (longdouble: numpy's solvers are float64); A [K][K] positive definite, b [n][K]"""
    K = A.shape[0]
    Lo = np.zeros_like(A)
    for i in range(K):
        for j in range(i + 1):
            s = A[i, j] - np.sum(Lo[i, :j] * Lo[j, :j])
            Lo[i, j] = np.sqrt(s) if i == j else s / Lo[j, j]
    y = np.zeros_like(b)
    for i in range(K):
        y[:, i] = (b[:, i] - y[:, :i] @ Lo[i, :i]) / Lo[i, i]
    x = np.zeros_like(b)
    for i in reversed(range(K)):
        x[:, i] = (y[:, i] - x[:, i + 1:] @ Lo[i + 1:, i]) / Lo[i, i]
    return x


def _host_case(K, n_time, n):
    """a random grid near 1 and weights spanning 10x, built as tests/test_gpu_chi2_offset.py builds them; the columns u^p
    and, per prior (flat; A~ + I) the system of the host and its longdouble restatement; per shift the light curve and the
    longdouble sums and results (made once per shape, never changed)"""
    key = (K, n_time, n)
    if key in _hosts:
        return _hosts[key]
    rng = np.random.default_rng(synth.SEED + 7919 * n_time + n)
    g = 1.0 - np.abs(rng.normal(0.0, 2e-3, (n, n_time)))
    w = rng.uniform(1.0, 10.0, n_time) / (10.0 * SIGMA ** 2)
    sig_mean = float(np.mean(w ** -0.5))
    base = 1.0 + rng.normal(0.0, SIGMA, n_time)
    u = np.linspace(-1.0, 1.0, n_time) if n_time > 1 else np.zeros(1)
    B = np.stack([u ** p for p in range(K)])
    flat = linear_system(w, B, INF)
    priors = {"flat": flat, "plus_identity": linear_system(w, B, 1.0 / np.sqrt(flat.D))}
    systems = {}
    for name, s in priors.items():
        gl = s.g.astype(LD)
        # (the Gram matrix of the columns the device holds, in longdouble: the host's own A~ to its rounding)
        A = (gl / w.astype(LD)) @ gl.T + (LD(0) if name == "flat" else np.eye(K, dtype=LD))
        assert np.abs(A.astype(np.float64) - s.A).max() <= 1e-14 and s.lambda_min >= 1e-6
        systems[name] = dict(g=s.g, minv=s.minv, A=A, lam=s.lambda_min)
    gl = g.astype(LD)
    shifts = {}
    for k in SHIFTS:
        flux = base + k * sig_mean * (1.0 + u)
        d = flux.astype(LD)[None, :] - gl
        S2 = np.sum(w.astype(LD) * d * d, axis=1)
        per = {}
        for name, s in systems.items():
            b = d @ s["g"].astype(LD).T
            c = _cholesky_solve(s["A"], b)
            per[name] = (np.maximum(0.5 * (S2 - np.sum(b * c, axis=1)), LD(0)), c)
        shifts[k] = dict(flux=flux, S2=S2.astype(np.float64), ref=per)
    _hosts[key] = dict(K=K, g=g, w=w, B=B, sig_mean=sig_mean, systems=systems, shifts=shifts, S0=math.fsum(w.tolist()))
    return _hosts[key]


def _bar(S2, K, lam):
    return 1e-12 * 0.5 * S2 * (1.0 + 4.0 * math.sqrt(K / lam)) + 1e-12


def _coef_bar(S2, K, lam):
    return 1e-12 * np.sqrt(K * S2) / lam + 1e-15


def _case(K, n_time, n):
    key = (K, n_time, n)
    if key not in _cases:
        c = dict(_host_case(K, n_time, n))
        # one more double in front: views one double off the 16-byte boundary
        pad = torch.empty(n * n_time + 1, dtype=torch.float64, device=_lib.compute_device())
        pad[1:] = _lib.dev(c["g"]).reshape(-1)
        c["g_d"] = pad[1:].clone().view(n, n_time)
        c["g_off"] = pad[1:].view(n, n_time)
        assert c["g_d"].data_ptr() % 16 == 0 and c["g_off"].data_ptr() % 16 == 8
        assert np.array_equal(c["g_d"].cpu().numpy(), c["g"])                     # (the yardstick's grid is the device's)
        c["w_d"] = _lib.dev(c["w"])
        c["wb_d"] = {name: _lib.dev(s["g"]) for name, s in c["systems"].items()}
        _cases[key] = c
    return _cases[key]


@pytest.mark.parametrize("K, n_time, ns", [pytest.param(K, t, NS, id="%d-%d" % (K, t)) for K in KS for t in _n_times(K)]
                         + [pytest.param(K, t, [n], id="%d-%d-%d" % (K, t, n)) for K, t, n in CAPPED])
def test_baseline_reduction_matches_longdouble(K, n_time, ns):
    for n in ns:
        if (K, n_time, n) in CAPPED:
            assert 4 * chi2_rows_blocks(n, n_time, 2 + K, STAGE_MAX[K]) < n
        c = _case(K, n_time, n)
        for k, sh in c["shifts"].items():
            f_d = _lib.dev(sh["flux"])
            plain = _lib.chi2_grid_weighted(f_d, c["w_d"], c["g_d"])
            for name, s in c["systems"].items():
                wb = c["wb_d"][name]
                coef = torch.full((n, K), -7.0, dtype=torch.float64, device=f_d.device)
                got = _lib.chi2_grid_baseline(f_d, c["w_d"], c["g_d"], wb, s["minv"], coef_out=coef)
                h_ref, c_ref = sh["ref"][name]
                got_h = got.cpu().numpy()
                err = np.abs(got_h.astype(LD) - h_ref).astype(np.float64)
                ratio = float((err / _bar(sh["S2"], K, s["lam"])).max())
                c_err = np.abs(coef.cpu().numpy().astype(LD) - c_ref).astype(np.float64)
                c_ratio = float((c_err / _coef_bar(sh["S2"], K, s["lam"])[:, None]).max())
                _worst["h"], _worst["coef"] = max(_worst["h"], ratio), max(_worst["coef"], c_ratio)
                print("K %d n_time %d n %d shift %g sigma %s lambda_min %.3g: |d h| / bar %.3g, |d coef| / bar %.3g "
                      "(largest so far %.3g, %.3g)" % (K, n_time, n, k, name, s["lam"], ratio, c_ratio, _worst["h"],
                                                       _worst["coef"]))
                assert ratio <= 1.0 and c_ratio <= 1.0
                assert (got_h >= 0.0).all()
                # rows one double off their 16-byte boundary: the same bits; and again: the same bits
                coef2 = torch.empty_like(coef)
                assert torch.equal(_lib.chi2_grid_baseline(f_d, c["w_d"], c["g_off"], wb, s["minv"], coef_out=coef2), got)
                assert torch.equal(coef2, coef)
                assert torch.equal(_lib.chi2_grid_baseline(f_d, c["w_d"], c["g_d"], wb, s["minv"]), got)
            # M = 0: chi2_grid_weighted, bit for bit, on both alignments; the coefficients are 0
            wb, zero = c["wb_d"]["flat"], np.zeros(K * (K + 1) // 2)
            coef = torch.full((n, K), -7.0, dtype=torch.float64, device=f_d.device)
            assert torch.equal(_lib.chi2_grid_baseline(f_d, c["w_d"], c["g_d"], wb, zero, coef_out=coef), plain)
            assert torch.equal(_lib.chi2_grid_baseline(f_d, c["w_d"], c["g_off"], wb, zero), plain)
            assert (coef == 0.0).all()


@pytest.mark.parametrize("K", [2, 3, 4])
def test_flat_priors_absorb_the_trend(K):
    """K >= 2: the shift k sigma (1 + u) lies in the span of the columns, so the flat-prior value does not move"""
    for n_time in (65, STAGE_MAX[K] + 1):
        c = _case(K, n_time, 257)
        s = c["systems"]["flat"]
        base = _lib.chi2_grid_baseline(_lib.dev(c["shifts"][0.0]["flux"]), c["w_d"], c["g_d"], c["wb_d"]["flat"],
                                       s["minv"]).cpu().numpy()
        for k in (3.0, 100.0):
            sh = c["shifts"][k]
            moved = _lib.chi2_grid_baseline(_lib.dev(sh["flux"]), c["w_d"], c["g_d"], c["wb_d"]["flat"],
                                            s["minv"]).cpu().numpy()
            ratio = float((np.abs(moved - base) / _bar(sh["S2"], K, s["lam"])).max())
            print("K %d n_time %d shift %g sigma: |d h| / bar at the shifted S2 %.3g" % (K, n_time, k, ratio))
            assert ratio <= 1.0


@pytest.mark.parametrize("n_time", [1, 2, 65, 333, 1364, 1365])
def test_one_column_of_ones_is_the_offset_reduction(n_time):
    for n in (3, 257):
        c = _case(1, n_time, n)
        assert np.array_equal(c["B"], np.ones((1, n_time)))
        for k, sh in c["shifts"].items():
            f_d = _lib.dev(sh["flux"])
            for name, prec in (("flat", 0.0), ("plus_identity", None)):
                s = c["systems"][name]
                if prec is None:
                    prec = math.fsum((c["w"] * c["B"][0] ** 2).tolist())             # A~ + I: 1 / s^2 = D
                coef = torch.empty((n, 1), dtype=torch.float64, device=f_d.device)
                off = torch.empty(n, dtype=torch.float64, device=f_d.device)
                a = _lib.chi2_grid_baseline(f_d, c["w_d"], c["g_d"], c["wb_d"][name], s["minv"], coef_out=coef).cpu().numpy()
                b = _lib.chi2_grid_offset(f_d, c["w_d"], c["g_d"], c["S0"], prec, offset_out=off).cpu().numpy()
                ratio = float((np.abs(a - b) / _bar(sh["S2"], 1, s["lam"])).max())
                # the offset in flux units: coef / sqrt(D)
                d_c = np.abs(coef.cpu().numpy()[:, 0] / math.sqrt(c["S0"]) - off.cpu().numpy())
                c_ratio = float((d_c * math.sqrt(c["S0"]) / _coef_bar(sh["S2"], 1, s["lam"])).max())
                print("n_time %d n %d shift %g %s: |h - offset kernel's| / bar %.3g, coefficient %.3g" % (n_time, n, k, name, ratio, c_ratio))
                assert ratio <= 1.0 and c_ratio <= 1.0


@pytest.mark.parametrize("K, n_time", [(1, 65), (2, 1025), (4, 65), (4, 683)])
def test_secondary_rule_is_the_weighted_kernels(K, n_time):
    c = _case(K, n_time, 257)
    f_d = _lib.dev(c["shifts"][3.0]["flux"])
    wb, minv = c["wb_d"]["flat"], c["systems"]["flat"]["minv"]
    rng = np.random.default_rng(n_time)
    sec = rng.uniform(0.0, 1.0, 257)
    sec[:7] = np.nan
    sec[7] = 0.5                                                   # equality excludes
    excluded = sec >= 0.5                                          # (false for NaN)
    assert excluded[7] and not excluded[:7].any() and 0 < excluded.sum() < 257
    sec_d = _lib.dev(sec)
    for g in (c["g_d"], c["g_off"]):
        got = _lib.chi2_grid_baseline(f_d, c["w_d"], g, wb, minv, sec_d, 0.5).cpu().numpy()
        want = _lib.chi2_grid_weighted(f_d, c["w_d"], g, sec_d, 0.5).cpu().numpy()
        assert np.array_equal(np.isposinf(got), excluded) and np.array_equal(np.isposinf(got), np.isposinf(want))
        assert not np.isnan(got).any()
        free = _lib.chi2_grid_baseline(f_d, c["w_d"], g, wb, minv).cpu().numpy()
        assert np.array_equal(got[~excluded], free[~excluded])
        # sec_limit = +inf: the rule is off
        assert np.array_equal(_lib.chi2_grid_baseline(f_d, c["w_d"], g, wb, minv, sec_d, INF).cpu().numpy(), free)


@pytest.mark.parametrize("K, n_time", [(1, 64), (3, 333), (4, 683)])
def test_accumulates_onto_finite_inf_and_nan(K, n_time):
    c = _case(K, n_time, 257)
    f_d = _lib.dev(c["shifts"][3.0]["flux"])
    wb, minv = c["wb_d"]["plus_identity"], c["systems"]["plus_identity"]["minv"]
    h = _lib.chi2_grid_baseline(f_d, c["w_d"], c["g_d"], wb, minv).cpu().numpy()
    out0 = np.random.default_rng(n_time).uniform(0.0, 50.0, 257)
    out0[::5] = np.inf
    out0[1::7] = np.nan
    fin = np.isfinite(out0)
    assert fin.sum() > 100 and np.isposinf(out0).sum() > 10 and np.isnan(out0).sum() > 10
    coef = torch.empty((257, K), dtype=torch.float64, device=f_d.device)
    acc = _lib.chi2_grid_baseline(f_d, c["w_d"], c["g_d"], wb, minv, out=_lib.dev(out0).clone(), coef_out=coef).cpu().numpy()
    assert np.array_equal(acc[fin], out0[fin] + h[fin])
    assert np.array_equal(np.isposinf(acc), np.isposinf(out0)) and np.array_equal(np.isnan(acc), np.isnan(out0))
    # (the coefficients do not depend on what out held)
    coef2 = torch.empty_like(coef)
    _lib.chi2_grid_baseline(f_d, c["w_d"], c["g_d"], wb, minv, coef_out=coef2)
    assert torch.equal(coef, coef2)
    # with a rule of its own: +inf from either side
    sec = np.linspace(0.0, 1.0, 257)
    acc = _lib.chi2_grid_baseline(f_d, c["w_d"], c["g_d"], wb, minv, _lib.dev(sec), 0.5, out=_lib.dev(out0).clone()).cpu().numpy()
    assert np.array_equal(np.isposinf(acc), (np.isposinf(out0) | (sec >= 0.5)) & ~np.isnan(out0))


def test_arguments():
    c = _case(2, 63, 3)
    f_d, w_d, grid, wb = _lib.dev(c["shifts"][0.0]["flux"]), c["w_d"], c["g_d"], c["wb_d"]["flat"]
    minv = np.ascontiguousarray(c["systems"]["flat"]["minv"])
    assert _lib.chi2_grid_baseline(f_d, w_d, grid[:0], wb, minv).shape == (0,)
    L = _lib.lib()
    out = torch.full((3,), -7.0, dtype=torch.float64, device=grid.device)
    coef = torch.full((3, 2), -7.0, dtype=torch.float64, device=grid.device)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = (f_d.data_ptr(), w_d.data_ptr(), grid.data_ptr())
    o, g, m, co = out.data_ptr(), wb.data_ptr(), minv.ctypes.data, coef.data_ptr()
    bad = minv.copy()
    bad[1] = np.nan
    huge = minv.copy()
    huge[2] = np.inf
    # (n_terms = 5: ten entries would be read if the count were not refused first)
    ten = np.zeros(15)
    assert L.trx_chi2_grid_baseline(*p, 63, 0, None, INF, 0, o, g, 2, m, co, st) == 0                  # n == 0: nothing runs
    for args in ((None, p[1], p[2], 63, 3, None, INF, 0, o, g, 2, m, co),
                 (p[0], None, p[2], 63, 3, None, INF, 0, o, g, 2, m, co),
                 (p[0], p[1], None, 63, 3, None, INF, 0, o, g, 2, m, co),
                 (*p, 63, 3, None, INF, 0, None, g, 2, m, co),
                 (*p, 63, 3, None, INF, 0, o, None, 2, m, co),
                 (*p, 63, 3, None, INF, 0, o, g, 2, None, co),
                 (*p, 63, -1, None, INF, 0, o, g, 2, m, co),
                 (*p, 0, 3, None, INF, 0, o, g, 2, m, co),
                 (*p, 63, 3, None, INF, 0, o, g, 0, ten.ctypes.data, co),
                 (*p, 63, 3, None, INF, 0, o, g, 5, ten.ctypes.data, co),
                 (*p, 63, 3, None, INF, 0, o, g, -1, ten.ctypes.data, co),
                 (*p, 63, 3, None, INF, 0, o, g, 2, bad.ctypes.data, co),
                 (*p, 63, 3, None, INF, 0, o, g, 2, huge.ctypes.data, co)):
        assert L.trx_chi2_grid_baseline(*args, st) == 1                                               # TRX_ERR_ARG
        assert L.trx_last_error()
    torch.cuda.synchronize()
    assert (out == -7.0).all() and (coef == -7.0).all()                                               # nothing was enqueued
    with pytest.raises(_lib.TrxError):
        _lib.chi2_grid_baseline(f_d, w_d, grid, wb, bad)
    # a NULL coef_out is allowed
    assert L.trx_chi2_grid_baseline(*p, 63, 3, None, INF, 0, o, g, 2, m, None, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, _lib.chi2_grid_baseline(f_d, w_d, grid, wb, minv)) and (coef == -7.0).all()
