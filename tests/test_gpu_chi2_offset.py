"""chi2_rows_kernel<STAGE, Chi2Offset> (trx_chi2_grid_offset): the weighted row reduction with a constant
baseline offset of the light curve marginalised in closed form,
    h = 0.5 (S2 - S1^2 / (S0 + prior_prec)),  offset = S1 / (S0 + prior_prec),  S0 = sum w, S1 = sum w d, S2 = sum w d^2.

The yardstick is the same formula in np.longdouble on the downloaded grid.  Bars, none of them chosen from results:
  |d h| <= 1e-12 x 0.5 S2 + 1e-12, S2 the unprofiled sum: each sum carries at most n_time x 2^-53 relative error of its
        absolute terms (2.3e-13 at 2049 stamps) and S1^2 / S0 <= S2 (Cauchy-Schwarz), the form of DESIGN.md section 14;
  offset_out: 1e-12 relative + 1e-15;
  prior_prec = +inf: the bits of chi2_grid_weighted (S1^2 / inf = 0; S2 is formed term for term the same way).
Shapes: lanes without stamps (1, 2), one pair a lane (63, 64, 65 pairs are 31 .. 32), odd lengths (every second row off
its 16-byte boundary), both sides of the LDS staging limit (2048, 2049); odd row counts; and (CAPPED) more rows than
the capped grid has waves, so that a wave's trip takes two rows, an odd remainder of them."""
import ctypes
import math

import numpy as np
import pytest
import torch

from test_gpu_reductions import chi2_rows_blocks
from triceratops_amd import _lib, synth

pytestmark = pytest.mark.gpu

N_TIMES = [1, 2, 63, 64, 65, 129, 333, 2048, 2049]
NS = [1, 2, 3, 257]
CAPPED = [(65, 8195), (2048, 5123)]          # (n_time, n): 8 blocks a CU; 5 at the staged limit's 32 KB of LDS a block
SIGMA = 1e-3
INF = float("inf")
LD = np.longdouble
_cases = {}
_worst = {"h": 0.0, "offset": 0.0}


def _case(n_time, n):
    """a random grid near 1, weights spanning 10x, a light curve; per offset of 0, 3 and 100 mean sigma the longdouble
    sums (made once per shape, never changed)"""
    key = (n_time, n)
    if key not in _cases:
        rng = np.random.default_rng(synth.SEED + 7919 * n_time + n)
        g = 1.0 - np.abs(rng.normal(0.0, 2e-3, (n, n_time)))
        w = rng.uniform(1.0, 10.0, n_time) / (10.0 * SIGMA ** 2)
        sig_mean = float(np.mean(w ** -0.5))
        base = 1.0 + rng.normal(0.0, SIGMA, n_time)
        # one more double in front: views one double off the 16-byte boundary
        pad = torch.empty(n * n_time + 1, dtype=torch.float64, device=_lib.compute_device())
        pad[1:] = _lib.dev(g).reshape(-1)
        g_d = pad[1:].clone().view(n, n_time)
        g_off = pad[1:].view(n, n_time)
        assert g_d.data_ptr() % 16 == 0 and g_off.data_ptr() % 16 == 8
        gl = g_d.cpu().numpy().astype(LD)
        S0 = math.fsum(w.tolist())
        sums = {}
        for k in (0.0, 3.0, 100.0):
            flux = base + k * sig_mean
            d = flux.astype(LD)[None, :] - gl
            sums[k] = (flux, np.sum(w.astype(LD) * d, axis=1), np.sum(w.astype(LD) * d * d, axis=1))
        _cases[key] = dict(g_d=g_d, g_off=g_off, w=w, w_d=_lib.dev(w), S0=S0, sums=sums, sig_mean=sig_mean)
    return _cases[key]


def _ref(S0, S1, S2, prec):
    den = LD(S0) + LD(prec)
    return 0.5 * (S2 - S1 * S1 / den), S1 / den


def _bar(S2):
    return 1e-12 * 0.5 * S2.astype(np.float64) + 1e-12


@pytest.mark.parametrize("n_time, n", [(t, n) for n in NS for t in N_TIMES] + CAPPED)
def test_offset_reduction_matches_longdouble(n_time, n):
    if (n_time, n) in CAPPED:
        assert 4 * chi2_rows_blocks(n, n_time) < n
    c = _case(n_time, n)
    for k, (flux, S1, S2) in c["sums"].items():
        f_d = _lib.dev(flux)
        plain = _lib.chi2_grid_weighted(f_d, c["w_d"], c["g_d"])
        for prec in (0.0, c["S0"] / 3.0, 1e-6 * c["S0"]):
            off = torch.full((n,), -7.0, dtype=torch.float64, device=f_d.device)
            got = _lib.chi2_grid_offset(f_d, c["w_d"], c["g_d"], c["S0"], prec, offset_out=off)
            h_ref, c_ref = _ref(c["S0"], S1, S2, prec)
            err = np.abs(got.cpu().numpy().astype(LD) - h_ref).astype(np.float64)
            ratio = float((err / _bar(S2)).max())
            c_err = np.abs(off.cpu().numpy().astype(LD) - c_ref).astype(np.float64)
            c_ratio = float((c_err / (1e-12 * np.abs(c_ref).astype(np.float64) + 1e-15)).max())
            _worst["h"], _worst["offset"] = max(_worst["h"], ratio), max(_worst["offset"], c_ratio)
            print("n_time %d n %d offset %g sigma prior_prec %.3g: |d h| / bar %.3g, |d c| / bar %.3g (largest so far %.3g, %.3g)"
                  % (n_time, n, k, prec, ratio, c_ratio, _worst["h"], _worst["offset"]))
            assert ratio <= 1.0 and c_ratio <= 1.0
            assert (got.cpu().numpy() >= 0.0).all()
            # rows one double off their 16-byte boundary: the same bits; and again: the same bits
            off2 = torch.empty_like(off)
            assert torch.equal(_lib.chi2_grid_offset(f_d, c["w_d"], c["g_off"], c["S0"], prec, offset_out=off2), got)
            assert torch.equal(off2, off)
            assert torch.equal(_lib.chi2_grid_offset(f_d, c["w_d"], c["g_d"], c["S0"], prec), got)
        # no offset: chi2_grid_weighted, bit for bit, on both alignments; the offsets are 0
        off = torch.full((n,), -7.0, dtype=torch.float64, device=f_d.device)
        assert torch.equal(_lib.chi2_grid_offset(f_d, c["w_d"], c["g_d"], c["S0"], INF, offset_out=off), plain)
        assert torch.equal(_lib.chi2_grid_offset(f_d, c["w_d"], c["g_off"], c["S0"], INF), plain)
        assert (off == 0.0).all()
        assert torch.equal(_lib.chi2_grid_weighted(f_d, c["w_d"], c["g_off"]), plain)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("n_time", N_TIMES)
def test_flat_prior_is_shift_invariant(n_time, n):
    c = _case(n_time, n)
    base = _lib.chi2_grid_offset(_lib.dev(c["sums"][0.0][0]), c["w_d"], c["g_d"], c["S0"], 0.0).cpu().numpy()
    for k in (3.0, 100.0):
        flux, _, S2 = c["sums"][k]
        moved = _lib.chi2_grid_offset(_lib.dev(flux), c["w_d"], c["g_d"], c["S0"], 0.0).cpu().numpy()
        ratio = float((np.abs(moved - base) / _bar(S2)).max())
        print("n_time %d n %d shift %g sigma: |d h| / bar at the shifted S2 %.3g" % (n_time, n, k, ratio))
        assert ratio <= 1.0


@pytest.mark.parametrize("n_time", [65, 2049])
def test_secondary_rule_is_the_weighted_kernels(n_time):
    c = _case(n_time, 257)
    flux = c["sums"][3.0][0]
    f_d = _lib.dev(flux)
    rng = np.random.default_rng(n_time)
    sec = rng.uniform(0.0, 1.0, 257)
    sec[:7] = np.nan
    sec[7] = 0.5                                                   # equality excludes
    excluded = sec >= 0.5                                          # (false for NaN)
    assert excluded[7] and not excluded[:7].any() and 0 < excluded.sum() < 257
    sec_d = _lib.dev(sec)
    for g in (c["g_d"], c["g_off"]):
        got = _lib.chi2_grid_offset(f_d, c["w_d"], g, c["S0"], 0.0, sec_d, 0.5).cpu().numpy()
        want = _lib.chi2_grid_weighted(f_d, c["w_d"], g, sec_d, 0.5).cpu().numpy()
        assert np.array_equal(np.isposinf(got), excluded) and np.array_equal(np.isposinf(got), np.isposinf(want))
        assert not np.isnan(got).any()
        free = _lib.chi2_grid_offset(f_d, c["w_d"], g, c["S0"], 0.0).cpu().numpy()
        assert np.array_equal(got[~excluded], free[~excluded])
        # sec_limit = +inf: the rule is off
        assert np.array_equal(_lib.chi2_grid_offset(f_d, c["w_d"], g, c["S0"], 0.0, sec_d, INF).cpu().numpy(), free)


@pytest.mark.parametrize("n_time, n", [(64, 257), (333, 257), (2049, 257), CAPPED[0]], ids=["64", "333", "2049", "65-8195"])
def test_accumulates_onto_finite_inf_and_nan(n_time, n):
    if (n_time, n) in CAPPED:
        assert 4 * chi2_rows_blocks(n, n_time) < n
    c = _case(n_time, n)
    f_d = _lib.dev(c["sums"][3.0][0])
    h = _lib.chi2_grid_offset(f_d, c["w_d"], c["g_d"], c["S0"], 0.0).cpu().numpy()
    out0 = np.random.default_rng(n_time).uniform(0.0, 50.0, n)
    out0[::5] = np.inf
    out0[1::7] = np.nan
    fin = np.isfinite(out0)
    assert fin.sum() > 100 and np.isposinf(out0).sum() > 10 and np.isnan(out0).sum() > 10
    off = torch.empty(n, dtype=torch.float64, device=f_d.device)
    acc = _lib.chi2_grid_offset(f_d, c["w_d"], c["g_d"], c["S0"], 0.0, out=_lib.dev(out0).clone(),
                                offset_out=off).cpu().numpy()
    assert np.array_equal(acc[fin], out0[fin] + h[fin])
    assert np.array_equal(np.isposinf(acc), np.isposinf(out0)) and np.array_equal(np.isnan(acc), np.isnan(out0))
    # (the offsets do not depend on what out held)
    off2 = torch.empty_like(off)
    _lib.chi2_grid_offset(f_d, c["w_d"], c["g_d"], c["S0"], 0.0, offset_out=off2)
    assert torch.equal(off, off2)
    # with a rule of its own: +inf from either side
    sec = np.linspace(0.0, 1.0, n)
    acc = _lib.chi2_grid_offset(f_d, c["w_d"], c["g_d"], c["S0"], 0.0, _lib.dev(sec), 0.5,
                                out=_lib.dev(out0).clone()).cpu().numpy()
    assert np.array_equal(np.isposinf(acc), (np.isposinf(out0) | (sec >= 0.5)) & ~np.isnan(out0))


def test_arguments():
    c = _case(63, 3)
    f_d, w_d, grid = _lib.dev(c["sums"][0.0][0]), c["w_d"], c["g_d"]
    empty = _lib.chi2_grid_offset(f_d, w_d, grid[:0], c["S0"], 0.0)
    assert empty.shape == (0,)
    L = _lib.lib()
    out = torch.full((3,), -7.0, dtype=torch.float64, device=grid.device)
    off = torch.full((3,), -7.0, dtype=torch.float64, device=grid.device)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    nan = float("nan")
    p = (f_d.data_ptr(), w_d.data_ptr(), grid.data_ptr())
    S0, o, c_out = c["S0"], out.data_ptr(), off.data_ptr()
    assert L.trx_chi2_grid_offset(*p, 63, 0, None, INF, 0, o, S0, 0.0, c_out, st) == 0              # n == 0: nothing runs
    for args in ((None, p[1], p[2], 63, 3, None, INF, 0, o, S0, 0.0, c_out),
                 (p[0], None, p[2], 63, 3, None, INF, 0, o, S0, 0.0, c_out),
                 (p[0], p[1], None, 63, 3, None, INF, 0, o, S0, 0.0, c_out),
                 (*p, 63, 3, None, INF, 0, None, S0, 0.0, c_out),
                 (*p, 63, -1, None, INF, 0, o, S0, 0.0, c_out),
                 (*p, 0, 3, None, INF, 0, o, S0, 0.0, c_out),
                 (*p, 63, 3, None, INF, 0, o, 0.0, 0.0, c_out),
                 (*p, 63, 3, None, INF, 0, o, -S0, 0.0, c_out),
                 (*p, 63, 3, None, INF, 0, o, INF, 0.0, c_out),
                 (*p, 63, 3, None, INF, 0, o, nan, 0.0, c_out),
                 (*p, 63, 3, None, INF, 0, o, S0, -1.0, c_out),
                 (*p, 63, 3, None, INF, 0, o, S0, nan, c_out)):
        assert L.trx_chi2_grid_offset(*args, st) == 1                                               # TRX_ERR_ARG
        assert L.trx_last_error()
    torch.cuda.synchronize()
    assert (out == -7.0).all() and (off == -7.0).all()                                              # nothing was enqueued
    # a NULL offset_out and prior_prec = +inf are allowed
    assert L.trx_chi2_grid_offset(*p, 63, 3, None, INF, 0, o, S0, INF, None, st) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, _lib.chi2_grid_weighted(f_d, w_d, grid)) and (off == -7.0).all()
