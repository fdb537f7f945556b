"""chi2_white_lin_kernel<STAGE, J, K> (trxb_chi2_grid_white_baseline, include/trx_gls.h): the row
reduction of a model grid under white noise whose size is marginalised over J candidates, with K baseline columns
marginalised under every candidate,
    S2_j = sum w_j d^2,  b_jk = sum w_j B_k d,  coef_j = A_j^-1 b_j,  h_j = 0.5 max(S2_j - b_j . coef_j, 0),
    T = -ln sum_j exp(lnc_j - h_j)   (clamped at 0).

Yardsticks and bars, written before the first run:
  out against _numerics.white_baseline_halfchi2 in np.longdouble on the downloaded grid and the same tables:
      |d T| <= max_j bar_h(j) + 16 eps (1 + |T| + max|lnc|),
      bar_h(j) = 1e-12 x 0.5 S2_j x (1 + 4 sqrt(K / lambda_j)) + 1e-12,
  lambda_j the smallest eigenvalue of candidate j's unit-diagonal system: the first part is tests/test_gpu_chi2_baseline.py's
  bar for h (each sum carries at most n_time x 2^-53 of its absolute terms, |d b~_k| <= eps sqrt(S2) by Cauchy-Schwarz, and a
  perturbation d b~ moves the quadratic form by at most 2 sqrt(S2) |d b~| / sqrt(lambda)), the second the soft minimum's
  (tests/test_gpu_chi2_white_mix.py: T is 1-Lipschitz in the h_j);
  cand_out[:, j] against _lib.chi2_grid_baseline on candidate j's own system (datasets.linear_system): two device results,
  so 2 bar_h(j); coef_out[:, j, k] against that call's scaled coefficients / sqrt(D_jk) within
  2 (1e-12 sqrt(K S2_j) / lambda_j + 1e-15) / sqrt(D_jk), that file's coefficient bar twice;
  minv = 0 against _lib.chi2_grid_white_mix on the same weights and log-weights within that file's bar.
Shapes: one stamp, one pair, an odd three, both sides of a lane's last pair (63, 64, 65) and of the second (127, 128, 129), an
odd length with several trips (333), past every stage limit (2049), and both sides of the stage limit of every (J, K) used;
n = 1, 2, 3, 257; J = 1, 2, 3, 5, 8; K = 1, 2, 4 (J (1 + K) = 2 ... 40: two rows a pass up to 10 sums, one past that); flat
priors where n_time > K, finite ones (5 sigma) where not and in a test of their own; residuals at 0, 3 and 100 sigma; and
one CAPPED case per row mode with more rows than the capped grid has wave slots (_lib.white_lin_blocks).
Measured (one MI355X): the largest |d T| / bar of the whole file, printed by the last test, is 1.3e-4."""
import math

import numpy as np
import pytest
import torch

from test_gpu_chi2_ou import LEVELS, SIGMA, _case
from triceratops_amd import _lib, _numerics, synth
from triceratops_amd import datasets as D

pytestmark = pytest.mark.gpu

N_TIMES = [1, 2, 3, 63, 64, 65, 127, 128, 129, 333, 2049]
NS = [1, 2, 3, 257]
JS = [1, 2, 3, 5, 8]
KS = [1, 2, 4]
CAPPED = [(65, 16387, 3, 2), (65, 16387, 8, 4)]          # (n_time, n, J, K): two rows a pass; one row a pass
CANDS = [(1.0, 0.0, 0.2), (0.5, 0.0, 0.05), (2.0, 1.0, 0.1), (3.0, 0.0, 0.25), (1.5, 3.0, 0.1), (1.0, 0.5, 0.1),
         (2.5, 2.0, 0.15), (0.75, 0.1, 0.05)]
CLOSE = [(1.0 + 1e-5 * k, 1e-3 * k, 1.0) for k in range(8)]
INF = float("inf")
EPS = np.finfo(np.float64).eps
LD = np.longdouble
_systems = {}
_worst = {"t": 0.0, "h": 0.0, "coef": 0.0}


def stage_max(J, K):
    return ((2 * 2048) // (1 + J + K)) & ~1


def _system(n_time, J, K, prior="auto", cands=CANDS):
    """the light curve's errors (one set per n_time, those of test_gpu_chi2_white_mix.py), the first J candidates as its
    white_grid and the columns u^p, p < K, as its white_baseline: the host's system, per candidate the plain baseline
    system of its weights, and the device copies"""
    if prior == "auto":
        prior = "flat" if n_time > K else "finite"
    key = (n_time, J, K, prior, cands is CANDS)
    if key not in _systems:
        rng = np.random.default_rng(synth.SEED + 104729 * n_time)
        t = rng.uniform(-0.2, 0.2, n_time)                               # (folded: no order)
        err = SIGMA * rng.uniform(0.6, 1.8, n_time)
        u = np.linspace(-1.0, 1.0, n_time) if n_time > 1 else np.full(1, 0.5)
        B = np.stack([u ** p for p in range(K)])
        sig = np.full(K, INF if prior == "flat" else 5.0 * SIGMA)
        dicts = [{"time": t, "flux": np.ones(n_time), "flux_err": err,
                  "white_grid": [(k, s * SIGMA, w) for k, s, w in cands[:J]],
                  "white_baseline": B, "white_baseline_sigma": sig}]
        sets = D.validate(dicts)
        system = D.white_baseline_system(sets[0], D.white_grids(dicts, sets)[0], *D.white_baselines(dicts, sets)[0])
        per = [D.linear_system(system.w[j], B, sig) for j in range(J)]
        _systems[key] = dict(d=sets[0], sys=system, per=per, w_d=_lib.dev(system.w), B_d=_lib.dev(system.B),
                             g_d=[_lib.dev(p.g) for p in per], lam=np.asarray(system.lambda_min), K=K, J=J)
    return _systems[key]


def _lin(f_d, g, s, lnc=None, minv=None, **kw):
    return _lib.chi2_grid_white_baseline(f_d, g, s["w_d"], s["B_d"], s["sys"].minv if minv is None else minv,
                                         s["sys"].lnc if lnc is None else lnc, **kw)


def _s2(y, s):
    return np.stack([np.sum(s["sys"].w[j] * y * y, axis=-1) for j in range(s["J"])], axis=-1)


def _bar_h(S2, s):
    """[n][J]: test_gpu_chi2_baseline.py's bar for h, per candidate"""
    return 1e-12 * 0.5 * S2 * (1.0 + 4.0 * np.sqrt(s["K"] / s["lam"]))[None, :] + 1e-12


def _bar_t(S2, s, want, lnc):
    return _bar_h(S2, s).max(axis=-1) + 16 * EPS * (1.0 + np.abs(np.asarray(want, dtype=np.float64)) + np.abs(lnc).max())


def _check(n_time, n, J, K, levels, rows=None, prior="auto"):
    c = _case(n_time, n)
    s = _system(n_time, J, K, prior)
    sel = slice(None) if rows is None else rows
    for level in levels:
        f_d = _lib.dev(c["flux"][level])
        y = c["flux"][level][None, :] - c["g"][sel]
        S2 = _s2(y, s)
        h_ref = _numerics.white_baseline_halfchi2(y, s["sys"], LD, return_candidates=True)[1]
        balanced = np.asarray(h_ref[0] - h_ref[0].min(), dtype=np.float64) - np.log(J)
        for name, lnc in (("system", s["sys"].lnc), ("balanced", balanced)):
            want = _numerics.white_baseline_halfchi2(y, s["sys"]._replace(lnc=lnc), LD)
            assert want.dtype == LD
            cand = torch.full((n, J), -1.0, dtype=torch.float64, device=f_d.device)
            coef = torch.full((n, J, K), -1.0, dtype=torch.float64, device=f_d.device)
            got = _lin(f_d, c["g_d"], s, lnc, cand_out=cand, coef_out=coef)
            g = got.cpu().numpy()
            ratio = float((np.abs(g[sel].astype(LD) - want).astype(np.float64) / _bar_t(S2, s, want, lnc)).max())
            _worst["t"] = max(_worst["t"], ratio)
            print("n_time %d n %d J %d K %d level %g sigma, lnc %s: |d T| / bar %.3g (largest so far %.3g)"
                  % (n_time, n, J, K, level, name, ratio, _worst["t"]))
            assert ratio <= 1.0
            assert (g >= 0.0).all()
            # rows one double off their 16-byte boundary, and without the optional outputs: the same bits
            cand2, coef2 = torch.empty_like(cand), torch.empty_like(coef)
            assert torch.equal(_lin(f_d, c["g_off"], s, lnc, cand_out=cand2, coef_out=coef2), got)
            assert torch.equal(cand2, cand) and torch.equal(coef2, coef)
            assert torch.equal(_lin(f_d, c["g_d"], s, lnc), got)
        # every candidate against the plain baseline reduction on its own system
        hc, cc = cand.cpu().numpy(), coef.cpu().numpy()
        bar = _bar_h(S2, s)
        for j in range(J):
            p = s["per"][j]
            one_c = torch.empty((n, K), dtype=torch.float64, device=f_d.device)
            one = _lib.chi2_grid_baseline(f_d, s["w_d"][j].contiguous(), c["g_d"], s["g_d"][j], p.minv, coef_out=one_c)
            rh = float((np.abs(hc[sel, j] - one.cpu().numpy()[sel]) / (2.0 * bar[:, j])).max())
            cbar = 2.0 * (1e-12 * np.sqrt(K * S2[:, j]) / s["lam"][j] + 1e-15)[:, None] / np.sqrt(p.D)[None, :]
            rc = float((np.abs(cc[sel, j] - one_c.cpu().numpy()[sel] / np.sqrt(p.D)) / cbar).max())
            _worst["h"], _worst["coef"] = max(_worst["h"], rh), max(_worst["coef"], rc)
            assert rh <= 1.0 and rc <= 1.0, (j, rh, rc)


@pytest.mark.parametrize("n_time, n", [(t, n) for n in NS for t in N_TIMES])
def test_matches_the_longdouble_statement_and_the_candidates_own_baseline_reductions(n_time, n):
    for J in JS:
        for K in KS:
            _check(n_time, n, J, K, LEVELS if (n <= 3 or (J, K) in ((2, 1), (8, 4))) else (3.0,))


@pytest.mark.parametrize("J, K", [(J, K) for J in JS for K in KS])
def test_both_sides_of_the_stage_limit(J, K):
    limit = stage_max(J, K)
    by_regs = 4 if J * (1 + K) <= 24 else 3 if J * (1 + K) <= 35 else 2
    assert (1 + J + K) * limit * 8 <= 32768 < (1 + J + K) * (limit + 2) * 8        # (the staged vectors fill 32 KB, no more)
    assert _lib.white_lin_blocks(10 ** 6, limit, J, K) == _lib.white_lin_blocks(10 ** 6, limit + 1, J, K) == 256 * by_regs
    for n_time in (limit, limit + 1):
        _check(n_time, 3, J, K, (3.0,))
        _check(n_time, 257, J, K, (3.0,))


@pytest.mark.parametrize("n_time, n, J, K", CAPPED)
def test_past_the_capped_grid(n_time, n, J, K):
    blocks = _lib.white_lin_blocks(n, n_time, J, K)
    per_pass = 2 if J * (1 + K) <= 10 else 1
    assert 4 * blocks * per_pass < n                                 # (a further pass for some waves)
    rows = np.unique(np.concatenate([np.arange(64), np.arange(n - 64, n), 4 * blocks + np.arange(-8, 8),
                                     4 * blocks * per_pass + np.arange(-8, 8),
                                     np.random.default_rng(n_time).integers(0, n, 256)]))
    assert rows.max() == n - 1 and (rows > 4 * blocks * per_pass).any()
    _check(n_time, n, J, K, (3.0,), rows)


@pytest.mark.parametrize("n_time, n", [(3, 3), (65, 257), (333, 3), (2049, 3)])
def test_finite_priors(n_time, n):
    for J, K in ((1, 1), (2, 2), (3, 4), (8, 4)):
        _check(n_time, n, J, K, LEVELS, prior="finite")


@pytest.mark.parametrize("J, K", [(1, 1), (2, 4), (5, 2), (8, 4)])
@pytest.mark.parametrize("n_time, n", [(1, 3), (65, 257), (333, 257), (2049, 3)])
def test_minv_zero_is_the_white_mix_reduction(n_time, n, J, K):
    """minv = 0: h_j = 0.5 S2_j, so T is chi2_grid_white_mix's on the same weights and log-weights, within that file's bar
    (the sums are folded in another order), and the coefficients are 0"""
    c = _case(n_time, n)
    s = _system(n_time, J, K)
    lnc = s["sys"].lnc
    for level in LEVELS:
        f_d = _lib.dev(c["flux"][level])
        cand = torch.empty((n, J), dtype=torch.float64, device=f_d.device)
        coef = torch.empty((n, J, K), dtype=torch.float64, device=f_d.device)
        got = _lin(f_d, c["g_d"], s, minv=np.zeros_like(s["sys"].minv), cand_out=cand, coef_out=coef).cpu().numpy()
        mix_c = torch.empty_like(cand)
        mix = _lib.chi2_grid_white_mix(f_d, c["g_d"], s["w_d"], lnc, cand_out=mix_c).cpu().numpy()
        h = mix_c.cpu().numpy()
        bar = (1e-12 * h + 1e-12).max(axis=-1) + 16 * EPS * (1.0 + np.abs(mix) + np.abs(lnc).max())
        assert (np.abs(got - mix) <= bar).all(), float((np.abs(got - mix) / bar).max())
        assert (np.abs(cand.cpu().numpy() - h) <= 1e-12 * h + 1e-12).all()
        assert not coef.cpu().numpy().any()


@pytest.mark.parametrize("J, K", [(2, 1), (3, 4), (8, 2), (8, 4)])
@pytest.mark.parametrize("n_time, n", [(2, 3), (65, 257), (128, 257), (2049, 3)])
def test_candidates_at_minus_800_or_switched_off_do_not_reach_the_sum(n_time, n, J, K):
    """one candidate at lnc = 0, the others at -800: exp underflows to 0, the sum is 1, out has the bits of that candidate's
    h (on candidates whose h lie close together); then at -inf: switched off altogether"""
    c = _case(n_time, n)
    s = _system(n_time, J, K, cands=CLOSE)
    f_d = _lib.dev(c["flux"][3.0])
    for g in (c["g_d"], c["g_off"]):
        cand = torch.empty((n, J), dtype=torch.float64, device=f_d.device)
        _lin(f_d, g, s, cand_out=cand)
        assert float((cand.max(dim=1).values - cand.min(dim=1).values).max().cpu()) < 40.0
        for keep in sorted({0, J // 2, J - 1}):
            lnc = np.full(J, -800.0)
            lnc[keep] = 0.0
            assert torch.equal(_lin(f_d, g, s, lnc), cand[:, keep].contiguous())
            lnc[lnc < 0] = -INF
            assert torch.equal(_lin(f_d, g, s, lnc), cand[:, keep].contiguous())
    assert bool(torch.isposinf(_lin(f_d, c["g_d"], s, np.full(J, -INF))).all())


@pytest.mark.parametrize("J, K", [(2, 2), (3, 1), (8, 4)])
@pytest.mark.parametrize("n_time, n", [(65, 257), (128, 3), (333, 257), (2049, 3)])
def test_permuting_the_candidates(n_time, n, J, K):
    """a candidate's place decides the order in which its sums are folded, not their value: within the bars"""
    c = _case(n_time, n)
    s = _system(n_time, J, K)
    f_d = _lib.dev(c["flux"][3.0])
    y = c["flux"][3.0][None, :] - c["g"]
    S2 = _s2(y, s)
    cand = torch.empty((n, J), dtype=torch.float64, device=f_d.device)
    coef = torch.empty((n, J, K), dtype=torch.float64, device=f_d.device)
    _lin(f_d, c["g_d"], s, cand_out=cand)
    h0 = cand.cpu().numpy()[0]
    lnc = h0 - h0.min() - np.log(J)                                  # (balanced at row 0)
    got = _lin(f_d, c["g_d"], s, lnc, cand_out=cand, coef_out=coef).cpu().numpy()
    rng = np.random.default_rng(J + n_time)
    for perm in (np.arange(J)[::-1].copy(), rng.permutation(J)):
        p_d = torch.as_tensor(perm, device=cand.device)
        cand_p, coef_p = torch.empty_like(cand), torch.empty_like(coef)
        got_p = _lib.chi2_grid_white_baseline(f_d, c["g_d"], s["w_d"].index_select(0, p_d).contiguous(), s["B_d"],
                                              np.ascontiguousarray(s["sys"].minv[perm]), lnc[perm], cand_out=cand_p,
                                              coef_out=coef_p).cpu().numpy()
        bar = _bar_h(S2, s)
        assert (np.abs(cand_p.cpu().numpy() - cand.cpu().numpy()[:, perm]) <= 2.0 * bar[:, perm]).all()
        bar_t = 2.0 * bar.max(axis=-1) + 16 * EPS * (1.0 + np.abs(got) + np.abs(lnc).max())
        assert (np.abs(got_p - got) <= bar_t).all(), float((np.abs(got_p - got) / bar_t).max())


@pytest.mark.parametrize("n_time, n, J, K", [(65, 257, 3, 2), (65, 257, 8, 4), (314, 257, 8, 4), (315, 257, 8, 4),
                                             (2049, 257, 2, 1), (2049, 257, 8, 4)] + CAPPED)
def test_a_rows_bits_are_its_own(n_time, n, J, K):
    """the same row at position 0, 1 and n - 1 (behind the capped grid where n says so), in launches of one and of two rows
    (other grids of blocks), in a view one double off, and on a second run: out, cand_out and coef_out"""
    c = _case(n_time, n)
    s = _system(n_time, J, K)
    f_d = _lib.dev(c["flux"][3.0])
    g = c["g_d"].clone()
    g[1] = g[0]
    g[n - 1] = g[0]

    def run(grid):
        m = int(grid.shape[0])
        cand = torch.empty((m, J), dtype=torch.float64, device=g.device)
        coef = torch.empty((m, J, K), dtype=torch.float64, device=g.device)
        out = _lin(f_d, grid, s, cand_out=cand, coef_out=coef)
        return [v.cpu().numpy() for v in (out, cand, coef)]
    whole = run(g)
    for v in whole:
        assert v[0].tobytes() == v[1].tobytes() == v[n - 1].tobytes()
    assert whole[0][0] > 0
    for m in (1, 2):
        for v, w in zip(run(g[:m].clone()), whole):
            assert v.tobytes() == w[:m].tobytes()
    pad = torch.empty(n * n_time + 1, dtype=torch.float64, device=g.device)
    pad[1:] = g.reshape(-1)
    off = pad[1:].view(n, n_time)
    assert off.data_ptr() % 16 == 8
    for again in (off, g):
        for v, w in zip(run(again), whole):
            assert v.tobytes() == w.tobytes()
    # the other rows are those of the unchanged grid
    plain = run(c["g_d"])
    for v, w in zip(plain, whole):
        assert np.array_equal(v[2:n - 1], w[2:n - 1])


@pytest.mark.parametrize("n_time, n, J, K", [(64, 257, 2, 1), (64, 257, 8, 4), (333, 257, 5, 2), (2049, 257, 8, 4), CAPPED[0]])
def test_accumulates_onto_finite_inf_and_nan(n_time, n, J, K):
    c = _case(n_time, n)
    s = _system(n_time, J, K)
    f_d = _lib.dev(c["flux"][3.0])
    h = _lin(f_d, c["g_d"], s).cpu().numpy()
    out0 = np.random.default_rng(n_time).uniform(0.0, 50.0, n)
    out0[::5] = np.inf
    out0[1::7] = np.nan
    fin = np.isfinite(out0)
    cand = torch.empty((n, J), dtype=torch.float64, device=f_d.device)
    coef = torch.empty((n, J, K), dtype=torch.float64, device=f_d.device)
    acc = _lin(f_d, c["g_d"], s, out=_lib.dev(out0).clone(), cand_out=cand, coef_out=coef).cpu().numpy()
    assert np.array_equal(acc[fin], out0[fin] + h[fin])
    assert np.array_equal(np.isposinf(acc), np.isposinf(out0)) and np.array_equal(np.isnan(acc), np.isnan(out0))
    free, free_c = torch.empty_like(cand), torch.empty_like(coef)
    _lin(f_d, c["g_d"], s, cand_out=free, coef_out=free_c)
    assert torch.equal(cand, free) and torch.equal(coef, free_c)     # (neither is accumulated)
    # with a rule of its own: +inf from either side
    sec = np.linspace(0.0, 1.0, n)
    acc = _lin(f_d, c["g_d"], s, secdepth=_lib.dev(sec), sec_limit=0.5, out=_lib.dev(out0).clone()).cpu().numpy()
    assert np.array_equal(np.isposinf(acc), (np.isposinf(out0) | (sec >= 0.5)) & ~np.isnan(out0))


@pytest.mark.parametrize("J, K", [(1, 2), (2, 1), (8, 4)])
@pytest.mark.parametrize("n_time", [65, 315, 2049])
def test_secondary_rule_is_the_weighted_kernels(n_time, J, K):
    c = _case(n_time, 257)
    s = _system(n_time, J, K)
    f_d = _lib.dev(c["flux"][3.0])
    rng = np.random.default_rng(n_time)
    sec = rng.uniform(0.0, 1.0, 257)
    sec[:7] = np.nan
    sec[7] = 0.5                                                   # equality excludes
    excluded = sec >= 0.5                                          # (false for NaN)
    assert excluded[7] and not excluded[:7].any() and 0 < excluded.sum() < 257
    sec_d = _lib.dev(sec)
    w_d = _lib.dev(1.0 / s["d"].flux_err ** 2)
    for g in (c["g_d"], c["g_off"]):
        cand = torch.empty((257, J), dtype=torch.float64, device=g.device)
        got = _lin(f_d, g, s, secdepth=sec_d, sec_limit=0.5, cand_out=cand).cpu().numpy()
        want = _lib.chi2_grid_weighted(f_d, w_d, g, sec_d, 0.5).cpu().numpy()
        assert np.array_equal(np.isposinf(got), excluded) and np.array_equal(np.isposinf(got), np.isposinf(want))
        assert not np.isnan(got).any()
        cand_free = torch.empty_like(cand)
        free = _lin(f_d, g, s, cand_out=cand_free).cpu().numpy()
        assert np.array_equal(got[~excluded], free[~excluded])
        assert torch.equal(cand, cand_free) and bool(torch.isfinite(cand).all())          # (the rule leaves cand_out alone)
        assert np.array_equal(_lin(f_d, g, s, secdepth=sec_d, sec_limit=INF).cpu().numpy(), free)


@pytest.mark.parametrize("J, K", [(1, 1), (3, 2), (8, 4)])
@pytest.mark.parametrize("n_time", [1, 2, 65, 129, 333, 2049])
def test_a_nan_in_a_row_is_a_nan_row_and_no_other(n_time, J, K):
    n = 257
    c = _case(n_time, n)
    s = _system(n_time, J, K)
    f_d = _lib.dev(c["flux"][3.0])
    spots = sorted({0, n_time - 1, n_time // 2, min(127, n_time - 1), min(128, n_time - 1), (n_time - 1) & ~1})
    rows = [3 + 11 * i for i in range(len(spots))]
    clean = _lin(f_d, c["g_d"], s).cpu().numpy()
    g = c["g_d"].clone()
    for r, t in zip(rows, spots):
        g[r, t] = float("nan")
    got = _lin(f_d, g, s).cpu().numpy()
    hit = np.zeros(n, dtype=bool)
    hit[rows] = True
    assert np.isnan(got[hit]).all() and np.array_equal(got[~hit], clean[~hit])
    acc = _lin(f_d, g, s, out=torch.ones(n, dtype=torch.float64, device=g.device)).cpu().numpy()
    assert np.isnan(acc[hit]).all() and np.array_equal(acc[~hit], 1.0 + clean[~hit])


def test_arguments_and_empty_grid():
    c = _case(63, 3)
    s = _system(63, 3, 2)
    f_d = _lib.dev(c["flux"][0.0])
    w, B, minv, lnc = s["w_d"], s["B_d"], s["sys"].minv, s["sys"].lnc
    call = _lib.chi2_grid_white_baseline
    assert _lin(f_d, c["g_d"][:0], s).shape == (0,)
    assert _lin(f_d, c["g_d"][:0], s, cand_out=torch.empty((0, 3), dtype=torch.float64, device=w.device),
                coef_out=torch.empty((0, 3, 2), dtype=torch.float64, device=w.device)).shape == (0,)
    with pytest.raises(AssertionError):
        call(f_d, c["g_d"], w[:, :5].contiguous(), B, minv, lnc)                     # weights of another length
    with pytest.raises(AssertionError):
        call(f_d, c["g_d"], w, B[:, :5].contiguous(), minv, lnc)                     # columns of another length
    with pytest.raises(AssertionError):
        call(f_d, c["g_d"], w[:2].contiguous(), B, minv, lnc)                        # ... of another J
    with pytest.raises(AssertionError):
        call(f_d, c["g_d"], w, B, minv[:, :2], lnc)                                  # minv of another K
    with pytest.raises(AssertionError):
        call(f_d, c["g_d"], w, B, minv, lnc, coef_out=torch.empty((3, 3), dtype=torch.float64, device=w.device))
    with pytest.raises(AssertionError):
        call(f_d, c["g_d"], w, torch.ones((5, 63), dtype=torch.float64, device=w.device), np.zeros((3, 15)), lnc)
    for bad in (float("nan"), INF):
        x = lnc.copy()
        x[1] = bad
        with pytest.raises(Exception, match="lnc"):
            call(f_d, c["g_d"], w, B, minv, x)
    x = minv.copy()
    x[2, 1] = float("nan")
    with pytest.raises(Exception, match="minv"):
        call(f_d, c["g_d"], w, B, x, lnc)


def test_zz_report_the_largest_ratio():
    """(runs last in the file: the figures DESIGN.md section 14 and the README quote; measured on one MI355X: T 1.3e-4 of its
    bar, the candidates against their own baseline reductions 2.6e-4 of the two bars, the coefficients 3.3e-4)"""
    print("chi2_white_lin_kernel: largest |d T| / bar over the file %.3g; cand_out against chi2_grid_baseline %.3g of the "
          "two bars, coef_out %.3g" % (_worst["t"], _worst["h"], _worst["coef"]))
    assert 0.0 < _worst["t"] <= 1.0 and _worst["h"] <= 1.0 and _worst["coef"] <= 1.0
    assert math.isfinite(_worst["t"])
