"""chi2_white_mix_kernel<STAGE, J> (trxv_chi2_grid_white_mix, include/trx_mix.h): the row reduction of
a model grid under white noise whose size -- an error scale k and a jitter s -- is marginalised over J candidates,
    h_j = chi2_grid_weighted with inv_var = w_j,  w_j[t] = 1 / (k_j^2 sigma_t^2 + s_j^2),
    T = -ln sum_j exp(lnc_j - h_j)   (clamped at 0).

Two yardsticks:
  cand_out[:, j] is _lib.chi2_grid_weighted with w_j, bit for bit -- every j, shape and alignment --, and so is out at J = 1,
  lnc = 0;
  out against _numerics.white_mix_halfchi2 in np.longdouble on the downloaded grid and the same tables.  Bar, written before
  the first run:  |d T| <= max_j (1e-12 h_j + 1e-12) + 16 eps (1 + |T| + max|lnc|): the soft minimum is 1-Lipschitz in the h_j,
  the first part is the plain weighted reduction's bar (tests/test_gpu_chi2_offset.py), the second the soft minimum's
  (tests/test_gpu_softmin_rows.py).
Shapes: one stamp, one pair, an odd three, both sides of a lane's last pair (63, 64, 65) and of the second (127, 128, 129),
an odd length with several trips (333), the stage limit and one past it for J = 2 (1364, 1365) and J = 8 (454, 455), past
every stage limit (2049); n = 1, 2, 3, 257; J = 1, 2, 3, 5, 8; residuals at 0, 3 and 100 sigma; scales 0.5 ... 3, jitters
0 ... 3 sigma; and one CAPPED case per staging mode with more rows than the capped grid has wave slots
(_lib.white_mix_blocks).  The candidates' log-weights come twice: those of datasets.white_mix_system (one candidate
usually dominates) and a set that balances the candidates at row 0 (every term of the sum counts).
Measured (one MI355X): the largest |d T| / bar of the whole file, printed by the last test, is 3e-4."""
import numpy as np
import pytest
import torch

from test_gpu_chi2_ou import LEVELS, SIGMA, _case
from triceratops_amd import _lib, _numerics, synth
from triceratops_amd import datasets as D

pytestmark = pytest.mark.gpu

N_TIMES = [1, 2, 3, 63, 64, 65, 127, 128, 129, 333, 454, 455, 1364, 1365, 2049]
NS = [1, 2, 3, 257]
JS = [1, 2, 3, 5, 8]
# (n_time, n, J): staged (4 x 66 doubles a block: 8 blocks a CU) and not (455 stamps at J = 8 are past the stage limit)
CAPPED = [(65, 16387, 3), (455, 16387, 8)]
# (k, s / sigma, prior weight)
CANDS = [(1.0, 0.0, 0.2), (0.5, 0.0, 0.05), (2.0, 1.0, 0.1), (3.0, 0.0, 0.25), (1.5, 3.0, 0.1), (1.0, 0.5, 0.1),
         (2.5, 2.0, 0.15), (0.75, 0.1, 0.05)]
# eight candidates a part in 10^5 apart: their h (up to 3e4 here) differ by far less than the 55 between exp's underflow
# and 800
CLOSE = [(1.0 + 1e-5 * k, 1e-3 * k, 1.0) for k in range(8)]
INF = float("inf")
EPS = np.finfo(np.float64).eps
LD = np.longdouble
_systems, _refs = {}, {}
_worst = {"t": 0.0}


def _system(n_time, J, cands=CANDS):
    """the light curve's errors (one set per n_time, those of test_gpu_chi2_ou.py) with the first J candidates as its
    white_grid: weights and log-weights on the host and on the device"""
    key = (n_time, J, cands is CANDS)
    if key not in _systems:
        rng = np.random.default_rng(synth.SEED + 104729 * n_time)
        t = rng.uniform(-0.2, 0.2, n_time)                               # (folded: no order)
        err = SIGMA * rng.uniform(0.6, 1.8, n_time)
        dicts = [{"time": t, "flux": np.ones(n_time), "flux_err": err,
                  "white_grid": [(k, s * SIGMA, w) for k, s, w in cands[:J]]}]
        sets = D.validate(dicts)
        w, lnc = D.white_mix_system(sets[0], D.white_grids(dicts, sets)[0])
        _systems[key] = dict(d=sets[0], w=w, lnc=lnc, w_d=_lib.dev(w))
    return _systems[key]


def _reference(n_time, n, level, rows=None):
    """per candidate of the eight: the long-double h of the rows asked for (None: all), and chi2_grid_weighted's h of every
    row on the device"""
    key = (n_time, n, level)
    if key not in _refs:
        c = _case(n_time, n)
        s = _system(n_time, 8)
        sel = slice(None) if rows is None else rows
        y = (c["flux"][level][None, :] - c["g"][sel]).astype(LD)
        f_d = _lib.dev(c["flux"][level])
        h = np.stack([LD(0.5) * np.sum(s["w"][j].astype(LD) * y * y, axis=-1) for j in range(8)], axis=-1)
        one = torch.stack([_lib.chi2_grid_weighted(f_d, s["w_d"][j], c["g_d"]) for j in range(8)], dim=1)
        _refs[key] = dict(h=h, one=one.contiguous(), f_d=f_d, sel=sel)
    return _refs[key]


def _soft_min(h, lnc):
    """the long-double statement from the candidates' long-double h [n][J]"""
    a = h - np.asarray(lnc, dtype=LD)
    m = a.min(axis=-1)
    s = np.zeros(m.shape, dtype=LD)
    for j in range(a.shape[-1]):
        s = s + np.exp(m - a[..., j])
    return np.maximum(m - np.log(s), LD(0.0))


def _bar(h, want, lnc):
    h = np.asarray(h, dtype=np.float64)
    return (1e-12 * h + 1e-12).max(axis=-1) + 16 * EPS * (1.0 + np.abs(np.asarray(want, dtype=np.float64)) + np.abs(lnc).max())


def _mix(f_d, g, s, lnc=None, **kw):
    return _lib.chi2_grid_white_mix(f_d, g, s["w_d"], s["lnc"] if lnc is None else lnc, **kw)


def _check(n_time, n, Js, levels, rows=None):
    c = _case(n_time, n)
    for level in levels:
        ref = _reference(n_time, n, level, rows)
        f_d, sel = ref["f_d"], ref["sel"]
        for J in Js:
            s = _system(n_time, J)
            # the eight-candidate system's first J weight vectors are this system's
            assert np.array_equal(s["w"], _system(n_time, 8)["w"][:J])
            balanced = np.asarray(ref["h"][0, :J] - ref["h"][0, :J].min(), dtype=np.float64) - np.log(J)
            for name, lnc in (("system", s["lnc"]), ("balanced", balanced)):
                cand = torch.full((n, J), -1.0, dtype=torch.float64, device=f_d.device)
                got = _mix(f_d, c["g_d"], s, lnc, cand_out=cand)
                assert torch.equal(cand, ref["one"][:, :J]), "cand_out is not chi2_grid_weighted's"
                want = _soft_min(ref["h"][:, :J], lnc)
                g = got.cpu().numpy()
                bar = _bar(ref["h"][:, :J], want, lnc)
                ratio = float((np.abs(g[sel].astype(LD) - want).astype(np.float64) / bar).max())
                _worst["t"] = max(_worst["t"], ratio)
                print("n_time %d n %d J %d level %g sigma, lnc %s (max |lnc| %.3g): |d T| / bar %.3g (largest so far %.3g)"
                      % (n_time, n, J, level, name, np.abs(lnc).max(), ratio, _worst["t"]))
                assert ratio <= 1.0
                assert (g >= 0.0).all()
                # the statement of _numerics itself, in long double, is what `want` is
                if n <= 3:
                    y = c["flux"][level][None, :] - c["g"]
                    host = _numerics.white_mix_halfchi2(y, s["w"], lnc, dtype=LD)
                    assert host.dtype == LD and np.array_equal(host, want)
                # rows one double off their 16-byte boundary: the same bits, candidates included; and again: the same bits
                cand2 = torch.empty_like(cand)
                assert torch.equal(_mix(f_d, c["g_off"], s, lnc, cand_out=cand2), got) and torch.equal(cand2, cand)
                assert torch.equal(_mix(f_d, c["g_d"], s, lnc), got)               # (without cand_out)


@pytest.mark.parametrize("n_time, n", [(t, n) for n in NS for t in N_TIMES])
def test_mix_matches_the_candidates_in_bits_and_the_longdouble_statement(n_time, n):
    _check(n_time, n, JS, LEVELS)


@pytest.mark.parametrize("n_time, n, J", CAPPED)
def test_mix_past_the_capped_grid(n_time, n, J):
    blocks = _lib.white_mix_blocks(n, n_time, J)
    assert 4 * blocks * 2 < n                                        # (every wave two rows a pass, and a further pass)
    staged = n_time <= (((2 * 2048) // (1 + J)) & ~1)
    assert staged == (n_time == 65)
    rows = np.unique(np.concatenate([np.arange(64), np.arange(n - 64, n), 4 * blocks + np.arange(-8, 8),
                                     8 * blocks + np.arange(-8, 3),
                                     np.random.default_rng(n_time).integers(0, n, 256)]))
    assert rows.max() == n - 1 and (rows > 8 * blocks).any()
    _check(n_time, n, (J,), (3.0,), rows)


def test_stage_limits_are_the_launchers():
    # (what the shapes above straddle: one block more a CU past the limit, none of it LDS)
    assert _lib.white_mix_blocks(10 ** 6, 1364, 2) == 1280 and _lib.white_mix_blocks(10 ** 6, 1365, 2) == 2048
    assert _lib.white_mix_blocks(10 ** 6, 454, 8) == 1280 and _lib.white_mix_blocks(10 ** 6, 455, 8) == 2048
    assert _lib.white_mix_blocks(10 ** 6, 2048, 1) == 1280 and _lib.white_mix_blocks(10 ** 6, 2049, 1) == 2048


@pytest.mark.parametrize("n_time, n", [(1, 3), (64, 257), (65, 257), (129, 3), (333, 257), (2048, 3), (2049, 257)])
def test_one_candidate_at_lnc_zero_is_chi2_grid_weighted_in_bits(n_time, n):
    c = _case(n_time, n)
    s = _system(n_time, 1)
    assert s["lnc"].tolist() == [0.0]
    assert np.array_equal(s["w"][0], 1.0 / (s["d"].flux_err * s["d"].flux_err))
    sec = _lib.dev(np.linspace(0.0, 1.0, n))
    for j in (0, 4):                                                 # (the unit candidate, and k = 1.5 with a 3 sigma jitter)
        w_d = _system(n_time, 8)["w_d"][j].contiguous()
        one_w = w_d[None, :].contiguous()
        for level in LEVELS:
            f_d = _lib.dev(c["flux"][level])
            for g in (c["g_d"], c["g_off"]):
                mix = lambda **kw: _lib.chi2_grid_white_mix(f_d, g, one_w, np.zeros(1), **kw)      # noqa: E731
                assert torch.equal(mix(), _lib.chi2_grid_weighted(f_d, w_d, g))
                assert torch.equal(mix(secdepth=sec, sec_limit=0.5), _lib.chi2_grid_weighted(f_d, w_d, g, sec, 0.5))
                acc = torch.full((n,), 2.5, dtype=torch.float64, device=g.device)
                assert torch.equal(mix(out=acc.clone()), _lib.chi2_grid_weighted(f_d, w_d, g, out=acc.clone()))


@pytest.mark.parametrize("n_time, n", [(1, 3), (3, 257), (65, 257), (2048, 3), (2049, 257)])
def test_one_candidate_with_a_log_weight(n_time, n):
    """J = 1 takes no exp and no log: T = max(h - lnc, 0) against the long-double statement, a weight that drives short rows
    below 0, and -inf"""
    c = _case(n_time, n)
    s = _system(n_time, 1)
    for level in LEVELS:
        ref = _reference(n_time, n, level)
        for lnc in (np.array([-2.5]), np.array([3.0]), np.array([float(np.asarray(ref["h"][:, 0], dtype=np.float64).mean())])):
            cand = torch.empty((n, 1), dtype=torch.float64, device=ref["f_d"].device)
            got = _mix(ref["f_d"], c["g_d"], s, lnc, cand_out=cand)
            assert torch.equal(cand, ref["one"][:, :1])
            want = _soft_min(ref["h"][:, :1], lnc)
            g = got.cpu().numpy()
            assert (np.abs(g.astype(LD) - want).astype(np.float64) <= _bar(ref["h"][:, :1], want, lnc)).all() and (g >= 0).all()
            assert torch.equal(_mix(ref["f_d"], c["g_off"], s, lnc), got)
        assert bool(torch.isposinf(_mix(ref["f_d"], c["g_d"], s, np.array([-INF]))).all())


@pytest.mark.parametrize("J", [2, 3, 8])
@pytest.mark.parametrize("n_time, n", [(2, 3), (65, 257), (128, 257), (455, 257), (2049, 3)])
def test_candidates_at_minus_800_or_switched_off_do_not_reach_the_sum(n_time, n, J):
    """one candidate at lnc = 0, the others at -800: exp underflows to 0, the sum is 1, out has that candidate's bits
    (on candidates whose h lie close together: one that is 800 below another would take the minimum itself); then at -inf:
    switched off altogether"""
    c = _case(n_time, n)
    s = _system(n_time, J, CLOSE)
    f_d = _lib.dev(c["flux"][3.0])
    for g in (c["g_d"], c["g_off"]):
        one = torch.stack([_lib.chi2_grid_weighted(f_d, s["w_d"][j], g) for j in range(J)], dim=1)
        assert float((one.max(dim=1).values - one.min(dim=1).values).max().cpu()) < 40.0
        for keep in sorted({0, J // 2, J - 1}):
            lnc = np.full(J, -800.0)
            lnc[keep] = 0.0
            assert torch.equal(_mix(f_d, g, s, lnc), one[:, keep].contiguous())
            lnc[lnc < 0] = -INF
            assert torch.equal(_mix(f_d, g, s, lnc), one[:, keep].contiguous())


@pytest.mark.parametrize("J", [2, 3, 8])
@pytest.mark.parametrize("n_time, n", [(65, 257), (128, 3), (333, 257), (455, 257), (2049, 3)])
def test_permuting_the_candidates(n_time, n, J):
    c = _case(n_time, n)
    s = _system(n_time, J)
    ref = _reference(n_time, n, 3.0)
    lnc = np.asarray(ref["h"][0, :J] - ref["h"][0, :J].min(), dtype=np.float64) - np.log(J)        # (balanced at row 0)
    cand = torch.empty((n, J), dtype=torch.float64, device=ref["f_d"].device)
    got = _mix(ref["f_d"], c["g_d"], s, lnc, cand_out=cand).cpu().numpy()
    rng = np.random.default_rng(J + n_time)
    for perm in (np.arange(J)[::-1].copy(), rng.permutation(J)):
        p_d = torch.as_tensor(perm, device=cand.device)
        cand_p = torch.empty_like(cand)
        got_p = _lib.chi2_grid_white_mix(ref["f_d"], c["g_d"], s["w_d"].index_select(0, p_d).contiguous(), lnc[perm],
                                         cand_out=cand_p).cpu().numpy()
        assert torch.equal(cand_p, cand.index_select(1, p_d))
        bar = 16 * EPS * (1.0 + np.abs(got) + np.abs(lnc).max())
        assert (np.abs(got_p - got) <= bar).all(), float((np.abs(got_p - got) / bar).max())


@pytest.mark.parametrize("n_time, n, J", [(65, 257, 3), (65, 257, 8), (454, 257, 8), (455, 257, 8), (2049, 257, 3),
                                          (2049, 257, 8)] + CAPPED)
def test_a_rows_bits_are_its_own(n_time, n, J):
    """the same row at position 0, 1 and n - 1 (behind the capped grid where n says so), in a launch of its own, in a view
    one double off, and on a second run"""
    c = _case(n_time, n)
    s = _system(n_time, J)
    f_d = _lib.dev(c["flux"][3.0])
    w8 = _system(n_time, 8)["w"]
    y0 = (c["flux"][3.0] - c["g"][0]).astype(LD)
    h0 = np.array([float(LD(0.5) * np.sum(w8[j].astype(LD) * y0 * y0)) for j in range(J)])
    lnc = h0 - h0.min() - np.log(J)                                  # (balanced at row 0)
    g = c["g_d"].clone()
    g[1] = g[0]
    g[n - 1] = g[0]
    cand = torch.empty((n, J), dtype=torch.float64, device=g.device)
    got = _mix(f_d, g, s, lnc, cand_out=cand)
    h, hc = got.cpu().numpy(), cand.cpu().numpy()
    assert h[0] > 0 and h[0].tobytes() == h[1].tobytes() == h[n - 1].tobytes()
    assert hc[0].tobytes() == hc[1].tobytes() == hc[n - 1].tobytes()
    assert _mix(f_d, g[:1].clone(), s, lnc).cpu().numpy().tobytes() == h[:1].tobytes()
    assert _mix(f_d, g[:2].clone(), s, lnc).cpu().numpy().tobytes() == h[:2].tobytes()
    pad = torch.empty(n * n_time + 1, dtype=torch.float64, device=g.device)
    pad[1:] = g.reshape(-1)
    off = pad[1:].view(n, n_time)
    assert off.data_ptr() % 16 == 8
    assert torch.equal(_mix(f_d, off, s, lnc), got)
    assert torch.equal(_mix(f_d, g, s, lnc), got)
    # the other rows are those of the unchanged grid
    plain = _mix(f_d, c["g_d"], s, lnc).cpu().numpy()
    assert np.array_equal(h[2:n - 1], plain[2:n - 1])


@pytest.mark.parametrize("n_time, n, J", [(64, 257, 2), (64, 257, 8), (333, 257, 2), (333, 257, 8), (2049, 257, 8), CAPPED[0]])
def test_accumulates_onto_finite_inf_and_nan(n_time, n, J):
    c = _case(n_time, n)
    s = _system(n_time, J)
    f_d = _lib.dev(c["flux"][3.0])
    h = _mix(f_d, c["g_d"], s).cpu().numpy()
    out0 = np.random.default_rng(n_time).uniform(0.0, 50.0, n)
    out0[::5] = np.inf
    out0[1::7] = np.nan
    fin = np.isfinite(out0)
    assert fin.sum() > 100 and np.isposinf(out0).sum() > 10 and np.isnan(out0).sum() > 10
    cand = torch.empty((n, J), dtype=torch.float64, device=f_d.device)
    acc = _mix(f_d, c["g_d"], s, out=_lib.dev(out0).clone(), cand_out=cand).cpu().numpy()
    assert np.array_equal(acc[fin], out0[fin] + h[fin])
    assert np.array_equal(np.isposinf(acc), np.isposinf(out0)) and np.array_equal(np.isnan(acc), np.isnan(out0))
    free = torch.empty_like(cand)
    _mix(f_d, c["g_d"], s, cand_out=free)
    assert torch.equal(cand, free)                                   # (cand_out is not accumulated)
    # with a rule of its own: +inf from either side
    sec = np.linspace(0.0, 1.0, n)
    acc = _mix(f_d, c["g_d"], s, secdepth=_lib.dev(sec), sec_limit=0.5, out=_lib.dev(out0).clone()).cpu().numpy()
    assert np.array_equal(np.isposinf(acc), (np.isposinf(out0) | (sec >= 0.5)) & ~np.isnan(out0))


@pytest.mark.parametrize("J", [2, 8])
@pytest.mark.parametrize("n_time", [65, 455, 2049])
def test_secondary_rule_is_the_weighted_kernels(n_time, J):
    c = _case(n_time, 257)
    s = _system(n_time, J)
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
        got = _mix(f_d, g, s, secdepth=sec_d, sec_limit=0.5, cand_out=cand).cpu().numpy()
        want = _lib.chi2_grid_weighted(f_d, w_d, g, sec_d, 0.5).cpu().numpy()
        assert np.array_equal(np.isposinf(got), excluded) and np.array_equal(np.isposinf(got), np.isposinf(want))
        assert not np.isnan(got).any()
        cand_free = torch.empty_like(cand)
        free = _mix(f_d, g, s, cand_out=cand_free).cpu().numpy()
        assert np.array_equal(got[~excluded], free[~excluded])
        assert torch.equal(cand, cand_free) and bool(torch.isfinite(cand).all())          # (the rule leaves cand_out alone)
        # sec_limit = +inf: the rule is off
        assert np.array_equal(_mix(f_d, g, s, secdepth=sec_d, sec_limit=INF).cpu().numpy(), free)


@pytest.mark.parametrize("J", [1, 3, 8])
@pytest.mark.parametrize("n_time", [1, 2, 65, 129, 333, 455, 2049])
def test_a_nan_in_a_row_is_a_nan_row_and_no_other(n_time, J):
    n = 257
    c = _case(n_time, n)
    s = _system(n_time, J)
    f_d = _lib.dev(c["flux"][3.0])
    spots = sorted({0, n_time - 1, n_time // 2, min(127, n_time - 1), min(128, n_time - 1), (n_time - 1) & ~1})
    rows = [3 + 11 * i for i in range(len(spots))]
    clean = _mix(f_d, c["g_d"], s).cpu().numpy()
    g = c["g_d"].clone()
    for r, t in zip(rows, spots):
        g[r, t] = float("nan")
    got = _mix(f_d, g, s).cpu().numpy()
    hit = np.zeros(n, dtype=bool)
    hit[rows] = True
    assert np.isnan(got[hit]).all() and np.array_equal(got[~hit], clean[~hit])
    # ... also under accumulation
    acc = _mix(f_d, g, s, out=torch.ones(n, dtype=torch.float64, device=g.device)).cpu().numpy()
    assert np.isnan(acc[hit]).all() and np.array_equal(acc[~hit], 1.0 + clean[~hit])


def test_arguments_and_empty_grid():
    c = _case(63, 3)
    s = _system(63, 3)
    f_d = _lib.dev(c["flux"][0.0])
    w = s["w_d"]
    assert _mix(f_d, c["g_d"][:0], s).shape == (0,)
    assert _mix(f_d, c["g_d"][:0], s, cand_out=torch.empty((0, 3), dtype=torch.float64, device=w.device)).shape == (0,)
    with pytest.raises(AssertionError):
        _lib.chi2_grid_white_mix(f_d, c["g_d"], w[:, :5].contiguous(), s["lnc"])           # weights of another length
    with pytest.raises(AssertionError):
        _lib.chi2_grid_white_mix(f_d, c["g_d"], w[:2].contiguous(), s["lnc"])              # ... of another J
    with pytest.raises(AssertionError):
        _lib.chi2_grid_white_mix(f_d, c["g_d"], w, s["lnc"][:2])
    with pytest.raises(AssertionError):
        _lib.chi2_grid_white_mix(f_d, c["g_d"], w, s["lnc"], cand_out=torch.empty((3, 2), dtype=torch.float64, device=w.device))
    with pytest.raises(AssertionError):
        _lib.chi2_grid_white_mix(f_d[:5], c["g_d"], w, s["lnc"])
    with pytest.raises(AssertionError):
        _lib.chi2_grid_white_mix(f_d, c["g_d"], torch.ones((9, 63), dtype=torch.float64, device=w.device), np.zeros(9))
    # the library refuses a NaN or +inf log-weight before it enqueues anything
    for bad in (float("nan"), INF):
        lnc = s["lnc"].copy()
        lnc[1] = bad
        with pytest.raises(Exception, match="lnc"):
            _lib.chi2_grid_white_mix(f_d, c["g_d"], w, lnc)


def test_zz_report_the_largest_ratio():
    """(runs last in the file: the figure DESIGN.md section 14 and the README quote; measured on one MI355X: 3e-4)"""
    print("chi2_white_mix_kernel against np.longdouble: largest |d T| / bar over the file %.3g" % _worst["t"])
    assert 0.0 < _worst["t"] <= 1.0
