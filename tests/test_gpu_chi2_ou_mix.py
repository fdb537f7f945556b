"""ou_mix_kernel<ONE, J> (trxm_chi2_grid_ou_mix, include/trx_mix.h): the row reduction of a model grid
under correlated noise whose amplitude and time scale are marginalised over J candidates,
    h_j = chi2_grid_ou with candidate j's tables,  T = -ln sum_j exp(lnc_j - h_j)   (clamped at 0).

Two yardsticks:
  cand_out[:, j] is _lib.chi2_grid_ou with candidate j's tables, bit for bit -- every j, shape and alignment;
  out against _numerics.ou_mix_halfchi2 in np.longdouble on the downloaded grid and the same tables.  Bar, not chosen from
  results:  |d T| <= max_j row_bar(y, alpha_j, omega_j) + 8 eps (1 + |T| + max|lnc|): the soft minimum is 1-Lipschitz in the
  a_j = h_j - lnc_j, row_bar is the bound of one candidate's h (tests/test_gpu_chi2_ou.py), and the rest is the rounding of
  a_j, m - a_j, exp, the sum, log and the last difference (each at most an eps of |T| + |lnc| + ln J or of 1).
Shapes: test_gpu_chi2_ou.py's -- one stamp, one pair, both sides of a lane's last pair (63, 64, 65) and of one trip (128,
129: ONE and not), odd lengths, many trips (2049) --, odd row counts, J = 1, 2, 3 (tables in registers), 8 (in LDS where a
row is one trip), and (CAPPED) more rows than the capped grid of 512 blocks has waves at J = 3.  The candidates' log-weights
come twice: those of datasets.ou_mix_system (one candidate usually dominates) and a set that balances the candidates at
row 0 (every term of the sum counts).
Measured (one MI355X): the largest |d T| / bar of the whole file, printed by the last test, is 2.4e-4."""
import numpy as np
import pytest
import torch

from test_datasets_red_noise_api import PAIRS, SIGMA, row_bar
from test_gpu_chi2_ou import LEVELS, _case
from triceratops_amd import _lib, _numerics, synth
from triceratops_amd import datasets as D

pytestmark = pytest.mark.gpu

N_TIMES = [1, 2, 63, 64, 65, 128, 129, 333, 2049]
NS = [1, 3, 257]
JS = [1, 2, 3, 8]
CAPPED = (65, 8195)                          # (n_time, n) at J = 3: 4 x 512 waves, two rows each
MIX_BLOCKS_MAX = 512
# (s_r / sigma, tau / cadence): test_gpu_chi2_ou.py's six -- phi == 0 and phi == 1 among them -- and two more
CANDS = PAIRS + [(3.0, 1e-6), (3.0, float("inf")), (1.0, 30.0), (0.3, 300.0)]
WEIGHTS = [0.2, 0.05, 0.1, 0.25, 0.1, 0.1, 0.15, 0.05]
# eight candidates a part in a thousand apart: their h differ by far less than the 55 between exp's underflow and 800
CLOSE = [(1.0 + 1e-3 * k, 10.0 - 1e-2 * k) for k in range(8)]
INF = float("inf")
EPS = np.finfo(np.float64).eps
LD = np.longdouble
_systems, _refs = {}, {}
_worst = {"t": 0.0}


def _system(n_time, J, cands=CANDS):
    """the light curve's stamps and errors (one per n_time, those of test_gpu_chi2_ou.py) with the first J candidates as
    its red_grid: tables and log-weights on the host and on the device"""
    key = (n_time, J, cands is CANDS)
    if key not in _systems:
        rng = np.random.default_rng(synth.SEED + 104729 * n_time)
        t = np.cumsum(rng.uniform(0.3, 1.7, n_time))
        err = SIGMA * rng.uniform(0.6, 1.8, n_time)
        grid = [(r * SIGMA, tau, w) for (r, tau), w in zip(cands[:J], WEIGHTS)]
        d = D.validate([{"time": t, "flux": np.ones(n_time), "flux_err": err, "red_grid": grid}])[0]
        alpha, beta, omega, lnc = D.ou_mix_system(d)
        _systems[key] = dict(d=d, abw=(alpha, beta, omega), lnc=lnc, abw_d=tuple(_lib.dev(v) for v in (alpha, beta, omega)))
    return _systems[key]


def _reference(n_time, n, level):
    """per candidate of the eight: the long-double h [n] and the row bar, and chi2_grid_ou's h on the device"""
    key = (n_time, n, level)
    if key not in _refs:
        c = _case(n_time, n)
        s = _system(n_time, 8)
        y = c["flux"][level][None, :] - c["g"]
        f_d = _lib.dev(c["flux"][level])
        alpha, beta, omega = s["abw"]
        h = np.stack([_numerics.ou_halfchi2(y, alpha[j], beta[j], omega[j], dtype=LD) for j in range(8)], axis=-1)
        bars = np.stack([row_bar(y, alpha[j], omega[j]) for j in range(8)], axis=-1)
        one = torch.stack([_lib.chi2_grid_ou(f_d, c["g_d"], *(v[j].contiguous() for v in s["abw_d"])) for j in range(8)], dim=1)
        _refs[key] = dict(h=h, bars=bars, one=one.contiguous(), f_d=f_d)
    return _refs[key]


def _soft_min(h, lnc):
    """the long-double statement from the candidates' long-double h [n][J]"""
    a = h - np.asarray(lnc, dtype=LD)
    m = a.min(axis=-1)
    s = np.zeros(m.shape, dtype=LD)
    for j in range(a.shape[-1]):
        s = s + np.exp(m - a[..., j])
    return np.maximum(m - np.log(s), LD(0.0))


def _mix(f_d, g, s, lnc=None, **kw):
    return _lib.chi2_grid_ou_mix(f_d, g, *s["abw_d"], s["lnc"] if lnc is None else lnc, **kw)


def _check(n_time, n, Js, levels):
    c = _case(n_time, n)
    for level in levels:
        ref = _reference(n_time, n, level)
        f_d = ref["f_d"]
        for J in Js:
            s = _system(n_time, J)
            # the eight-candidate system's first J tables are this system's
            assert all(np.array_equal(a, b[:J]) for a, b in zip(s["abw"], _system(n_time, 8)["abw"]))
            balanced = np.asarray(ref["h"][0, :J] - ref["h"][0, :J].min(), dtype=np.float64) - np.log(J)
            for name, lnc in (("system", s["lnc"]), ("balanced", balanced)):
                cand = torch.full((n, J), -1.0, dtype=torch.float64, device=f_d.device)
                got = _mix(f_d, c["g_d"], s, lnc, cand_out=cand)
                assert torch.equal(cand, ref["one"][:, :J]), "cand_out is not chi2_grid_ou's"
                want = _soft_min(ref["h"][:, :J], lnc)
                g = got.cpu().numpy()
                bar = ref["bars"][:, :J].max(axis=-1) + 8 * EPS * (1.0 + np.abs(np.asarray(want, dtype=np.float64))
                                                                  + np.abs(lnc).max())
                ratio = float((np.abs(g.astype(LD) - want).astype(np.float64) / bar).max())
                _worst["t"] = max(_worst["t"], ratio)
                print("n_time %d n %d J %d level %g sigma, lnc %s (max |lnc| %.3g): |d T| / bar %.3g (largest so far %.3g)"
                      % (n_time, n, J, level, name, np.abs(lnc).max(), ratio, _worst["t"]))
                assert ratio <= 1.0
                assert (g >= 0.0).all()
                # against the float64 statement of _numerics, to the same bar
                y = c["flux"][level][None, :] - c["g"]
                host = _numerics.ou_mix_halfchi2(y, *s["abw"], lnc)
                assert (np.abs(g - host) <= 2 * bar).all()
                # rows one double off their 16-byte boundary: the same bits, candidates included; and again: the same bits
                cand2 = torch.empty_like(cand)
                assert torch.equal(_mix(f_d, c["g_off"], s, lnc, cand_out=cand2), got) and torch.equal(cand2, cand)
                assert torch.equal(_mix(f_d, c["g_d"], s, lnc), got)               # (without cand_out)


@pytest.mark.parametrize("n_time, n", [(t, n) for n in NS for t in N_TIMES])
def test_mix_matches_the_candidates_in_bits_and_the_longdouble_statement(n_time, n):
    _check(n_time, n, JS, LEVELS)


def test_mix_past_the_capped_grid():
    n_time, n = CAPPED
    assert 4 * MIX_BLOCKS_MAX * 2 < n
    _check(n_time, n, (3,), (3.0,))


@pytest.mark.parametrize("n_time, n", [(1, 3), (64, 257), (65, 257), (129, 3), (333, 257), (2049, 257)])
def test_one_candidate_at_lnc_zero_is_chi2_grid_ou_in_bits(n_time, n):
    c = _case(n_time, n)
    s = _system(n_time, 1)
    assert s["lnc"].tolist() == [0.0]
    sec = _lib.dev(np.linspace(0.0, 1.0, n))
    for level in LEVELS:
        f_d = _lib.dev(c["flux"][level])
        for g in (c["g_d"], c["g_off"]):
            one = _lib.chi2_grid_ou(f_d, g, *(v[0] for v in s["abw_d"]))
            assert torch.equal(_mix(f_d, g, s), one)
            assert torch.equal(_mix(f_d, g, s, secdepth=sec, sec_limit=0.5),
                               _lib.chi2_grid_ou(f_d, g, *(v[0] for v in s["abw_d"]), sec, 0.5))
            acc = torch.full((n,), 2.5, dtype=torch.float64, device=g.device)
            assert torch.equal(_mix(f_d, g, s, out=acc.clone()),
                               _lib.chi2_grid_ou(f_d, g, *(v[0] for v in s["abw_d"]), out=acc.clone()))


@pytest.mark.parametrize("J", [2, 3, 8])
@pytest.mark.parametrize("n_time, n", [(2, 3), (65, 257), (128, 257), (129, 257), (2049, 3)])
def test_candidates_at_minus_800_do_not_reach_the_sum(n_time, n, J):
    """one candidate at lnc = 0, the others at -800: exp underflows to 0, the sum is 1, out has that candidate's bits
    (on candidates whose h lie close together: one that is 800 below another would take the minimum itself)"""
    c = _case(n_time, n)
    s = _system(n_time, J, CLOSE)
    f_d = _lib.dev(c["flux"][3.0])
    for g in (c["g_d"], c["g_off"]):
        one = torch.stack([_lib.chi2_grid_ou(f_d, g, *(v[j] for v in s["abw_d"])) for j in range(J)], dim=1)
        assert float((one.max(dim=1).values - one.min(dim=1).values).max().cpu()) < 40.0
        for keep in sorted({0, J // 2, J - 1}):
            lnc = np.full(J, -800.0)
            lnc[keep] = 0.0
            assert torch.equal(_mix(f_d, g, s, lnc), one[:, keep].contiguous())
            lnc[lnc < 0] = -INF                                               # (switched off altogether)
            assert torch.equal(_mix(f_d, g, s, lnc), one[:, keep].contiguous())


@pytest.mark.parametrize("J", [2, 3, 8])
@pytest.mark.parametrize("n_time, n", [(65, 257), (128, 3), (333, 257), (2049, 3)])
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
        tables = tuple(v.index_select(0, p_d).contiguous() for v in s["abw_d"])
        cand_p = torch.empty_like(cand)
        got_p = _lib.chi2_grid_ou_mix(ref["f_d"], c["g_d"], *tables, lnc[perm], cand_out=cand_p).cpu().numpy()
        assert torch.equal(cand_p, cand.index_select(1, p_d))
        bar = 8 * EPS * (1.0 + np.abs(got) + np.abs(lnc).max())
        assert (np.abs(got_p - got) <= bar).all(), float((np.abs(got_p - got) / bar).max())


@pytest.mark.parametrize("n_time, n, J", [(65, 257, 3), (65, 257, 8), (2049, 257, 3), (2049, 257, 8), CAPPED + (3,)])
def test_a_rows_bits_are_its_own(n_time, n, J):
    """the same row at position 0, 1 and n - 1 (behind the capped grid where n says so), in a launch of its own, in a view
    one double off, and on a second run"""
    c = _case(n_time, n)
    s = _system(n_time, J)
    f_d = _lib.dev(c["flux"][3.0])
    ref = _reference(n_time, n, 3.0)
    lnc = np.asarray(ref["h"][0, :J] - ref["h"][0, :J].min(), dtype=np.float64) - np.log(J)
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


@pytest.mark.parametrize("n_time, n, J", [(64, 257, 2), (64, 257, 8), (333, 257, 2), (333, 257, 8), (2049, 257, 8),
                                          CAPPED + (3,)])
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
    acc = _mix(f_d, c["g_d"], s, out=_lib.dev(out0).clone()).cpu().numpy()
    assert np.array_equal(acc[fin], out0[fin] + h[fin])
    assert np.array_equal(np.isposinf(acc), np.isposinf(out0)) and np.array_equal(np.isnan(acc), np.isnan(out0))
    # with a rule of its own: +inf from either side
    sec = np.linspace(0.0, 1.0, n)
    acc = _mix(f_d, c["g_d"], s, secdepth=_lib.dev(sec), sec_limit=0.5, out=_lib.dev(out0).clone()).cpu().numpy()
    assert np.array_equal(np.isposinf(acc), (np.isposinf(out0) | (sec >= 0.5)) & ~np.isnan(out0))


@pytest.mark.parametrize("J", [2, 8])
@pytest.mark.parametrize("n_time", [65, 2049])
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
@pytest.mark.parametrize("n_time", [1, 2, 65, 129, 333, 2049])
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
    a, b, w = s["abw_d"]
    assert _mix(f_d, c["g_d"][:0], s).shape == (0,)
    assert _mix(f_d, c["g_d"][:0], s, cand_out=torch.empty((0, 3), dtype=torch.float64, device=a.device)).shape == (0,)
    with pytest.raises(AssertionError):
        _lib.chi2_grid_ou_mix(f_d, c["g_d"], a[:, :5].contiguous(), b, w, s["lnc"])        # a table of another length
    with pytest.raises(AssertionError):
        _lib.chi2_grid_ou_mix(f_d, c["g_d"], a[:2].contiguous(), b, w, s["lnc"])           # ... of another J
    with pytest.raises(AssertionError):
        _lib.chi2_grid_ou_mix(f_d, c["g_d"], a, b, w, s["lnc"][:2])
    with pytest.raises(AssertionError):
        _lib.chi2_grid_ou_mix(f_d, c["g_d"], a, b, w, s["lnc"],
                              cand_out=torch.empty((3, 2), dtype=torch.float64, device=a.device))
    with pytest.raises(AssertionError):
        _lib.chi2_grid_ou_mix(f_d[:5], c["g_d"], a, b, w, s["lnc"])
    # the library refuses a NaN or +inf log-weight before it enqueues anything
    for bad in (float("nan"), INF):
        lnc = s["lnc"].copy()
        lnc[1] = bad
        with pytest.raises(Exception, match="lnc"):
            _lib.chi2_grid_ou_mix(f_d, c["g_d"], a, b, w, lnc)


def test_zz_report_the_largest_ratio():
    """(runs last in the file: the figure DESIGN.md section 14 quotes)"""
    print("ou_mix_kernel against np.longdouble: largest |d T| / bar over the file %.3g" % _worst["t"])
    assert 0.0 < _worst["t"] <= 1.0
