"""The Monte-Carlo error of a calc_probs table on the host: the delta-method propagation of
_numerics._mc_errors against brute force, and target._finish / _defer_finish with records that carry the moments of
the evidences (sharding.MOMENT_COLS) and with records that do not."""
import warnings

import numpy as np
import pytest

from triceratops_amd import sharding
from triceratops_amd._numerics import _mc_errors, _normalize_probabilities

N_SCEN = 18


def _fpp_nfpp(lnZ):
    prob, _ = _normalize_probabilities(lnZ)
    return 1 - (prob[0] + prob[3] + prob[9]), np.sum(prob[15:])


def test_propagation_matches_the_scatter_of_replicas():
    """18 synthetic scenarios of N = 4000 Gamma-distributed weights, 80 % of them zero, 3000 replicas: the std of FPP
    and NFPP across the replicas against the formula evaluated from ONE replica's (lnZ, lnM2), median over replicas"""
    rng = np.random.default_rng(20261016)
    N, R = 4000, 3000
    scale = np.exp(rng.uniform(-1.5, 1.5, N_SCEN))[:, None]
    lnZ, lnM2 = np.empty((R, N_SCEN)), np.empty((R, N_SCEN))
    for r0 in range(0, R, 250):
        w = rng.standard_gamma(1.0, (250, N_SCEN, N)) * scale
        w *= rng.random((250, N_SCEN, N)) < 0.2
        lnZ[r0:r0 + 250] = np.log(w.mean(axis=2))
        lnM2[r0:r0 + 250] = np.log((w * w).mean(axis=2))
    fpp, nfpp, e_fpp, e_nfpp = (np.empty(R) for _ in range(4))
    for r in range(R):
        fpp[r], nfpp[r] = _fpp_nfpp(lnZ[r])
        e = _mc_errors(lnZ[r], lnM2[r], N, "ok")
        e_fpp[r], e_nfpp[r] = e["FPP_err"], e["NFPP_err"]
    for name, spread, formula in (("FPP", np.std(fpp), np.median(e_fpp)), ("NFPP", np.std(nfpp), np.median(e_nfpp))):
        print("%s: std over replicas %.5g, median formula %.5g, ratio %.4f" % (name, spread, formula, formula / spread))
        assert abs(formula / spread - 1) < 0.10, name
    # and lnZ_err per scenario against the scatter of lnZ
    e = np.array([_mc_errors(lnZ[r], lnM2[r], N, "ok")["lnZ_err"] for r in range(0, R, 10)])
    assert np.all(np.abs(np.median(e, axis=0) / np.std(lnZ, axis=0) - 1) < 0.10)


def test_hand_made_cases():
    N = 1000
    # a single nonzero weight w in one scenario: mean w / N, mean square w^2 / N -> ess = 1
    lnZ = np.full(N_SCEN, -np.inf)
    lnM2 = np.full(N_SCEN, -np.inf)
    lnZ[0], lnM2[0] = np.log(3.0 / N), np.log(9.0 / N)
    e = _mc_errors(lnZ, lnM2, N, _normalize_probabilities(lnZ)[1])
    assert e["ess"][0] == pytest.approx(1.0, rel=1e-14)
    assert e["lnZ_err"][0] == pytest.approx(np.sqrt(1 - 1 / N), rel=1e-14)
    assert np.all(e["ess"][1:] == 0.0) and np.all(np.isnan(e["lnZ_err"][1:]))
    # all the evidence in A: FPP = 0 exactly, its first-order error 0
    assert e["FPP_err"] == 0.0 and e["NFPP_err"] == 0.0
    # every weight equal: ess = N, lnZ_err = 0
    lnZ2 = np.full(N_SCEN, np.log(2.0))
    e = _mc_errors(lnZ2, 2 * lnZ2, N, "ok")
    assert np.allclose(e["ess"], N, rtol=1e-14) and np.all(e["lnZ_err"] == 0.0)
    assert e["FPP_err"] == 0.0 and e["NFPP_err"] == 0.0
    # two scenarios, A = row 0 and B = row 1, equal evidences and errors: sqrt(2) Z^2 s / (2 Z)^2 = s / (2 sqrt 2)
    lnZ3 = np.full(N_SCEN, -np.inf)
    lnM3 = np.full(N_SCEN, -np.inf)
    lnZ3[:2], lnM3[:2] = -5.0, -10.0 + np.log(1 + 0.04 * N)      # 1 / ess - 1 / N = 0.04
    e = _mc_errors(lnZ3, lnM3, N, "ok")
    assert e["lnZ_err"][0] == pytest.approx(0.2, rel=1e-12)
    assert e["FPP_err"] == pytest.approx(0.2 / (2 * np.sqrt(2)), rel=1e-12)
    # nearly all the evidence in A (FPP ~ 1e-20): the other side is summed, not subtracted -- finite and >= 0
    lnZ4 = np.full(N_SCEN, -50.0)
    lnZ4[[0, 3, 9]] = 0.0
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        e = _mc_errors(lnZ4, 2 * lnZ4 + np.log(5.0), N, "ok")
    assert np.isfinite(e["FPP_err"]) and 0 < e["FPP_err"] < 1e-18
    # all -inf, and an anomaly: no error to report, no warning raised
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        e = _mc_errors(np.full(N_SCEN, -np.inf), np.full(N_SCEN, -np.inf), N, "all_neginf")
        assert np.all(e["ess"] == 0.0) and np.all(np.isnan(e["lnZ_err"]))
        assert np.isnan(e["FPP_err"]) and np.isnan(e["NFPP_err"])
        bad = lnZ2.copy()
        bad[4] = np.nan
        e = _mc_errors(bad, 2 * lnZ2, N, _normalize_probabilities(bad)[1])
        assert np.isnan(e["FPP_err"]) and np.isnan(e["NFPP_err"]) and np.isnan(e["ess"][4])
        # unknown moments (NaN lnM2) of a finite evidence: NaN errors
        e = _mc_errors(lnZ2, np.full(N_SCEN, np.nan), N, "ok")
        assert np.all(np.isnan(e["ess"])) and np.isnan(e["FPP_err"])


def _records(rng, n_cols):
    """units and run_units(as_rows=True)-style records of one 18-scenario table (10 target calls, one nearby star)"""
    from triceratops_amd.triceratops import _TARGET_CALLS
    N = 50_000
    # (first row, names, star number, ID, thunk, key, weight, N, (job, star)): the units of target._prepare
    units = [(j0, names, snum, 42, None, key, 1.0, N, (0, 0)) for key, names, j0, snum in _TARGET_CALLS]
    units += [(15, ("NTP",), 1, 43, None, "NTP", 1.0, N, (0, 1)), (16, ("NEB", "NEBx2P"), 1, 43, None, "NEB", 1.0, N, (0, 1))]
    lnZ = rng.uniform(-30, -20, N_SCEN)
    lnZ[5] = -np.inf
    ess = rng.uniform(20, 2000, N_SCEN)
    lnM2 = 2 * lnZ - np.log(ess / N)
    lnW = -np.log(rng.uniform(2, 50, N_SCEN))
    rec = []
    for u in units:
        j0, nb = u[0], len(u[1])
        r = np.zeros((nb, len(sharding.RECORD_COLS) + 2))
        r[:, 14], r[:, 15], r[:, 16] = lnZ[j0:j0 + nb], lnM2[j0:j0 + nb], lnW[j0:j0 + nb]
        r[:, 0] = 1.0
        rec.append(r[:, :n_cols])
    return units, rec, lnZ, lnM2, lnW, N


def test_finish_sets_the_error_attributes():
    from triceratops_amd.triceratops import target
    rng = np.random.default_rng(5)
    units, rec, lnZ, lnM2, lnW, N = _records(rng, 17)
    tg = target.__new__(target)
    tg._finish(units, rec, N_SCEN)
    want = _mc_errors(lnZ, lnM2, N, "ok")
    fin = np.isfinite(lnZ)
    assert np.allclose(tg.ess[fin], N * np.exp(2 * lnZ[fin] - lnM2[fin]), rtol=1e-12) and tg.ess[5] == 0.0
    assert np.array_equal(tg.lnZ_err, want["lnZ_err"], equal_nan=True) and np.isnan(tg.lnZ_err[5])
    assert np.allclose(tg.lnZ_err[fin], np.sqrt(1 / tg.ess[fin] - 1 / N), rtol=1e-12)
    assert np.allclose(tg.w_max_frac, np.exp(lnW), rtol=1e-15)
    assert tg.FPP_err == want["FPP_err"] and tg.NFPP_err == want["NFPP_err"]
    assert np.isfinite(tg.FPP_err) and tg.FPP_err > 0 and np.isfinite(tg.NFPP_err) and tg.NFPP_err > 0
    # brute-force delta method on the table itself
    Z = np.exp(lnZ - lnZ[fin].max())
    V = np.where(fin, (Z * np.nan_to_num(tg.lnZ_err)) ** 2, 0.0)
    a = np.zeros(N_SCEN, dtype=bool)
    a[[0, 3, 9]] = True
    A, B, VA, VB = Z[a].sum(), Z[~a].sum(), V[a].sum(), V[~a].sum()
    assert tg.FPP_err == pytest.approx(np.sqrt((A * A * VB + B * B * VA) / (A + B) ** 4), rel=1e-12)
    # the deferred table (calc_probs_many on several ranks) reads the same
    tg2 = target.__new__(target)
    tg2._defer_finish(units, rec, N_SCEN)
    for name in ("ess", "lnZ_err", "w_max_frac"):
        assert np.array_equal(getattr(tg2, name), getattr(tg, name), equal_nan=True), name
    assert tg2.FPP_err == tg.FPP_err and tg2.NFPP_err == tg.NFPP_err and tg2.FPP == tg.FPP


def test_finish_without_moments_gives_nan_errors():
    from triceratops_amd.triceratops import target
    rng = np.random.default_rng(6)
    units, rec, lnZ, _, _, _ = _records(rng, 15)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        tg = target.__new__(target)
        tg._finish(units, rec, N_SCEN)
        assert np.array_equal(tg.lnZ, lnZ)
        assert np.all(np.isnan(tg.ess[np.isfinite(lnZ)])) and tg.ess[5] == 0.0
        assert np.all(np.isnan(tg.lnZ_err)) and np.all(np.isnan(tg.w_max_frac))
        assert np.isnan(tg.FPP_err) and np.isnan(tg.NFPP_err)
        tg2 = target.__new__(target)
        tg2._defer_finish(units, rec, N_SCEN)
        assert np.isnan(tg2.FPP_err) and np.array_equal(tg2.lnZ, lnZ)


def test_run_units_carries_the_moments_beside_the_records():
    """a unit whose evidence path reports moments (the _lib sink) gets them in the two columns behind RECORD_COLS;
    its result dicts do not change"""
    from triceratops_amd import _lib

    def thunk():
        _lib.moments_emit(-3.0, -0.5)
        _lib.moments_emit(-4.0, -0.25)
        d = {c: np.zeros(100) for c in sharding.RECORD_COLS if c != "lnZ"}
        return dict(d, lnZ=-1.0), dict(d, lnZ=-2.0)

    def quiet():
        d = {c: np.zeros(100) for c in sharding.RECORD_COLS if c != "lnZ"}
        return dict(d, lnZ=-1.5)
    units = [(0, ("EB", "EBx2P"), 1, 7, thunk, "EB"), (2, ("TP",), 1, 7, quiet, "TP")]
    rows = sharding.run_units(units, as_rows=True)
    assert rows[0].shape == (2, 17) and np.array_equal(rows[0][:, 14:], [[-1.0, -3.0, -0.5], [-2.0, -4.0, -0.25]])
    assert rows[1].shape == (1, 17) and rows[1][0, 14] == -1.5 and np.all(np.isnan(rows[1][0, 15:]))
    dicts = sharding.run_units(units)
    assert sorted(dicts[0][0]) == sorted(sharding.RECORD_COLS)
    assert not _lib.moments_wanted()


class _Replayed(Exception):
    pass


class _StubScenario:
    """what records_to_rows reads of a binary lnZ_* call drawn from numpy's stream (seeded numpy modes)"""
    philox = False
    want_moments = False
    moments = None

    def __init__(self):
        from types import SimpleNamespace
        self.a = SimpleNamespace(planet=0)

    def run_operator_chain(self, is_host, ncol):
        raise _Replayed()


def _binary_pending(stride, lnz1=500.0, ties1=1.0):
    """a Pending of a binary call with the record the library writes at `stride` doubles per branch: no tie in branch 0,
    `ties1` rows at the minimum of branch 1, branch 1's lnZ = lnz1"""
    import torch
    from triceratops_amd import fused
    rec = torch.zeros(fused.RECORD_MOMENTS, dtype=torch.float64)
    r = rec.numpy()
    for b, lnz in ((0, -3.0), (1, lnz1)):
        r[b * stride:b * stride + 14] = 1.0
        r[b * stride + 14] = lnz
        r[b * stride + 15] = 1000.0                       # masked draws
        r[b * stride + fused.SCEN_TIES] = 1.0 if b == 0 else ties1
        if stride == fused.SCENARIO_OUT_MOMENTS:
            r[b * stride + fused.SCEN_LNM2], r[b * stride + fused.SCEN_LNWMAX] = -7.0 - b, -0.5 - b
    r[2 * stride] = 0.0                                   # the limb-darkening flag
    return fused.Pending(_StubScenario(), rec, None, [], 14, 100, stride=stride)


@pytest.mark.parametrize("stride", [18, 20])
def test_records_of_either_width_replay_only_real_ties(monkeypatch, stride):
    """records_to_rows in a seeded numpy mode: a record without TRX_FLAG_WEIGHT_MOMENTS (fused.MOMENTS = False) is read
    at its own width -- no replay through the operator chain because of what sits where a 20-double record keeps its
    tie count, and a real tie in branch 1 is still replayed; with the flag the moments land behind the 15 columns"""
    from triceratops_amd import device_pipeline as dp
    from triceratops_amd import fused
    monkeypatch.setattr(dp, "RNG", dp.NumpyStreamRng())
    rows = fused.records_to_rows([("k", _binary_pending(stride))])["k"]
    assert rows.shape == (2, 17) and np.array_equal(rows[:, 14], [-3.0, 500.0])
    if stride == 18:
        assert np.all(np.isnan(rows[:, 15:]))
    else:
        assert np.array_equal(rows[:, 15:], [[-7.0, -0.5], [-8.0, -1.5]])
    # (branch 1's lnZ where the other width keeps the tie count: 1.0 must not look like a tie either)
    fused.records_to_rows([("k", _binary_pending(stride, lnz1=1.0))])
    with pytest.raises(_Replayed):
        fused.records_to_rows([("k", _binary_pending(stride, lnz1=-3.0, ties1=2.0))])
