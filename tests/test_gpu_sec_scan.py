"""The secondary-eclipse verdicts that the 25-point scan decides (trx_cells.hpp: rowc_kernel<SEC>'s quick test on the centre
point, the cross-workgroup list, sec_scan_kernel<8> / <8, WT> over the list, sec_scan_kernel<64> over every row) against
the CPU oracle, on the rows of tests/sec_rows.py -- rows whose verdict rests on the scan by construction (0.05 % of
synth.eb_rows' draws do).  Production library; no row is left out of any comparison.

Tolerances, none of them chosen here: ATOL_FLUX = 5e-13 and RTOL_H = 1e-9 of tests/test_gpu_kernels.py; 1e-12 relative
between the fused weighted kernel and the grid route (tests/test_gpu_lnl_weighted.py).  The designed verdicts keep 0.5 % of
the limit -- 3.7e-6 in depth -- on either side: the patterns are compared exactly.

Shapes: synth.time_grid(48) (rows batched per wave) and synth.time_grid(320) (one row per wave, cost-ordered
rowc_kernel<true, false, true>); n in {1, 7, 8, 9, 63, 64, 65, 511, 513, 4099}: 8-entry scan workgroups, 64-row blocks,
the 64 x 8 = 512 entries of the scan grid's first stride, and a list of several strides.

Measured on an MI355X: depths within 1.8e-14 of the oracle's (no grazing row stands out: the worst is a deep central
eclipse), finite chi^2/2 within 1.6e-13 relative of the oracle's, the fused weighted kernel within 4.3e-15 of the grid route.
On a build whose list scan takes only the centre point every test below but (a) fails; on one whose list scan stops after
its first stride (b) to (e) fail at every size whose list is longer than 512 entries (4099 rows; 513 scan-excluded rows;
1025 scan-decided rows).
"""
import numpy as np
import pytest
import torch

import sec_rows as S
from oracle import oracle as O
from triceratops_amd import _lib, synth

pytestmark = pytest.mark.gpu

RTOL_H = 1e-9
ATOL_FLUX = 5e-13
RTOL_ROUTES = 1e-12
SIZES = (1, 7, 8, 9, 63, 64, 65, 511, 513, 4099)
N_TIMES = (48, 320)
# "mixed": the four kinds; "open": the list holds all n rows; "scan-excluded": it holds all n rows and EVERY one of them must
# come back +inf -- an entry the scan drops anywhere (the 513th, a stride's tail) shows, whatever kind the shuffle put there
ARRANGEMENTS = {"mixed": S.KINDS, "open": S.OPEN_KINDS, "scan-excluded": ("scan-excluded",)}
VARIANT_IDS = sorted(S.VARIANTS)

_lcs, _refs = {}, {}


def _lc(n_time):
    """the light curve of tests/test_gpu_kernels.py::_lc, on the host and on the device"""
    if n_time not in _lcs:
        rng = np.random.default_rng(synth.SEED)
        t = synth.time_grid(n_time)
        flux = synth.noisy_light_curve(rng, O.flux_grid(O.MODEL_TP, t, synth.reference_tp_row())[0][0])
        _lcs[n_time] = dict(t=t, flux=flux, t_d=_lib.dev(t), f_d=_lib.dev(flux),
                            w_d=_lib.dev(np.full(n_time, 1.0 / synth.SIGMA ** 2)))
    return _lcs[n_time]


def _ref(variant):
    """once per variant and module: every designed row, the oracle's chi^2/2 on both light curves and its secondary
    depths; never changed afterwards (a test's rows are indices into it)"""
    if variant not in _refs:
        rows, kind = S.all_rows(variant)
        host = S.blocks(variant)["host"]
        r = dict(rows=rows, kind=kind, host=host, flags=_lib.FLAG_COMPANION_IS_HOST if host else 0,
                 sec=S.oracle_depth(rows, host), argmin=S.scan_argmin(variant))
        for nt in N_TIMES:
            lc = _lc(nt)
            r[nt] = O.lnl_batch(O.MODEL_EB, lc["t"], lc["flux"], synth.SIGMA, rows, companion_is_host=host)
            r[nt].setflags(write=False)
        excluded = np.isin(kind, [S.KINDS.index(k) for k in S.EXCLUDED_KINDS])
        assert np.array_equal(np.isposinf(r[48]), excluded) and np.array_equal(np.isposinf(r[320]), excluded)
        _refs[variant] = r
    return _refs[variant]


def _lnl(variant, nt, rows_d, flags=0, sigma=synth.SIGMA, out=None):
    lc = _lc(nt)
    return _lib.lnl_batch(_lib.MODEL_EB, _ref(variant)["flags"] | flags, lc["t_d"], lc["f_d"], sigma, rows_d, synth.EXPTIME,
                          synth.NSAMPLES, out=out)


def _weighted(variant, nt, rows_d, limit):
    lc = _lc(nt)
    return _lib.lnl_batch_weighted(_lib.MODEL_EB, _ref(variant)["flags"], lc["t_d"], lc["f_d"], lc["w_d"], rows_d,
                                   synth.EXPTIME, synth.NSAMPLES, limit)


def _depths(variant, rows_d):
    grid, sec = _lib.flux_grid(_lib.MODEL_EB, _ref(variant)["flags"], _lc(48)["t_d"], rows_d, synth.EXPTIME, synth.NSAMPLES)
    return grid, sec


def _against(got, want, what):
    """the +inf pattern exactly, no NaN, every finite row within RTOL_H; returns the largest relative error"""
    assert got.shape == want.shape and not np.isnan(got).any(), what
    bad = np.flatnonzero(np.isposinf(got) != np.isposinf(want))
    assert bad.size == 0, "%s: %d verdicts differ, first rows %s: got %s, oracle %s" % (what, bad.size, bad[:8], got[bad[:8]],
                                                                                       want[bad[:8]])
    fin = np.isfinite(want)
    rel = float(np.max(np.abs(got[fin] - want[fin]) / np.abs(want[fin]))) if fin.any() else 0.0
    assert rel < RTOL_H, (what, rel)
    return rel


# ---------------------------------------------------------------------------------------
# a. the depth itself: sec_scan_kernel<64> over every row
@pytest.mark.parametrize("variant", VARIANT_IDS)
def test_depth_of_every_designed_row_against_the_oracle(variant):
    r = _ref(variant)
    sec = _depths(variant, _lib.dev(r["rows"]))[1].cpu().numpy()
    err = np.abs(sec - r["sec"])
    worst = int(np.argmax(err))
    print("%s: %d rows, max |secdepth - oracle| %.3g (row %d, %s, minimum at point %d)"
          % (variant, sec.size, err[worst], worst, S.KINDS[r["kind"][worst]], r["argmin"][worst]))
    assert not np.isnan(sec).any()
    assert err.max() < ATOL_FLUX, (err.max(), worst)


# ---------------------------------------------------------------------------------------
# b. verdicts of trx_lnl_batch: the quick test, the list, sec_scan_kernel<8>
@pytest.mark.parametrize("arrangement", sorted(ARRANGEMENTS))
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("variant", VARIANT_IDS)
def test_lnl_batch_verdicts(variant, n, arrangement):
    r = _ref(variant)
    rows, kind, at = S.arrange(ARRANGEMENTS[arrangement], n, 0, variant)
    rows_d = _lib.dev(rows)
    for nt in N_TIMES:
        got = _lnl(variant, nt, rows_d).cpu().numpy()
        rel = _against(got, r[nt][at], "%s n %d %s n_time %d" % (variant, n, arrangement, nt))
        print("%s n %d %s n_time %d: %d of %d rows +inf, max relative error of the others %.3g"
              % (variant, n, arrangement, nt, int(np.isposinf(got).sum()), n, rel))
        evaluated = _lnl(variant, nt, rows_d, _lib.FLAG_EVALUATE_EXCLUDED).cpu().numpy()
        assert evaluated.tobytes() == got.tobytes(), (nt, np.flatnonzero(evaluated != got)[:8])


# ---------------------------------------------------------------------------------------
# c. verdicts of trx_lnl_batch_weighted: rowc_kernel<true, WT>, sec_scan_kernel<8, WT>
@pytest.mark.parametrize("arrangement", sorted(ARRANGEMENTS))
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("variant", VARIANT_IDS)
def test_lnl_batch_weighted_verdicts(variant, n, arrangement):
    r = _ref(variant)
    rows, kind, at = S.arrange(ARRANGEMENTS[arrangement], n, 1, variant)
    rows_d = _lib.dev(rows)
    for nt in N_TIMES:
        lc = _lc(nt)
        what = "%s n %d %s n_time %d" % (variant, n, arrangement, nt)
        got = _weighted(variant, nt, rows_d, S.L).cpu().numpy()
        rel = _against(got, r[nt][at], what)
        grid, sec = _lib.flux_grid(_lib.MODEL_EB, r["flags"], lc["t_d"], rows_d, synth.EXPTIME, synth.NSAMPLES)
        route = _lib.chi2_grid_weighted(lc["f_d"], lc["w_d"], grid, sec, S.L).cpu().numpy()
        assert np.array_equal(np.isposinf(route), np.isposinf(got)) and not np.isnan(route).any(), what
        fin = np.isfinite(route)
        rel_route = float(np.max(np.abs(got[fin] / route[fin] - 1.0))) if fin.any() else 0.0
        print("%s: %d of %d rows +inf, max relative error against the oracle %.3g, against the grid route %.3g"
              % (what, int(np.isposinf(got).sum()), n, rel, rel_route))
        assert rel_route < RTOL_ROUTES, (what, rel_route)


# ---------------------------------------------------------------------------------------
# d. sec_scan_kernel<64>, <8> and <8, WT> give one depth, to the bit
# (513 rows of the four kinds: at most 385 of them open, one stride of the list scan; 1025 scan-decided rows: a list of two
# strides and an entry, so that a limit placed on a row's depth is also met by entries of the later strides)
@pytest.mark.parametrize("kinds,n", [(S.KINDS, 513), (("scan-excluded", "scan-kept"), 1025)], ids=["mixed-513", "scan-decided-1025"])
@pytest.mark.parametrize("variant", VARIANT_IDS)
def test_the_three_scans_agree_to_the_bit(variant, kinds, n):
    r = _ref(variant)
    rows, kind, at = S.arrange(kinds, n, 2, variant)
    rows_d = _lib.dev(rows)
    d = _depths(variant, rows_d)[1].cpu().numpy()
    assert np.abs(d - r["sec"][at]).max() < ATOL_FLUX
    argmin = r["argmin"][at]
    picks = []
    for k in ("scan-excluded", "scan-kept"):
        mine = np.flatnonzero(kind == S.KINDS.index(k))
        ends = [mine[argmin[mine] == 0][0], mine[argmin[mine] == S.N_POINTS - 1][0]]        # the scan's two end points
        rest = [i for i in mine if i not in ends and argmin[i] not in (0, S.N_POINTS - 1)]
        picks += ends + rest[:6]
    assert len(picks) == 16 and len(set(picks)) == 16
    for i in picks:
        what = "%s row %d (%s, minimum at point %d)" % (variant, i, S.KINDS[kind[i]], argmin[i])
        at_limit = _weighted(variant, 48, rows_d, float(d[i])).cpu().numpy()
        assert not np.isnan(at_limit).any()
        assert np.array_equal(np.isposinf(at_limit), d >= d[i]), (what, np.flatnonzero(np.isposinf(at_limit) != (d >= d[i]))[:8])
        above = _weighted(variant, 48, rows_d, float(np.nextafter(d[i], np.inf))).cpu().numpy()
        assert np.isfinite(above[i]), what
        assert np.array_equal(np.isposinf(above), d > d[i]), what
        sigma = float(d[i] / 1.5)
        plain = _lnl(variant, 48, rows_d, sigma=sigma).cpu().numpy()
        want = ~(d < 1.5 * np.float64(sigma))                  # the kernel's single IEEE multiply, formed in numpy
        assert not np.isnan(plain).any()
        assert np.array_equal(np.isposinf(plain), want), (what, np.flatnonzero(np.isposinf(plain) != want)[:8])


# ---------------------------------------------------------------------------------------
# e. the list and its counter between calls
def test_list_state_between_calls_and_streams():
    """a list of several strides, then an empty one, then a mixed one, back to back on one stream and interleaved on two:
    each call's bytes are those it gave on its own -- a counter that was not reset, or a list read beyond the counter,
    would show as verdicts of the call before"""
    variant = "companion"
    r = _ref(variant)
    calls = [S.arrange(S.OPEN_KINDS, 4099, 5, variant), S.arrange(("centre-excluded",), 65, 5, variant),
             S.arrange(S.KINDS, 513, 5, variant)]
    devs = [_lib.dev(c[0]) for c in calls]
    for nt in N_TIMES:
        alone = []
        for c, rows_d in zip(calls, devs):
            torch.cuda.synchronize()
            h = _lnl(variant, nt, rows_d).cpu().numpy()
            torch.cuda.synchronize()
            _against(h, r[nt][c[2]], "alone, %d rows, n_time %d" % (c[0].shape[1], nt))
            alone.append(h)
        assert np.isinf(alone[1]).all() and np.isfinite(alone[0]).sum() > 2000
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        # one stream, back to back; then both streams taking turns
        for order in ([(0, j) for j in range(3)], [(s, j) for j in range(3) for s in (0, 1)]):
            outs = []
            torch.cuda.synchronize()
            for s, j in order:
                with torch.cuda.stream(streams[s]):
                    outs.append((s, j, _lnl(variant, nt, devs[j])))
            torch.cuda.synchronize()
            for s, j, h in outs:
                assert h.cpu().numpy().tobytes() == alone[j].tobytes(), (nt, len(order), s, j)
