"""Uniform time grids: cells_kernel's stencil instantiation walks only the 64-cell trips of the window pass that can hold
an in-window cell (trx_cells.hpp, window_trips) and takes the flat model's chi^2 of the other trips from the launch header.

tests/golden/window_trips.npz (make_window_trips.py) holds the inputs -- grids of 478, 2000 and 2048 + 1 points at 0.12,
0.18 and 0.29 exposures per step, at several offsets against conjunction; TP rows with periods from many epochs per light
curve to none, windows that wrap round the orbit, eccentric two-passage rows, flat rows, a NaN-dilution row; EB rows on both
sides of the secondary-eclipse rule -- and what the library computed on them before the change, when every trip was walked
and the row's own lanes summed every cell's chi^2 term.

  * chi^2/2 against the CPU oracle: the project's 1e-9 relative bar;
  * chi^2/2 against that direct sum: 1e-12 relative (the same non-negative terms, added in another order: expected
    error n_time x 1.1e-16 = 2e-13);
  * flat rows: the same bits, all of them;
  * the flux grid: the same bits as before, and within 5e-13 of the oracle;
  * the evaluation census (TRX_FLAG_COUNT_EVALUATIONS): the same count in every cell -- no evaluation added or dropped,
    which also says that the in-window list is the same cells in the same order (the stencil's neighbours are list
    neighbours).
"""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import oracle as O
from triceratops_amd import _lib

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "window_trips.npz")
RTOL_ORACLE = 1e-9
RTOL_DIRECT = 1e-12
ATOL_FLUX = 5e-13
N_CASES = 10
BLOCKS = (("tp", _lib.MODEL_TP, O.MODEL_TP), ("eb", _lib.MODEL_EB, O.MODEL_EB))


@pytest.fixture(scope="module")
def gold():
    g = np.load(GOLD, allow_pickle=False)
    assert int(g["n_cases"]) == N_CASES
    return g


def _rel(got, want, what):
    assert np.array_equal(np.isposinf(want), np.isposinf(got)), what
    assert np.array_equal(np.isnan(want), np.isnan(got)), what
    fin = np.isfinite(want)
    rel = np.abs(got[fin] - want[fin]) / np.maximum(np.abs(want[fin]), 1e-300)
    return float(rel.max()) if fin.any() else 0.0


@pytest.mark.parametrize("ci", range(N_CASES))
def test_chi2_matches_the_oracle_and_the_direct_sum(gold, ci):
    p = "c%d_" % ci
    t, flux = gold[p + "t"], gold[p + "flux"]
    exptime, S, sigma = float(gold["exptime"]), int(gold["nsamples"]), float(gold["sigma"])
    t_d, f_d = _lib.dev(t), _lib.dev(flux)
    for key, model, omodel in BLOCKS:
        rows = gold[p + key]
        got = _lib.lnl_batch(model, 0, t_d, f_d, sigma, _lib.dev(rows), exptime, S).cpu().numpy()
        want = O.lnl_batch(omodel, t, flux, sigma, rows, exptime=exptime, nsamples=S)
        r_oracle = _rel(got, want, (ci, key, "oracle"))
        r_direct = _rel(got, gold[p + "h_" + key], (ci, key, "direct sum"))
        print("case %d (%d points) %s: vs oracle %.3g, vs the direct sum %.3g" % (ci, t.size, key, r_oracle, r_direct))
        assert r_oracle < RTOL_ORACLE, (ci, key, r_oracle)
        assert r_direct < RTOL_DIRECT, (ci, key, r_direct)
        if key == "tp":
            # the block's last three rows: two that pass the star by (flat: the same bits, and those of every other row
            # whose model is 1 over the data) and one whose dilution is NaN
            grid = O.flux_grid(omodel, t, rows, exptime=exptime, nsamples=S)[0]
            flat = np.all(grid == 1.0, axis=1)
            assert flat[-3] and flat[-2] and flat.sum() >= 2
            assert np.unique(got[flat].view(np.uint64)).size == 1
            assert np.isnan(got[-1])
        else:
            assert np.isposinf(got).any() and np.isfinite(got).any()         # both sides of the secondary-eclipse rule


@pytest.mark.parametrize("ci", range(N_CASES))
def test_flux_grid_and_evaluation_census_are_unchanged(gold, ci):
    p = "c%d_" % ci
    t = gold[p + "t"]
    exptime, S = float(gold["exptime"]), int(gold["nsamples"])
    t_d = _lib.dev(t)
    for key, model, omodel in BLOCKS:
        rows = np.ascontiguousarray(gold[p + key][:, gold[p + "pick_" + key]])
        r_d = _lib.dev(rows)
        grid = _lib.flux_grid(model, 0, t_d, r_d, exptime, S, False)[0].cpu().numpy()
        was = gold[p + "grid_" + key]
        assert np.array_equal(grid.view(np.uint64), was.view(np.uint64)), (ci, key)
        want = O.flux_grid(omodel, t, rows, exptime=exptime, nsamples=S)[0]
        assert np.array_equal(np.isnan(want), np.isnan(grid))
        fin = np.isfinite(want)
        assert np.abs(grid[fin] - want[fin]).max() < ATOL_FLUX
        count = _lib.flux_grid(model, _lib.FLAG_COUNT_EVALUATIONS, t_d, r_d, exptime, S, False)[0].cpu().numpy()
        assert np.array_equal(count, gold[p + "count_" + key].astype(np.float64)), (ci, key)
        if key == "tp":
            assert count[-3:-1].max() == 0.0        # the flat rows cost nothing


def test_the_grids_take_the_stencil_instantiation(gold):
    """(what the cases are for: a stencil cell costs ONE evaluation, its centre, where the smallest Gauss tier has three nodes;
    with the stencil switched off per call no evaluated cell costs fewer than three)"""
    from triceratops_amd import synth
    t_d = _lib.dev(gold["c3_t"])
    r_d = _lib.dev(synth.reference_tp_row())
    exptime, S = float(gold["exptime"]), int(gold["nsamples"])
    on, off = (_lib.flux_grid(_lib.MODEL_TP, _lib.FLAG_COUNT_EVALUATIONS | f, t_d, r_d, exptime, S, False)[0].cpu().numpy()
               for f in (0, _lib.FLAG_NO_STENCIL))
    assert np.any(on == 1.0) and off[off > 0].min() >= 3.0 and np.all(off[on == 1.0] >= 3.0)
