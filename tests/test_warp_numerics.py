"""The host side of the adaptive importance map: _numerics.warp_refine / warp_apply, and the
bindings' view of the two new ABI fields (trx_draw_args.warp, trx_scenario_args.warp_hist).  No GPU needed."""
import ctypes
import os

import numpy as np
import pytest

from triceratops_amd import _numerics as nm

D, B = nm.WARP_DIMS, nm.WARP_BINS


def _valid(edges, floor):
    assert edges.shape == (D, B + 1)
    assert np.all(edges[:, 0] == 0.0) and np.all(edges[:, -1] == 1.0)
    w = np.diff(edges, axis=1)
    assert np.all(w > 0)
    assert np.all(1.0 / (B * w) >= floor * (1 - 1e-12))


def test_identity_grid():
    I = nm.warp_identity()
    assert I.shape == (D, B + 1) and np.array_equal(I[3], np.arange(B + 1) / B)
    y = np.random.default_rng(1).random(100000)
    y[:3] = 0.0, np.nextafter(1.0, 0.0), 0.5
    assert np.array_equal(nm.warp_apply(I[0], y), y)
    assert np.all(nm.warp_lnj(I[0], y) == 0.0)


@pytest.mark.parametrize("floor", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("alpha", [0.5, 1.0])
def test_refine_gives_valid_edges(alpha, floor):
    rng = np.random.default_rng(5)
    edges = nm.warp_identity()
    for _ in range(4):                    # refined again and again, from ever less regular grids
        hist = rng.random((D, B)) ** 8 * 1e12
        hist[rng.integers(0, D), :] = 0.0
        edges = nm.warp_refine(edges, hist, alpha=alpha, floor=floor)
        _valid(edges, floor)


def test_flat_and_zero_histograms_return_the_identity_exactly():
    I = nm.warp_identity()
    assert np.array_equal(nm.warp_refine(I, np.zeros((D, B))), I)
    assert np.array_equal(nm.warp_refine(I, np.full((D, B), 12345.0)), I)
    # a dimension without weight keeps its row while the others move
    h = np.zeros((D, B))
    h[2, 7] = 1.0
    e = nm.warp_refine(I, h)
    assert np.array_equal(np.delete(e, 2, axis=0), np.delete(I, 2, axis=0)) and not np.array_equal(e[2], I[2])


def test_a_concentrated_histogram_narrows_the_bins_there():
    I = nm.warp_identity()
    h = np.zeros((D, B))
    h[4, 40] = 1e15
    e = nm.warp_refine(I, h, alpha=0.5, floor=0.1)
    _valid(e, 0.1)
    w = np.diff(e[4])
    k = int(np.argmin(w))
    # the narrowest bin lies where the weight was (the 3-point smoothing spreads it over bins 39 .. 41)
    assert 39 / B <= e[4, k] and e[4, k + 1] <= 42 / B
    assert w[k] < 0.1 / B
    # most of the proposal's mass went there, and the floor kept the rest of the cube covered
    inside = np.sum((e[4, :-1] >= 39 / B) & (e[4, 1:] <= 42 / B))
    assert inside >= 40
    assert w.max() <= 1.0 / (B * 0.1) * (1 + 1e-12)


def test_branches_combine_by_their_maxima():
    """a binary call's two blocks: the branch whose X is 30 lower counts with exp(-30)"""
    W = 8 + D * B
    blocks = np.zeros((2, W), dtype=np.uint64)
    X = np.array([-100.0, -130.0])
    blocks[:, 0] = X.view(np.uint64)
    blocks[:, 1] = 5
    blocks[0, 8 + 3 * B + 10] = 1000
    blocks[1, 8 + 3 * B + 50] = 1000
    bins = nm.warp_hist_bins(blocks)
    assert bins[3, 10] == 1000.0 and bins[3, 50] == 1000.0 * np.exp(-30.0) and bins.sum() == bins[3, 10] + bins[3, 50]
    as_doubles = blocks.astype(np.float64)
    as_doubles[:, 0] = X
    assert np.array_equal(nm.warp_hist_bins(as_doubles), bins)
    blocks[1, 1] = 0                                       # a branch without rows does not count at all
    assert nm.warp_hist_bins(blocks)[3, 50] == 0.0
    assert np.array_equal(nm.warp_refine(nm.warp_identity(), blocks), nm.warp_refine(nm.warp_identity(), nm.warp_hist_bins(blocks)))


def test_apply_is_monotonic_and_the_interpolant_of_the_edges():
    rng = np.random.default_rng(11)
    e = nm.warp_refine(nm.warp_identity(), rng.random((D, B)) ** 6)[1]
    y = np.sort(rng.random(200000))
    u = nm.warp_apply(e, y)
    assert np.all(np.diff(u) >= 0) and u.min() >= 0.0 and u.max() < 1.0
    assert np.max(np.abs(u - np.interp(y, np.arange(B + 1) / B, e))) <= 1e-15
    # ln J is the log of the slope
    k = np.minimum((y * B).astype(int), B - 1)
    assert np.allclose(nm.warp_lnj(e, y), np.log(B * np.diff(e)[k]), rtol=0, atol=1e-15)


def test_bindings_follow_the_header():
    from triceratops_amd import _lib, fused
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "trx.h")).read()
    assert "#define TRX_WARP_DIMS %d" % _lib.WARP_DIMS in text and "#define TRX_WARP_BINS %d" % _lib.WARP_BINS in text
    assert "#define TRX_WARP_BRANCH (8 + TRX_WARP_DIMS * TRX_WARP_BINS)" in text
    assert _lib.WARP_BRANCH == 8 + _lib.WARP_DIMS * _lib.WARP_BINS == fused.WARP_BRANCH
    assert [f[0] for f in fused.DrawArgs._fields_][-1] == "warp"
    assert "warp_hist" in [f[0] for f in fused.ScenarioArgs._fields_]
    if os.path.exists(_lib.LIB_PATH):
        L = _lib.lib()
        L.trx_draw_args_size.restype = L.trx_scenario_args_size.restype = ctypes.c_size_t
        assert L.trx_draw_args_size() == ctypes.sizeof(fused.DrawArgs)
        assert L.trx_scenario_args_size() == ctypes.sizeof(fused.ScenarioArgs)
    assert fused.WARP_GRIDS is None and fused.WARP_HIST is False
    flat = fused.warp_hist_to_flat(np.array([np.float64(-12.5).view(np.int64), 3, 0, 7], dtype=np.int64))
    assert list(flat) == [-12.5, 3.0, 0.0, 7.0]


def test_refined_needs_the_device_mode():
    import triceratops_amd
    from triceratops_amd.triceratops import target
    assert hasattr(target, "calc_probs_refined")
    tg = target.__new__(target)
    triceratops_amd.set_sampling("numpy")
    with pytest.raises(NotImplementedError):
        tg.calc_probs_refined(np.zeros(4), np.ones(4), 1e-3, 1.0, n_adapt=1)
    with pytest.raises(ValueError):
        tg.calc_probs_refined(np.zeros(4), np.ones(4), 1e-3, 1.0, n_adapt=-1)
