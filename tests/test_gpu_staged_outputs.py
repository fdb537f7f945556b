"""Destinations the device cannot write (trx_star_enqueue, csrc/trx_scenario.hip): a record, a posterior block or a weight
histogram in plain host memory goes through the library's arena and is copied back behind the kernels; in pinned memory
the kernels write it directly (the histogram is staged either way).  Both routes, through a launch chain and call by
call, must leave the same bytes: the argument blocks -- and with them the seeds -- are the same in all four runs, only
the destinations and the chain switch differ."""
import ctypes
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from helpers import GOLD, gold
from test_gpu_posterior import SEED, _device_mode

pytestmark = pytest.mark.gpu

N_DRAWS = 50_000                       # (the chain tests' calls form chains at this size)
POST_ROWS = (257, 0, 1)                # of the planet, the binary and the companion-prior call


def _slots(planet, W):
    """the record slots a call defines (tests/test_gpu_posterior_chain.py::_slots)"""
    nbr, ncol = (1, 11) if planet else (2, 14)
    return [b * W + i for b in range(nbr) for i in list(range(ncol + 2)) + list(range(16, W))] + [2 * W]


def _enqueue(L, blocks, stream, chain, pinned):
    """ONE trx_star_enqueue of the blocks on the stream, destinations pinned or plain: per call (defined record slots,
    posterior block [nbr][8 + 16 M] or None, histogram [nbr][WARP_BRANCH]), and trx_debug_chain_counts of the enqueue"""
    from triceratops_amd import _lib, fused
    n = len(blocks)

    def dest(shape, dtype):
        if pinned:
            t = torch.zeros(shape, dtype=dtype).pin_memory()
            return t, t.numpy(), t.data_ptr()
        a = np.zeros(shape, dtype=np.float64 if dtype == torch.float64 else np.int64)
        return a, a, a.ctypes.data

    calls = (fused.ScenarioArgs * n)()
    outs, sts = (ctypes.c_void_p * n)(), (ctypes.c_void_p * n)()
    alive, recs, posts, hists = [], [], [], []
    for i, (sa, M) in enumerate(zip(blocks, POST_ROWS)):
        keep, rec, outs[i] = dest((fused.RECORD_MOMENTS,), torch.float64)
        alive.append(keep)
        recs.append(rec)
        keep, hist, sa.warp_hist = dest((2, _lib.WARP_BRANCH), torch.int64)
        alive.append(keep)
        hists.append(hist)
        posts.append(None)
        sa.post_rows, sa.post = M, None
        if M:
            keep, posts[i], sa.post = dest((2, 8 + 16 * M), torch.float64)
            alive.append(keep)
        calls[i] = sa
        sts[i] = stream.cuda_stream
    c = [ctypes.c_long(0) for _ in range(3)]
    done = ctypes.c_int(0)
    L.trx_set_star_chain(1 if chain else 0)
    L.trx_debug_chain_counts(None, None, None, 1)
    assert L.trx_star_enqueue(calls, n, outs, sts, ctypes.byref(done)) == 0, L.trx_last_error()
    assert done.value == n
    L.trx_debug_chain_counts(ctypes.byref(c[0]), ctypes.byref(c[1]), ctypes.byref(c[2]), 0)
    stream.synchronize()                  # (`alive` holds every destination until here)
    out = []
    for sa, rec, post, hist in zip(blocks, recs, posts, hists):
        planet = bool(sa.draw.contents.planet)
        W = fused.SCENARIO_OUT_MOMENTS if sa.flags & _lib.FLAG_WEIGHT_MOMENTS else fused.SCENARIO_OUT
        nbr = 1 if planet else 2
        out.append((rec[_slots(planet, W)].copy(), None if post is None else post[:nbr].copy(), hist[:nbr].copy()))
    del alive
    return out, (int(c[0].value), int(c[1].value))


def test_staged_and_direct_destinations_hold_the_same_bytes_chained_or_not():
    from triceratops_amd import _lib, fused
    _lib.require_gpu()
    G = gold("lnz_cases.npz")
    base = (G["time"], G["flux"], float(G["sigma"][0]), 3.3, 0.82, 0.8, 5100.0, 0.0)
    bound = base + (10.0, os.path.join(GOLD, "contrast_curve_synth.csv"), "TESS")
    kw = dict(N=N_DRAWS, parallel=True)
    L = _lib.lib()
    saved = fused.TABLE_ROWS
    runs, counts = {}, {}
    with _device_mode():
        try:
            fused.TABLE_ROWS = 1
            fused.set_thread_seed(SEED)
            with fused.switches(WARP_HIST=True, POSTERIOR_ROWS=0):
                fused.begin_deferred(3)
                pend = [fused.lnZ_TTP(*base, **kw), fused.lnZ_TEB(*base, **kw), fused.lnZ_PTP(*bound, **kw)]
            assert all(isinstance(p, fused.Pending) for p in pend)
            blocks = [b[0] for b in fused._tls.batch]           # the argument blocks fused collected (not yet enqueued)
            fused._tls.batch = []
            assert len(blocks) == 3
            for i, (sa, p) in enumerate(zip(blocks, pend)):
                # (fused does not combine a histogram with posterior rows; the library does: the key fused would pass)
                sa.post_seed = p.scen.post_seed()
                if i % 2:
                    sa.flags |= _lib.FLAG_WEIGHT_MOMENTS
            stream = torch.cuda.Stream()
            _lib.wait_uploads(stream)                           # (the light curve went up asynchronously)
            torch.cuda.synchronize()
            for chain in (True, False):
                for pinned in (True, False):
                    runs[chain, pinned], counts[chain, pinned] = _enqueue(L, blocks, stream, chain, pinned)
        finally:
            fused._tls.batch = []
            fused.end_deferred()
            L.trx_set_star_chain(1)
            fused.TABLE_ROWS = saved
    for pinned in (True, False):
        assert counts[True, pinned] == (1, 3), counts
        assert counts[False, pinned] == (0, 0), counts
    want = runs[False, True]
    for i, ((rec, post, hist), M) in enumerate(zip(want, POST_ROWS)):
        ncol = 11 if i != 1 else 14
        assert np.isfinite(rec[ncol]) and rec[ncol + 1] > 100 and hist[:, 1].min() > 0          # lnZ, masked draws, rows with weight
        assert (post is None) == (M == 0)
        if M:
            assert post[0, 3] > 0 and np.all(np.isfinite(post))
    for key, got in runs.items():
        for i, ((ra, pa, ha), (rb, pb, hb)) in enumerate(zip(got, want)):
            assert ra.tobytes() == rb.tobytes(), ("record", key, i)
            assert ha.tobytes() == hb.tobytes(), ("histogram", key, i)
            assert (pa is None) == (pb is None)
            if pa is not None:
                assert pa.tobytes() == pb.tobytes(), ("posterior block", key, i)
