"""Posterior samples on the device: trx_posterior_from_halfchi2 and trx_scenario_args.post_rows against a numpy
restatement of the definition (include/trx.h): weights in np.longdouble, cumulative sums by longdouble cumsum.

Acceptance of a selection, given the yardstick's w, C, S and the reported u: for every j, w[r_j] > 0 and
C[r_j - 1] - tol <= t_j <= C[r_j] + tol with t_j = (u + j) / M * S and tol = (4 n 2^-53 + 1e-11) S -- the worst-case
rounding of an n-term fp64 sum in any order, plus the last-bit differences of chi^2 between bounded and full evaluation
(tests/test_gpu_mc_error.py holds 1e-11 for the effective sample size) --, r_j non-decreasing, and for every draw
|count_i - M w_i / S| < 1 + M tol / S."""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
LD = np.longdouble


def yardstick(h, lnprior, lnsigma):
    """(x, w, C, S, X) of the definition; w is None where the evidence is +inf (no posterior)"""
    x = (-0.5 * np.log(2 * np.pi) - lnsigma) - np.asarray(h, dtype=np.float64)
    if lnprior is not None:
        x = x + lnprior
    if np.any(x == np.inf):
        return x, None, None, LD(0), np.nan
    fin = np.isfinite(x)
    if not fin.any():
        return x, np.zeros(x.size, dtype=LD), np.zeros(x.size, dtype=LD), LD(0), -np.inf
    X = x[fin].max()
    with np.errstate(invalid="ignore", over="ignore"):
        d = x - X
        w = np.where(fin & (d > -80.0), np.exp(np.where(fin, d, 0.0).astype(LD)), LD(0))
    C = np.cumsum(w, dtype=LD)
    return x, w, C, C[-1], X


def accept(pos, u, w, C, S, M):
    n = w.size
    pos = np.asarray(pos, dtype=np.int64)
    assert pos.shape == (M,) and pos.min() >= 0 and pos.max() < n
    assert np.all(np.diff(pos) >= 0)
    assert np.all(w[pos] > 0)
    tol = (4 * n * LD(2) ** -53 + LD(1e-11)) * S
    t = (LD(u) + np.arange(M, dtype=LD)) / M * S
    before = np.where(pos > 0, C[np.maximum(pos - 1, 0)], LD(0))
    worst = max(float((before - t).max() / S), float((t - C[pos]).max() / S))
    print("n = %d, M = %d: targets outside [C[r - 1], C[r]] by at most %.3g S (tol %.3g S)" % (n, M, worst, float(tol / S)))
    assert np.all(before - tol <= t) and np.all(t <= C[pos] + tol)
    count = np.bincount(pos, minlength=n)
    assert np.all(np.abs(count - M * w / S) < 1 + M * tol / S)


def vector(kind, n, rng):
    """chi^2/2 values and a prior of n rows"""
    lp = rng.normal(0.0, 2.0, n)
    if kind == "broad":
        h = rng.uniform(0.0, 1e4, n)
    elif kind == "narrow":
        h = 500.0 + rng.uniform(0.0, 1.0, n)
    elif kind == "dominant":
        h = 1000.0 + rng.uniform(200.0, 1e4, n)
        h[n // 3] = 10.0
        lp[:] = 0.0
    elif kind == "excluded":
        h = rng.uniform(0.0, 50.0, n)
        h[::3] = np.inf
        h[1::7] = np.nan
        lp[::5] = -np.inf
        if n < 8:
            h[-1], lp[-1] = 3.0, 0.5
    elif kind == "none":
        h = np.full(n, np.inf)
        h[::2] = np.nan
    return h, lp


def select(h, lp, lnsigma, M, seed):
    from triceratops_amd import _lib
    h_d = _lib.dev(h)
    lp_d = None if lp is None else _lib.dev(lp)
    pos, hdr = _lib.posterior_from_halfchi2(h_d, lp_d, lnsigma, M, seed)
    return pos.cpu().numpy(), hdr.cpu().numpy()


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 2047, 2048, 2049, 100000, 3000000])
@pytest.mark.parametrize("kind", ["broad", "narrow", "dominant", "excluded", "none"])
def test_selection_matches_the_definition(n, kind):
    from triceratops_amd import _lib
    _lib.require_gpu()
    rng = np.random.default_rng(1000 * n % 9973 + len(kind))
    h, lp_all = vector(kind, n, rng)
    lnsigma = float(np.log(3e-4))
    for lp in (None, lp_all):
        x, w, C, S, X = yardstick(h, lp, lnsigma)
        for M in (1, 7, 1000, _lib.POST_MAX_ROWS):
            pos, hdr = select(h, lp, lnsigma, M, 12345 + M)
            again, hdr2 = select(h, lp, lnsigma, M, 12345 + M)
            assert np.array_equal(pos, again) and hdr.tobytes() == hdr2.tobytes()
            assert 0.0 <= hdr[0] < 1.0
            if S == 0:
                assert hdr[3] == 0 and np.all(pos == -1)
                continue
            assert hdr[1] == X and hdr[3] == np.count_nonzero(w)
            tol = (4 * n * LD(2) ** -53 + LD(1e-11)) * S
            assert abs(np.exp(LD(hdr[2])) - S) <= tol + 4e-16 * S
            accept(pos, hdr[0], w, C, S, M)
            if kind == "dominant":
                assert np.all(pos == n // 3)
            if M == 7:
                other, hdr3 = select(h, lp, lnsigma, M, 999)
                assert hdr3[0] != hdr[0]


def test_an_infinite_weight_leaves_no_posterior():
    h = np.array([3.0, -np.inf, 5.0, 1.0])
    pos, hdr = select(h, None, 0.0, 5, 1)
    assert hdr[3] == 0 and np.all(pos == -1)
    pos, hdr = select(np.zeros(0), None, 0.0, 5, 1)
    assert hdr[3] == 0 and np.all(pos == -1)


# ---------------------------------------------------------------------------------------------------------------------
# scenario level: TOI-465.01, the inputs of tests/test_toi465.py
N_DRAWS, M_ROWS, SEED = 100000, 1000, 4651


def _gold():
    from helpers import gold
    return gold("toi465_calc_probs.npz")


def _args(kind):
    """arguments of lnZ_TTP ("planet") / lnZ_PEB ("binary": two branches, a companion prior, the contrast curve)"""
    G = _gold()
    base = (G["time"], G["flux"], float(G["sigma"][0]), float(G["P_orb"][0]), float(G["real_stars_mass"][0]),
            float(G["real_stars_rad"][0]), float(G["real_stars_Teff"][0]), 0.0)
    if kind == "planet":
        return "lnZ_TTP", base, dict(N=N_DRAWS, parallel=True)
    return "lnZ_PEB", base + (float(G["real_stars_plx"][0]), os.path.join(GOLD, "toi465_cc.csv"), "TESS"), dict(N=N_DRAWS, parallel=True)


class _device_mode:
    def __enter__(self):
        import triceratops_amd
        triceratops_amd.set_sampling("device")

    def __exit__(self, *exc):
        import triceratops_amd
        from triceratops_amd import fused
        fused.set_thread_seed(None)
        triceratops_amd.set_sampling("numpy")


def _native(kind, rows, extra_flags=0, table_rows=1, moments=False):
    """the library's own call, deferred so that the raw record, posterior block and table can be read:
    (record, block [2][8 + 16 M] or None, table or None, the Pending)"""
    import torch
    from triceratops_amd import _lib, fused
    name, args, kw = _args(kind)
    old = (fused.POSTERIOR_ROWS, fused.TABLE_ROWS, _lib.EXTRA_FLAGS)
    sink = _lib.moments_swap([] if moments else None)
    with _device_mode():
        try:
            fused.POSTERIOR_ROWS, fused.TABLE_ROWS, _lib.EXTRA_FLAGS = rows, table_rows, extra_flags
            fused.set_thread_seed(SEED)
            fused.begin_deferred(1)
            pend = getattr(fused, name)(*args, **kw)
            assert isinstance(pend, fused.Pending)
            fused.flush()
            torch.cuda.synchronize()
            rec = pend.out.numpy().copy()
            post = None if pend.post is None else pend.post.numpy().copy()
            table = None if pend.table is None else pend.table.numpy().copy()
        finally:
            fused.end_deferred()
            _lib.moments_swap(sink)
            fused.POSTERIOR_ROWS, fused.TABLE_ROWS, _lib.EXTRA_FLAGS = old
    return rec, post, table, pend


def _chain(kind, monkeypatch):
    """the operator chain on the same seed: per branch (h, lnprior, idx, cols) of its masked draws, in list order --
    h is trx_lnz_scenario's, every row evaluated to the end"""
    import torch
    from triceratops_amd import _lib, fused
    name, args, kw = _args(kind)
    calls, dump = [], []
    real = _lib.lnz_scenario

    def spy(model, flags, time_d, flux_d, sigma, block, exptime, nsamples, lp, n_total, lnsigma):
        h, lnz = real(model, flags, time_d, flux_d, sigma, block, exptime, nsamples, lp, n_total, lnsigma)
        calls.append((h[:block.shape[1]].cpu().numpy(), None if lp is None else lp.cpu().numpy(), float(lnsigma)))
        return h, lnz

    monkeypatch.setattr(_lib, "lnz_scenario", spy)
    monkeypatch.setattr(fused, "DUMP", dump)
    monkeypatch.setattr(fused, "TABLE_ROWS", 1)
    with _device_mode():
        fused.set_thread_seed(SEED)
        getattr(fused, name)(*args, **kw)
        torch.cuda.synchronize()
    monkeypatch.undo()
    d = dump[0]
    cols = d["cols"].cpu().numpy()
    masks = [d["mask"]] + ([] if d["mask_twin"] is None else [d["mask_twin"]])
    out = []
    for (h, lp, lnsigma), m in zip(calls, masks):
        idx = np.flatnonzero(m.cpu().numpy())
        assert idx.size == h.size
        out.append((h, lp, idx, cols, lnsigma))
    return out


def _check_block(kind, post, pend, chain, M):
    for b, (h, lp, idx, cols, lnsigma) in enumerate(chain):
        blk = post[b]
        hdr, rows = blk[:8], blk[8:].reshape(16, M)
        x, w, C, S, X = yardstick(h, lp, lnsigma)
        assert S > 0 and hdr[3] > 0 and abs(hdr[1] - X) < 1e-9 and np.all(hdr[4:] == 0)
        pos = rows[14].astype(np.int64)
        assert np.array_equal(pos, rows[14])
        accept(pos, hdr[0], w, C, S, M)
        ncol = cols.shape[0]
        want = cols[:, idx[pos]]
        assert want.tobytes() == np.ascontiguousarray(rows[:ncol]).tobytes()      # the gathered columns, bit for bit
        assert np.all(rows[ncol:14] == 0)
        assert np.abs(rows[15] - x[pos]).max() < 1e-9
        # ... and the result dict: the twin branch at 2 P_orb with the orbit of 2 P_orb
        got, ref = pend.scen._posterior(blk, ncol, b == 1), pend.scen._table(want.copy(), 0.0, b == 1)
        for key in ref:
            if key != "lnZ":
                assert np.array_equal(got[key], ref[key]), key
        if b == 1:
            assert np.array_equal(got["P_orb"], 2 * want[2])
        assert np.array_equal(got["row"], pos) and np.array_equal(got["lnw"], rows[15])


@pytest.mark.parametrize("kind", ["planet", "binary"])
def test_scenario_block_against_the_operator_chain(kind, monkeypatch):
    """5 and 7: the native block -- bounded evaluation and TRX_FLAG_FULL_EVALUATION -- against the yardstick fed with the
    operator chain's h, lnprior, list order and columns on the same seed"""
    from triceratops_amd import _lib
    _lib.require_gpu()
    chain = _chain(kind, monkeypatch)
    assert len(chain) == (1 if kind == "planet" else 2)
    for flags in (0, _lib.FLAG_FULL_EVALUATION):
        rec, post, _, pend = _native(kind, M_ROWS, extra_flags=flags)
        _check_block(kind, post, pend, chain, M_ROWS)
    again = _native(kind, M_ROWS)[1]
    nbr = len(chain)
    assert again[:nbr].tobytes() == _native(kind, M_ROWS)[1][:nbr].tobytes()


@pytest.mark.parametrize("kind", ["planet", "binary"])
@pytest.mark.parametrize("moments", [False, True])
def test_record_is_unchanged_by_posterior_rows(kind, moments):
    """6: every slot of the record, both branches, with post_rows = M equals the record without, bit for bit; likewise
    with a table of 100 rows"""
    from triceratops_amd import _lib, fused
    _lib.require_gpu()
    W = fused.SCENARIO_OUT_MOMENTS if moments else fused.SCENARIO_OUT
    nbr, ncol = (1, 11) if kind == "planet" else (2, 14)
    # the slots a record has (include/trx.h): the columns, lnZ, the masked count, [16] ties, [17] status, the moments --
    # a planet's slots 13 .. 15 are never written (whatever the pinned buffer held) -- and the flag behind the records
    slots = [b * W + i for b in range(nbr) for i in list(range(ncol + 2)) + list(range(16, W))] + [2 * W]
    for table_rows in (1, 100):
        r0, _, t0, _ = _native(kind, 0, table_rows=table_rows, moments=moments)
        r1, post, t1, _ = _native(kind, M_ROWS, table_rows=table_rows, moments=moments)
        assert r0[slots].tobytes() == r1[slots].tobytes()
        assert post is not None and np.all(post[:nbr, 3] > 0)
        if table_rows > 1:
            # (of a table the K rows of each column and the K + 1 smallest chi^2 are written)
            K = table_rows
            for b in range(nbr):
                a0, a1 = t0[b].reshape(15, K + 1), t1[b].reshape(15, K + 1)
                assert a0[:ncol, :K].tobytes() == a1[:ncol, :K].tobytes() and a0[14].tobytes() == a1[14].tobytes()


def test_operator_chain_gives_the_same_key(monkeypatch):
    """fused.POSTERIOR_ROWS on the operator chain (trx_posterior_from_halfchi2): same keys, accepted by the yardstick"""
    import torch
    from triceratops_amd import _lib, fused
    _lib.require_gpu()
    chain = _chain("binary", monkeypatch)
    name, args, kw = _args("binary")
    monkeypatch.setattr(fused, "POSTERIOR_ROWS", M_ROWS)
    monkeypatch.setattr(fused, "NATIVE", False)
    monkeypatch.setattr(fused, "TABLE_ROWS", 1)
    with _device_mode():
        fused.set_thread_seed(SEED)
        res = getattr(fused, name)(*args, **kw)
        torch.cuda.synchronize()
    for d, (h, lp, idx, cols, lnsigma) in zip(res, chain):
        post = d["posterior"]
        assert set(post) == set(fused.POSTERIOR_KEYS)
        x, w, C, S, X = yardstick(h, lp, lnsigma)
        assert np.all(w[post["row"]] > 0) and np.all(np.diff(post["row"]) >= 0)
        assert np.array_equal(post["R_EB"], cols[0, idx[post["row"]]])


def _target():
    import pandas as pd
    from triceratops_amd.triceratops import target
    G = _gold()
    cols = ("ID", "Tmag", "Jmag", "Hmag", "Kmag", "ra", "dec", "mass", "rad", "Teff", "plx", "fluxratio", "tdepth")
    st = pd.DataFrame({c: G["real_stars_%s" % c] for c in cols})
    st["ID"] = st["ID"].astype(np.int64)
    return target(270380593, np.array([4]), stars=st, trilegal_fname=os.path.join(GOLD, "trilegal_synth.csv"))


def test_calc_posteriors_equals_calc_probs_and_samples_the_posterior(monkeypatch):
    """8: the 15-scenario TOI-465.01 case from one seed: probabilities, evidences and errors bit for bit; samples exactly
    where lnZ is finite; the TP row's mean R_p against the importance-weighted mean over all of that call's draws"""
    import torch
    import triceratops_amd
    from triceratops_amd import _lib, funcs, fused
    _lib.require_gpu()
    G = _gold()
    call = (G["time"], G["flux"], float(G["sigma"][0]), float(G["P_orb"][0]))
    kw = dict(contrast_curve_file=os.path.join(GOLD, "toi465_cc.csv"), N=N_DRAWS, parallel=True, verbose=0)
    a, b = _target(), _target()
    triceratops_amd.set_sampling("device")
    try:
        torch.manual_seed(465)
        a.calc_probs(*call, **kw)
        torch.manual_seed(465)
        b.calc_posteriors(*call, n_samples=M_ROWS, **kw)
        assert fused.POSTERIOR_ROWS == 0
        for name in ("lnZ", "ess", "lnZ_err"):
            assert np.asarray(getattr(a, name)).tobytes() == np.asarray(getattr(b, name)).tobytes(), name
        assert a.probs.prob.values.tobytes() == b.probs.prob.values.tobytes()
        for col in ("M_s", "R_s", "P_orb", "inc", "b", "ecc", "w", "R_p", "M_EB", "R_EB"):
            assert a.probs[col].values.tobytes() == b.probs[col].values.tobytes(), col
        assert a.FPP == b.FPP and a.NFPP == b.NFPP and a.FPP_err == b.FPP_err
        assert len(b.posterior) == 15
        for j in range(15):
            assert (b.posterior[j] is not None) == bool(np.isfinite(b.lnZ[j])), j
        assert all(p is None for p in a.posterior)
        # the TP call is the pass's first: its draw seed is the first number torch's CPU generator gives after the seed
        torch.manual_seed(465)
        flux, sigma = funcs.renorm_flux(call[1], call[2], float(G["real_stars_fluxratio"][0]))
        dump, calls = [], []
        real = _lib.lnz_scenario

        def spy(*args):
            h, lnz = real(*args)
            calls.append(h[:args[5].shape[1]].cpu().numpy())
            return h, lnz
        monkeypatch.setattr(_lib, "lnz_scenario", spy)
        monkeypatch.setattr(fused, "DUMP", dump)
        monkeypatch.setattr(fused, "TABLE_ROWS", 1)
        fused.lnZ_TTP(call[0], flux, sigma, call[3], float(G["real_stars_mass"][0]), float(G["real_stars_rad"][0]),
                      float(G["real_stars_Teff"][0]), 0.0, N_DRAWS, True, "TESS", False, 0.00139, 20)
        monkeypatch.undo()
    finally:
        triceratops_amd.set_sampling("numpy")
    idx = np.flatnonzero(dump[0]["mask"].cpu().numpy())
    rp = dump[0]["cols"].cpu().numpy()[0, idx]
    x, w, C, S, X = yardstick(calls[0], None, float(np.log(sigma)))
    w = w.astype(np.float64)
    mean = float((w * rp).sum() / w.sum())
    std = float(np.sqrt((w * (rp - mean) ** 2).sum() / w.sum()))
    ess = float(w.sum() ** 2 / (w * w).sum())
    got = float(np.mean(b.posterior[0]["R_p"]))
    print("TP R_p: samples %.6f, weighted mean %.6f, std_w %.4f, ess %.1f (reported %.1f)" % (got, mean, std, ess, b.ess[0]))
    assert abs(ess - b.ess[0]) < 1e-6 * ess
    assert abs(got - mean) < 4 * std / np.sqrt(min(M_ROWS, ess))
    q = b.posterior_summary()
    assert len(q) == int(np.isfinite(b.lnZ).sum()) and abs(q["R_p_q50"][0] - np.median(b.posterior[0]["R_p"])) == 0
