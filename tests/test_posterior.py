"""Posterior samples, the parts that need no GPU: the ABI's argument checks, the host-side summaries of
target.posterior, and the posterior columns of sharding.run_units' table (world 1 and gloo world 2)."""
import ctypes
import multiprocessing as mp
import os
import socket

import numpy as np
import pytest

from triceratops_amd import sharding

M_FAKE = 5


# ---- 1. ABI ---------------------------------------------------------------------------------------------------------
def test_posterior_from_halfchi2_rejects_bad_arguments_without_a_device():
    from triceratops_amd import _lib, fused
    L = _lib.lib()
    fn = L.trx_posterior_from_halfchi2
    buf = (ctypes.c_double * 16)()
    pos = (ctypes.c_long * 16)()
    big = (ctypes.c_double * (L.trx_workspace_bytes() // 8))()
    ws, nws = ctypes.addressof(big), L.trx_workspace_bytes()
    h, hdr, p = ctypes.addressof(buf), ctypes.addressof(buf), ctypes.addressof(pos)
    assert fn(h, None, 4, 0.0, -1, 1, p, hdr, ws, nws, None) == 1                        # M < 0
    assert fn(h, None, 4, 0.0, _lib.POST_MAX_ROWS + 1, 1, p, hdr, ws, nws, None) == 1    # M above the maximum
    assert fn(h, None, 4, 0.0, 4, 1, None, hdr, ws, nws, None) == 1                      # NULL outputs
    assert fn(h, None, 4, 0.0, 4, 1, p, None, ws, nws, None) == 1
    assert fn(None, None, 4, 0.0, 4, 1, p, hdr, ws, nws, None) == 1                      # rows without values
    assert fn(h, None, -1, 0.0, 4, 1, p, hdr, ws, nws, None) == 1
    assert fn(h, None, 4, 0.0, 4, 1, p, hdr, ws, nws - 8, None) == 3                     # TRX_ERR_WORKSPACE
    assert fn(h, None, 4, 0.0, 4, 1, p, hdr, None, nws, None) == 3
    assert _lib.POST_MAX_ROWS >= 4096 and fused.POST_MAX_ROWS == _lib.POST_MAX_ROWS


def test_struct_and_header_agree_on_the_new_fields():
    from triceratops_amd import _lib, fused
    L = _lib.lib()
    L.trx_scenario_args_size.restype = ctypes.c_size_t
    assert L.trx_scenario_args_size() == ctypes.sizeof(fused.ScenarioArgs)
    names = [f[0] for f in fused.ScenarioArgs._fields_]
    assert names[-3:] == ["post_rows", "post", "post_seed"]
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "trx.h")).read()
    assert "#define TRX_POST_MAX_ROWS %d" % _lib.POST_MAX_ROWS in text
    assert fused._post_branch(7) == 8 + 16 * 7 and "#define TRX_POST_BRANCH(M) (8 + 16 * (M))" in text
    assert fused.POSTERIOR_ROWS == 0
    # the resampler's key comes from the call's seed without touching a generator
    assert fused._mix(123, fused._POST_SALT) == fused._mix(123, fused._POST_SALT) != fused._mix(124, fused._POST_SALT)


# ---- 2. host-side summaries ------------------------------------------------------------------------------------------
def _hand_made_target(n=4000):
    from triceratops_amd import fused
    from triceratops_amd.triceratops import target
    rng = np.random.default_rng(7)
    tg = target.__new__(target)
    prob = np.array([0.6, 0.0, 0.3, 0.1])
    post = []
    for j in range(4):
        d = {k: rng.normal(10.0 * (j + 1), 1.0, n) for k in fused.POSTERIOR_KEYS[:14]}
        d["lnw"], d["row"] = rng.normal(size=n), np.sort(rng.integers(0, 10 ** 5, n))
        post.append(d)
    post[3] = None                      # a row with probability but no samples contributes nothing
    tg.__dict__.update(posterior=post, _pending_finish=None,
                       _probs_columns={"ID": np.arange(4) + 100, "scenario": np.array(["TP", "EB", "PTP", "DTP"]),
                                       "prob": prob})
    return tg, post, prob


def test_posterior_summary_is_np_quantile():
    tg, post, prob = _hand_made_target()
    q = (0.16, 0.5, 0.84)
    tab = tg.posterior_summary(q)
    assert list(tab["scenario"]) == ["TP", "EB", "PTP"] and list(tab["ID"]) == [100, 101, 102]
    for i, j in enumerate((0, 1, 2)):
        for c in ("R_p", "b", "ecc", "M_EB", "fluxratio_comp"):
            want = np.quantile(post[j][c], q)
            assert [tab["%s_q16" % c][i], tab["%s_q50" % c][i], tab["%s_q84" % c][i]] == list(want)
    assert list(tg.posterior_summary((0.025, 0.975)).columns[:5]) == ["ID", "scenario", "prob", "M_s_q2.5", "M_s_q97.5"]


def test_posterior_samples_follow_the_scenario_probabilities():
    tg, post, prob = _hand_made_target()
    n = 100000
    draws = tg.posterior_samples(n, rng=np.random.default_rng(11))
    assert len(draws) == n and "scenario" in draws.columns
    share = np.array([0.6, 0.0, 0.3]) / 0.9           # DTP has no samples: its 0.1 is shared out
    for name, p in zip(("TP", "EB", "PTP"), share):
        got = float(np.mean(draws["scenario"] == name))
        assert abs(got - p) <= 4 * np.sqrt(p * (1 - p) / n), (name, got, p)
    assert not np.any(draws["scenario"] == "DTP")
    # a scenario's rows are draws of ITS samples
    tp = draws[draws["scenario"] == "TP"]
    assert np.all(np.isin(tp["R_p"].to_numpy(), post[0]["R_p"]))
    assert abs(tp["R_p"].mean() - post[0]["R_p"].mean()) < 0.05
    tg.__dict__["posterior"] = None
    with pytest.raises(ValueError):
        tg.posterior_samples(3)


# ---- 3. sharding -----------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _fake_units(M, n_stars=3, drop=("PEB",)):
    """the layout of tests/test_sharding.py's units; results carry a made-up posterior (None for every third row)"""
    from triceratops_amd import fused
    from triceratops_amd.triceratops import _TARGET_CALLS
    units = []

    def thunk(n_res, tag):
        def run():
            out = []
            for r in range(n_res):
                d = {c: np.random.rand(100) + tag for c in sharding.RECORD_COLS if c != "lnZ"}
                d["lnZ"] = float(-50 * np.random.rand() - tag)
                if M and (tag + r) % 3:
                    d["posterior"] = {k: np.random.rand(M) + tag for k in fused.POSTERIOR_KEYS}
                    d["posterior"]["row"] = np.arange(M, dtype=np.int64) * (tag + 1)
                elif M:
                    d["posterior"] = None
                out.append(d)
            return out[0] if n_res == 1 else tuple(out)
        return run

    for key, names, j0, snum in _TARGET_CALLS:
        units.append(sharding.Unit(j0, names, snum, 111, None if key in drop else thunk(len(names), j0), key))
    for i in range(1, n_stars):
        j0 = 15 + 3 * (i - 1)
        units.append(sharding.Unit(j0, ("NTP",), 1, 200 + i, thunk(1, j0), "NTP"))
        units.append(sharding.Unit(j0 + 1, ("NEB", "NEBx2P"), 1, 200 + i, thunk(2, j0 + 1), "NEB"))
    return units


def _run(M, per_unit=True):
    from triceratops_amd import fused
    fused.POSTERIOR_ROWS = M
    sharding.per_unit_seed = per_unit
    try:
        return sharding.run_units(_fake_units(M), verbose=0, as_rows=True)
    finally:
        fused.POSTERIOR_ROWS = 0
        sharding.per_unit_seed = False


def _worker(rank, world, port, q, M):
    import torch.distributed as dist
    import triceratops_amd
    triceratops_amd.set_sampling("numpy")
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sent = []
    real = dist.all_gather_into_tensor

    def spy(out, mine, *a, **k):
        sent.append(int(mine.numel()))
        return real(out, mine, *a, **k)
    dist.all_gather_into_tensor = spy
    np.random.seed(4242)
    res = _run(M, per_unit=False)
    q.put((rank, res, sent))
    dist.barrier()
    dist.destroy_process_group()


def _gloo(M):
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, M)) for r in range(world)]
    for p in procs:
        p.start()
    got = sorted((q.get(timeout=120) for _ in range(world)), key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return got


def _same(a, b):
    return (a is None and b is None) or (a.shape == b.shape and a.tobytes() == b.tobytes())


def test_posterior_columns_travel_in_the_one_gather():
    from triceratops_amd import fused
    narrow = len(sharding.RECORD_COLS) + len(sharding.MOMENT_COLS)
    np.random.seed(4242)
    single = _run(M_FAKE)
    rows = [r for r in single if r is not None]
    assert all(r.shape[1] == narrow + 16 * M_FAKE for r in rows)
    assert any(np.isnan(r[:, narrow:]).all(axis=1).any() for r in rows)                 # rows without samples: NaN
    (_, res0, sent0), (_, res1, sent1) = _gloo(M_FAKE)
    assert len(sent0) == len(sent1) == 1                                               # ONE collective
    for a, b, c in zip(res0, res1, single):
        assert _same(a, b) and _same(a, c)
    # the columns come back as the dicts the units returned
    post = fused.posterior_from_flat(rows[0][0, narrow:], M_FAKE)
    assert post is None or (set(post) == set(fused.POSTERIOR_KEYS) and post["row"].dtype == np.int64)
    np.random.seed(4242)
    sharding.per_unit_seed = True
    fused.POSTERIOR_ROWS = M_FAKE
    try:
        dicts = sharding.run_units(_fake_units(M_FAKE), verbose=0)
    finally:
        sharding.per_unit_seed = False
        fused.POSTERIOR_ROWS = 0
    seen = [d["posterior"] for r in dicts if r is not None for d in r]
    assert any(p is None for p in seen) and any(p is not None for p in seen)
    first = next(p for p in seen if p is not None)
    assert first["R_p"].shape == (M_FAKE,) and np.array_equal(first["row"] % np.maximum(first["row"][1], 1), np.zeros(M_FAKE))


def test_without_posterior_rows_the_table_and_the_message_are_unchanged():
    narrow = len(sharding.RECORD_COLS) + len(sharding.MOMENT_COLS)
    np.random.seed(4242)
    single = _run(0)
    assert all(r.shape[1] == narrow for r in single if r is not None)
    (_, res0, sent0), (_, res1, sent1) = _gloo(0)
    # header row + the larger share of the 17 scenario rows of these units, 17 doubles each
    shares = [sum(len(u.names) for u, o in zip([u for u in _fake_units(0) if u.thunk is not None],
                                                sharding.schedule([sharding.unit_cost(u) for u in _fake_units(0)
                                                                   if u.thunk is not None], 2)) if o == r) for r in range(2)]
    assert sent0 == sent1 == [(1 + max(shares)) * narrow]
    for a, b, c in zip(res0, res1, single):
        assert _same(a, b) and _same(a, c)


def test_batched_passes_refuse_posterior_rows():
    from triceratops_amd import fused
    from triceratops_amd.triceratops import calc_probs_many, target
    fused.POSTERIOR_ROWS = 3
    try:
        with pytest.raises(NotImplementedError):
            calc_probs_many([])
        with pytest.raises(NotImplementedError):
            target.calc_probs_runs(target.__new__(target), None, None, 0.0, 1.0, n_runs=2)
    finally:
        fused.POSTERIOR_ROWS = 0
