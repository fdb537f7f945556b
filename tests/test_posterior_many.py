"""calc_posteriors_many and the summary mode of the sharded table, the parts that need no GPU: the quantile columns of
sharding.run_units (one rank and gloo world 2, the fake units of tests/test_posterior.py), the switch handling and the
argument checks of calc_posteriors_many, deferred tables with quantiles, and the resources of the post_* kernels read
from the built code objects."""
import multiprocessing as mp
import os
import pickle
import re
import subprocess

import numpy as np
import pytest

from triceratops_amd import sharding

from test_posterior import M_FAKE, _fake_units, _free_port, _run, _same

Q = (0.16, 0.5, 0.84)
NARROW = len(sharding.RECORD_COLS) + len(sharding.MOMENT_COLS)


def _run_summary(M, q, per_unit=True, units=None):
    from triceratops_amd import fused
    fused.POSTERIOR_ROWS, fused.POSTERIOR_SUMMARY = M, q
    sharding.per_unit_seed = per_unit
    try:
        return sharding.run_units(_fake_units(M) if units is None else units, verbose=0, as_rows=True)
    finally:
        fused.POSTERIOR_ROWS, fused.POSTERIOR_SUMMARY = 0, None
        sharding.per_unit_seed = False


def _summary_worker(rank, world, port, queue, M, q):
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
    res = _run_summary(M, q, per_unit=False)
    queue.put((rank, res, sent))
    dist.barrier()
    dist.destroy_process_group()


def _gloo_summary(M, q):
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    queue = ctx.Queue()
    procs = [ctx.Process(target=_summary_worker, args=(r, world, port, queue, M, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = sorted((queue.get(timeout=120) for _ in range(world)), key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    return got


# ---- 8. the summary columns travel in the one gather, at their own width ---------------------------------------------
@pytest.mark.parametrize("q", [Q, (0.025, 0.5)])
def test_summary_mode_gathers_quantiles_not_samples(q):
    from triceratops_amd import fused
    width = NARROW + 14 * len(q)
    np.random.seed(4242)
    samples = _run(M_FAKE)                               # the rows with their 16 M sample columns, one rank
    np.random.seed(4242)
    single = _run_summary(M_FAKE, q)
    assert sharding.last_layout.width == width and sharding.last_layout.summary_q == q
    assert len(samples) == len(single)
    with_samples = 0
    for a, b in zip(samples, single):
        assert (a is None) == (b is None)
        if a is None:
            continue
        assert b.shape == (a.shape[0], width)
        assert a[:, :NARROW].tobytes() == b[:, :NARROW].tobytes()
        for i in range(a.shape[0]):
            post = fused.posterior_from_flat(a[i, NARROW:], M_FAKE)
            if post is None:
                assert np.isnan(b[i, NARROW:]).all()
                continue
            with_samples += 1
            want = np.concatenate([np.quantile(post[c], q) for c in fused.POSTERIOR_KEYS[:14]])
            assert want.tobytes() == b[i, NARROW:].tobytes()
    assert with_samples >= 5
    (_, res0, sent0), (_, res1, sent1) = _gloo_summary(M_FAKE, q)
    live = [u for u in _fake_units(M_FAKE) if u[4] is not None]
    owner = sharding.schedule([sharding._COST.get(u[5], 1.0) for u in live], 2)
    shares = [sum(len(u[1]) for u, o in zip(live, owner) if o == r) for r in range(2)]
    assert sent0 == sent1 == [(1 + max(shares)) * width]                               # ONE collective of that width
    for a, b, c in zip(res0, res1, single):
        assert _same(a, b) and _same(a, c)


def test_row_layout_is_the_column_arithmetic_done_by_hand():
    """record 15, moments 2, then 16 M sample columns or 14 len(q) quantile columns, then the histogram words"""
    from triceratops_amd import fused
    plain = sharding.RowLayout()
    assert (plain.record, plain.lnZ, plain.moments, plain.width) == (slice(0, 15), 14, slice(15, 17), NARROW)
    assert plain.extra == plain.hist == slice(NARROW, NARROW) and plain.extra_key is None
    wide = sharding.RowLayout(post_rows=M_FAKE)
    assert wide.extra == slice(NARROW, NARROW + 16 * M_FAKE) and wide.width == NARROW + 16 * M_FAKE
    assert wide.extra_key == "posterior" and wide.summary_q is None
    short = sharding.RowLayout(post_rows=M_FAKE, summary_q=Q, hist=True)
    assert short.extra == slice(NARROW, NARROW + 14 * len(Q)) and short.extra_key == "posterior_quantiles"
    assert short.hist == slice(NARROW + 14 * len(Q), NARROW + 14 * len(Q) + fused.WARP_BRANCH) and short.width == short.hist.stop
    assert sharding.RowLayout(summary_q=Q).width == NARROW                  # (no samples: nothing to summarise)
    with pytest.raises(AttributeError):
        wide.post_rows = 3
    # the extras round-trip, and NaN in the defining slot is None
    post = {k: np.arange(M_FAKE) + 10.0 * i for i, k in enumerate(fused.POSTERIOR_KEYS)}
    row = np.full(wide.width, np.nan)
    assert wide.decode(row) is None
    row[wide.extra] = wide.encode(post)
    back = wide.decode(row)
    assert back["row"].dtype == np.int64 and all(np.array_equal(back[k], post[k]) for k in post)
    assert np.isnan(wide.encode(None)).all() and wide.encode(None).size == 16 * M_FAKE
    pickled = pickle.loads(pickle.dumps(short))
    assert (pickled.extra, pickled.hist, pickled.summary_q) == (short.extra, short.hist, Q)


def test_summary_rows_as_dicts():
    from triceratops_amd import fused
    np.random.seed(4242)
    fused.POSTERIOR_ROWS, fused.POSTERIOR_SUMMARY = M_FAKE, Q
    sharding.per_unit_seed = True
    try:
        dicts = sharding.run_units(_fake_units(M_FAKE), verbose=0)
    finally:
        fused.POSTERIOR_ROWS, fused.POSTERIOR_SUMMARY = 0, None
        sharding.per_unit_seed = False
    seen = [d for r in dicts if r is not None for d in r]
    assert all("posterior" not in d for d in seen)
    assert any(d["posterior_quantiles"] is None for d in seen)
    first = next(d["posterior_quantiles"] for d in seen if d["posterior_quantiles"] is not None)
    assert set(first) == set(fused.POSTERIOR_KEYS[:14]) and first["R_p"].shape == (len(Q),)


# ---- 9. calc_posteriors_many: the module switches, the argument checks ------------------------------------------------
def _stub_target(M, fail=False):
    """a target whose work units are the fake ones (21 scenario rows)"""
    from triceratops_amd.triceratops import target
    tg = target.__new__(target)

    def prepare(job=0, **kw):
        units = _fake_units(M)
        if fail:
            def boom():
                raise RuntimeError("a unit failed")
            units[0] = units[0][:4] + (boom,) + units[0][5:]
        return units, 21
    tg._prepare = prepare
    return tg


def test_calc_posteriors_many_restores_the_switches_and_checks_its_arguments():
    import triceratops_amd
    from triceratops_amd import fused
    from triceratops_amd.triceratops import calc_posteriors_many, calc_probs_many
    assert triceratops_amd.calc_posteriors_many.__doc__
    assert fused.POSTERIOR_ROWS == 0 and fused.POSTERIOR_SUMMARY is None
    np.random.seed(3)
    out = calc_posteriors_many([(_stub_target(M_FAKE), {}), (_stub_target(M_FAKE), {})], n_samples=M_FAKE)
    assert fused.POSTERIOR_ROWS == 0 and fused.POSTERIOR_SUMMARY is None
    assert len(out) == 2
    for tg in out:
        assert tg.posterior_quantiles is None and len(tg.posterior) == 21
        assert any(p is not None and p["R_p"].shape == (M_FAKE,) for p in tg.posterior)
    fused.POSTERIOR_ROWS = 2                                 # (a user's own setting comes back, too)
    try:
        with pytest.raises(RuntimeError, match="a unit failed"):
            calc_posteriors_many([(_stub_target(M_FAKE, fail=True), {})], n_samples=M_FAKE, keep="summary")
        assert fused.POSTERIOR_ROWS == 2 and fused.POSTERIOR_SUMMARY is None
        with pytest.raises(NotImplementedError):
            calc_probs_many([])                              # the user's switch still shuts the plain batch
    finally:
        fused.POSTERIOR_ROWS = 0
    for bad in (0, -1, fused.POST_MAX_ROWS + 1):
        with pytest.raises(ValueError):
            calc_posteriors_many([], n_samples=bad)
    with pytest.raises(ValueError):
        calc_posteriors_many([], keep="quantiles")
    with pytest.raises(ValueError):
        calc_posteriors_many([], keep="summary", q=())
    assert fused.POSTERIOR_ROWS == 0 and fused.POSTERIOR_SUMMARY is None
    assert calc_posteriors_many([]) == []


def test_a_sampling_mode_without_posterior_rows_raises(monkeypatch):
    """the numpy mode's evidences return no posterior rows: calc_posteriors_many says so, as calc_posteriors does"""
    from helpers import install_cpu_device_fakes
    from test_sharding import _two_jobs
    from triceratops_amd import fused
    from triceratops_amd.triceratops import calc_posteriors_many
    install_cpu_device_fakes(monkeypatch)
    np.random.seed(5)
    with pytest.raises(NotImplementedError, match="device paths"):
        calc_posteriors_many(_two_jobs(), n_samples=10)
    assert fused.POSTERIOR_ROWS == 0 and fused.POSTERIOR_SUMMARY is None
    tg = _two_jobs()[0][0]
    np.random.seed(5)
    kw = _two_jobs()[0][1]
    with pytest.raises(NotImplementedError, match="device paths"):
        tg.calc_posteriors(kw["time"], kw["flux_0"], kw["flux_err_0"], kw["P_orb"], n_samples=10,
                           **{k: v for k, v in kw.items() if k not in ("time", "flux_0", "flux_err_0", "P_orb")})


# ---- 6 (host half). keep="summary" is np.quantile of keep="samples" ---------------------------------------------------
def test_summary_equals_the_quantiles_of_the_samples_and_the_frames_agree():
    from triceratops_amd import fused
    from triceratops_amd.triceratops import calc_posteriors_many
    np.random.seed(8)
    a, = calc_posteriors_many([(_stub_target(M_FAKE), {})], n_samples=M_FAKE)
    np.random.seed(8)
    b, = calc_posteriors_many([(_stub_target(M_FAKE), {})], n_samples=M_FAKE, keep="summary", q=Q)
    assert b.posterior is None and len(b.posterior_quantiles) == 21
    assert np.array_equal(a.lnZ, b.lnZ) and a.FPP == b.FPP
    for p, s in zip(a.posterior, b.posterior_quantiles):
        assert (p is None) == (s is None)
        if p is not None:
            for c in fused.POSTERIOR_KEYS[:14]:
                assert np.array_equal(np.quantile(p[c], Q), s[c]), c
    fa, fb = a.posterior_summary(Q), b.posterior_summary(Q)
    assert len(fa) > 0 and list(fa.columns) == list(fb.columns)
    assert fa.equals(fb)
    with pytest.raises(ValueError, match="quantiles"):
        b.posterior_summary((0.1, 0.9))
    with pytest.raises(ValueError, match="quantiles only"):
        b.posterior_samples(3)


# ---- 10. deferred tables ----------------------------------------------------------------------------------------------
def test_a_deferred_table_with_quantiles_pickles():
    from triceratops_amd.triceratops import target
    np.random.seed(21)
    units = _fake_units(M_FAKE)
    res = _run_summary(M_FAKE, Q, per_unit=False, units=units)
    for name in ("posterior", "posterior_quantiles"):
        assert name in target._RESULTS
    now = target.__new__(target)
    layout = sharding.RowLayout(post_rows=M_FAKE, summary_q=Q)
    now._finish(units, res, 21, layout=layout)
    later = target.__new__(target)
    later.posterior = "stale"
    later._defer_finish(units, res, 21, layout)
    assert later.__dict__.get("_pending_finish") is not None and "posterior" not in later.__dict__
    clone = pickle.loads(pickle.dumps(later))
    assert clone.__dict__.get("_pending_finish") is None
    again = target.__new__(target)
    again._defer_finish(units, res, 21, layout)
    assert again.posterior is None                           # (reading a result fills the table)
    for tg in (clone, again):
        assert tg.posterior is None and len(tg.posterior_quantiles) == 21
        for x, y in zip(tg.posterior_quantiles, now.posterior_quantiles):
            assert (x is None) == (y is None)
            if x is not None:
                assert all(np.array_equal(x[c], y[c]) for c in y)
        assert tg.posterior_summary(Q).equals(now.posterior_summary(Q))
        assert np.array_equal(tg.lnZ, now.lnZ)
    assert any(x is not None for x in now.posterior_quantiles)


def test_a_deferred_table_with_samples_serves_summary_and_samples_at_first_read():
    """calc_posteriors_many(keep="samples") on several ranks leaves the targets of other ranks deferred: posterior_summary
    and posterior_samples must fill the table themselves, as the first thing read, also on a pickled clone"""
    from triceratops_amd.triceratops import target
    np.random.seed(22)
    units = _fake_units(M_FAKE)                          # (the layout; _run evaluates units of its own, laid out alike)
    res = _run(M_FAKE, per_unit=False)
    layout = sharding.RowLayout(post_rows=M_FAKE)
    now = target.__new__(target)
    now._finish(units, res, 21, layout=layout)
    want_frame = now.posterior_summary(Q)
    want_draws = now.posterior_samples(40, rng=np.random.default_rng(5))
    assert len(want_frame) > 0 and len(want_draws) == 40

    def deferred():
        tg = target.__new__(target)
        tg._defer_finish(units, res, 21, layout)
        assert tg.__dict__.get("_pending_finish") is not None and "posterior" not in tg.__dict__
        return tg
    first = deferred()
    assert first.posterior_samples(40, rng=np.random.default_rng(5)).equals(want_draws)
    assert first.__dict__.get("_pending_finish") is None and first.posterior_quantiles is None
    second = deferred()
    assert second.posterior_summary(Q).equals(want_frame)
    clone = pickle.loads(pickle.dumps(deferred()))
    assert clone.posterior_samples(40, rng=np.random.default_rng(5)).equals(want_draws)
    assert clone.posterior_summary(Q).equals(want_frame)
    for x, y in zip(clone.posterior, now.posterior):
        assert (x is None) == (y is None)
        if x is not None:
            assert all(np.array_equal(x[c], y[c]) for c in y)


# ---- 11. resources of the posterior kernels ---------------------------------------------------------------------------
def test_posterior_kernels_use_no_scratch_and_the_chain_forms_stay_within_the_single_call_budget(tmp_path):
    """0 B of scratch for every post_* kernel; the chain forms within 33 KB of LDS and 90 VGPRs"""
    from test_build_resources import READELF, _device_objects
    from triceratops_amd import _lib
    if not os.path.exists(READELF):
        pytest.skip("llvm-readelf not installed")
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libtrx.so not built")
    seen = set()
    for k, obj in enumerate(_device_objects(_lib.LIB_PATH)):
        f = tmp_path / ("dev%d.co" % k)
        f.write_bytes(obj)
        notes = subprocess.run([READELF, "--notes", str(f)], capture_output=True, text=True, check=True).stdout
        for blk in re.split(r"\n\s+- \.agpr_count", notes)[1:]:
            name = re.search(r"\.name:\s+(\S+)", blk).group(1)
            if "post_" not in name or "_kernel" not in name:
                continue

            def field(key):
                return int(re.search(r"\.%s:\s+(\d+)" % key, blk).group(1))
            short = re.search(r"(post_\w+?_kernel)", name).group(1)
            seen.add(short)
            print(short, "scratch", field("private_segment_fixed_size"), "VGPRs", field("vgpr_count"), "LDS",
                  field("group_segment_fixed_size"))
            assert field("private_segment_fixed_size") == 0, "%s uses scratch" % name
            if "chain" in short:
                assert field("vgpr_count") <= 90, "%s needs %d VGPRs" % (name, field("vgpr_count"))
                assert field("group_segment_fixed_size") <= 33 * 1024, name
    assert {"post_max_kernel", "post_x_kernel", "post_sum_kernel", "post_select_kernel", "post_sum_chain_kernel",
            "post_select_chain_kernel"} <= seen
