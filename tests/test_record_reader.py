"""The record of a native lnZ_* call (include/trx.h, TRX_SCENARIO_OUT) through its two readers on the host:
fused.Pending.result() (one call -> result dicts) and fused.records_to_rows (a pass -> rows of sharding.run_units' table).
Stub scenarios as in test_mc_error.py, records in which every slot of every branch holds its own value."""
import itertools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from triceratops_amd import _lib, fused, sharding
from triceratops_amd import device_pipeline as dp
from triceratops_amd.constants import Rsun, pi

# The slot of every named column in a branch record, a table block and a posterior block, written down from the
# comment of trx_draw_args.cols in include/trx.h -- on purpose not from fused's own description.  "a": the
# semi-major axis the impact parameter is formed from; the twin branch is the binary at 2 P_orb with the a of 2 P_orb.
SLOT = {"planet": {"R_p": 0, "P_orb": 1, "inc": 2, "a": 3, "R_s": 4, "u1": 5, "u2": 6, "ecc": 7, "argp": 8,
                   "fluxratio_comp": 9, "M_s": 10},
        "binary": {"R_EB": 0, "fluxratio_EB": 1, "P_orb": 2, "inc": 3, "a": 4, "R_s": 5, "u1": 6, "u2": 7, "ecc": 8,
                   "argp": 9, "fluxratio_comp": 10, "M_EB": 12, "M_s": 13}}
SLOT["twin"] = dict(SLOT["binary"], a=11)
NCOL = {"planet": 11, "binary": 14}
K_TABLE, M_POST = 3, 2
CASES = [(kind, stride, K, M) for kind, stride in itertools.product(("planet", "binary"), (18, 20))
         for K, M in ((0, 0), (K_TABLE, 0), (0, M_POST), (K_TABLE, M_POST))]


class _Scen(fused._Scenario):
    """what the readers use of a call drawn from numpy's stream: the kind, and _Scenario's own _table / _posterior"""
    philox = False

    def __init__(self, kind):
        self.a = SimpleNamespace(planet=int(kind == "planet"))

    def run_operator_chain(self, is_host, ncol):
        raise AssertionError("a record without ties was replayed")


def _columns(kind, uid, shape):
    """[ncol, *shape] columns in the library's order, every entry its own finite value; angles and ecc in range"""
    ncol = NCOL[kind]
    step = 1 + 0.01 * uid + 0.001 * np.arange(int(np.prod(shape, dtype=int))).reshape(shape)
    t = np.stack([(1.5 + 0.25 * j) * step for j in range(ncol)])
    s = SLOT[kind]
    t[s["inc"]], t[s["ecc"]], t[s["argp"]], t[s["a"]] = 70 * step, 0.1 * step, 100 * step, 1.1e12 * step
    if kind == "binary":
        t[SLOT["twin"]["a"]] = 1.7e12 * step
    return t


def _pending(kind, stride, K, M, uid, flag=0.0, status=(0.0, 0.0)):
    """a Pending as _Scenario._run_native builds it, and the record's two branches as [2][stride] for the checks"""
    ncol = NCOL[kind]
    rec = torch.zeros(fused.RECORD_MOMENTS, dtype=torch.float64)
    r = rec.numpy()
    table = torch.zeros((2, 15 * (K + 1)), dtype=torch.float64) if K else None
    post = torch.zeros((2, fused._post_branch(M)), dtype=torch.float64) if M else None
    for b in range(2):
        u = 2 * uid + b
        br = r[b * stride:(b + 1) * stride]
        br[:ncol] = _columns(kind, u, ())
        br[ncol], br[ncol + 1] = -10.0 - u, 1000 + u                  # lnZ, masked draws
        br[fused.SCEN_TIES], br[fused.SCEN_STATUS] = 1.0, status[b]
        if stride == fused.SCENARIO_OUT_MOMENTS:
            br[fused.SCEN_LNM2], br[fused.SCEN_LNWMAX] = -7.0 - u, -0.5 - 0.01 * u
        if K:
            blk = table.numpy()[b].reshape(15, K + 1)
            blk[:ncol] = _columns(kind, u, (K + 1,))                   # (draw 0 of the table is the record's best draw)
            blk[14] = 5.0 + u + np.arange(K + 1)                       # chi^2/2: finite, strictly increasing
        if M:
            blk = post.numpy()[b]
            blk[:4] = 0.25 + u, 3.0 + u, 40.0 + u, 2.0 + u             # ([3] > 0: the branch carries weight)
            rows = blk[8:].reshape(16, M)
            rows[:ncol] = 2 * _columns(kind, u, (M,))
            rows[14], rows[15] = 7 * u + np.arange(M), -3.0 - u - 0.5 * np.arange(M)
    r[2 * stride] = flag
    p = fused.Pending(_Scen(kind), rec, None, [object()], ncol, 100 + uid, stride=stride, table=table, table_rows=K,
                      post=post, post_rows=M)
    return p, r[:2 * stride].reshape(2, stride).copy()


@pytest.fixture
def numpy_mode(monkeypatch):
    """a seeded numpy mode: the readers then take the tie-replay decision on every record"""
    monkeypatch.setattr(dp, "RNG", dp.NumpyStreamRng())


def _expected_row(kind, branch, rec):
    """the 15 RECORD_COLS values of one branch record, from SLOT"""
    s = SLOT["twin" if branch == 1 else kind]
    v = {name: rec[j] for name, j in s.items()}
    if branch == 1:
        v["P_orb"] = 2 * v["P_orb"]
    v["b"] = (v["a"] * (1 - v["ecc"] ** 2) / (1 + v["ecc"] * np.sin(v["argp"] * pi / 180)) * np.cos(v["inc"] * pi / 180)
              / (v["R_s"] * Rsun))
    v["lnZ"] = rec[NCOL[kind]]
    return [v.get(c, 0.0) for c in sharding.RECORD_COLS]


def test_one_list_of_columns():
    assert sharding.RECORD_COLS is fused.RECORD_COLS
    assert fused.POSTERIOR_PARAMS == fused.RECORD_COLS[:14]
    assert fused.POSTERIOR_KEYS == fused.RECORD_COLS[:14] + ("lnw", "row")


def test_slot_mapping_and_agreement_of_the_two_readers(numpy_mode):
    """(a) every RECORD_COLS value is the slot trx.h documents for it, b the formula; (b) _record(result()) is the pass's
    row bit for bit, in one mixed pass of planet and binary calls of both strides, the moments behind (NaN at stride
    18); (c) the row's posterior columns decode to result()'s "posterior" """
    made = [_pending(*case, uid) for uid, case in enumerate(CASES)]
    rows = fused.records_to_rows([(k, p) for k, (p, _) in enumerate(made)])
    assert all(p.keep is None for p, _ in made)
    for k, ((kind, stride, K, M), (_, rec)) in enumerate(zip(CASES, made)):
        nbr = 1 if kind == "planet" else 2
        row = rows[k]
        assert row.shape == (nbr, 17 + 16 * M), (k, row.shape)
        for b in range(nbr):
            want = _expected_row(kind, b, rec[b])
            assert np.all(np.isfinite(want)) and len(set(want[:10])) == 10
            assert np.array_equal(row[b, :15], want), (CASES[k], b)
            if stride == 18:
                assert np.all(np.isnan(row[b, 15:17]))
            else:
                assert np.array_equal(row[b, 15:17], rec[b, [fused.SCEN_LNM2, fused.SCEN_LNWMAX]])
        single, _ = _pending(kind, stride, K, M, k)
        res = single.result()
        assert single.keep is None and isinstance(res, tuple) == (kind == "binary")
        assert np.array_equal(sharding._record(res), row[:, :15]), CASES[k]
        dicts = res if isinstance(res, tuple) else (res,)
        layout = sharding.RowLayout(M)
        for b, d in enumerate(dicts):
            assert list(d)[:15] == list(sharding.RECORD_COLS)
            assert all(d[c].shape == (K if K > 1 else 1,) for c in fused.POSTERIOR_PARAMS)
            if not M:
                assert "posterior" not in d
                continue
            got, want = layout.decode(row[b]), d["posterior"]
            assert list(got) == list(want) == list(fused.POSTERIOR_KEYS)
            for key in want:
                assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), (CASES[k], b, key)
            assert np.array_equal(want["row"], 7 * (2 * k + b) + np.arange(M))
            if b == 1:
                assert np.array_equal(want["P_orb"], 2 * single.post.numpy()[1][8:].reshape(16, M)[SLOT["twin"]["P_orb"]])


def test_a_branch_without_weight_has_no_posterior(numpy_mode):
    p, _ = _pending("binary", 20, 0, M_POST, 0)
    p.post.numpy()[1][3] = 0.0
    q, _ = _pending("binary", 20, 0, M_POST, 0)
    q.post.numpy()[1][3] = 0.0
    res = p.result()
    assert res[0]["posterior"] is not None and res[1]["posterior"] is None
    row = fused.records_to_rows([("k", q)])["k"]
    assert np.all(np.isnan(row[1, 17:])) and sharding.RowLayout(M_POST).decode(row[1]) is None


@pytest.mark.parametrize("kind,stride", itertools.product(("planet", "binary"), (18, 20)))
def test_failures_raise_the_same_errors(numpy_mode, kind, stride):
    """(d) a set limb-darkening flag: ValueError from both readers; status 1: TrxError from both -- but not where a
    planet call's record has it in the slot of the twin branch, which a planet call does not have"""
    for reader in ("result", "rows"):
        def read(**kw):
            good, _ = _pending(kind, stride, 0, 0, 0)
            bad, _ = _pending(kind, stride, 0, 0, 1, **kw)
            return bad.result() if reader == "result" else fused.records_to_rows([(0, good), (1, bad)])
        with pytest.raises(ValueError, match="can only convert an array of size 1 to a Python scalar"):
            read(flag=1.0)
        with pytest.raises(_lib.TrxError, match=r"1 lnZ_\* call\(s\) of this pass .* \(branch 0; record status 1\)"):
            read(status=(1.0, 0.0))
        if kind == "planet":
            read(status=(0.0, 1.0))
        else:
            with pytest.raises(_lib.TrxError, match=r"\(branch 1; record status 1\)"):
                read(status=(0.0, 1.0))


def test_statistics_agree(numpy_mode):
    """(e) N single result() calls and one records_to_rows over the same N book the same _lib.STATS"""
    def delta(read):
        before = dict(_lib.STATS)
        read([_pending(*case, uid)[0] for uid, case in enumerate(CASES)])
        return {k: _lib.STATS[k] - before[k] for k in before}
    one_by_one = delta(lambda ps: [p.result() for p in ps])
    in_one_pass = delta(lambda ps: fused.records_to_rows(list(enumerate(ps))))
    assert one_by_one == in_one_pass
    branches = sum(1 if kind == "planet" else 2 for kind, _, _, _ in CASES)
    assert one_by_one["native_calls"] == len(CASES) and one_by_one["launches"] == branches
    assert one_by_one["rows"] == sum(1000 + 2 * uid + b for uid, c in enumerate(CASES) for b in range(1 if c[0] == "planet" else 2))
    assert one_by_one["cells"] == sum((1000 + 2 * uid + b) * (100 + uid)
                                      for uid, c in enumerate(CASES) for b in range(1 if c[0] == "planet" else 2))


def test_moments_reach_the_sink_of_a_direct_call(numpy_mode):
    """result() reports a record's moments to the open sink (sharding.run_units reads them from there), one pair per
    branch in branch order, and none for a record without them; records_to_rows carries them in the rows instead"""
    prev = _lib.moments_swap([])
    try:
        _pending("binary", 18, 0, 0, 0)[0].result()
        assert _lib.moments_since(0) == []
        p, rec = _pending("binary", 20, 0, 0, 1)
        p.result()
        assert _lib.moments_since(0) == [tuple(rec[b, [fused.SCEN_LNM2, fused.SCEN_LNWMAX]]) for b in range(2)]
        fused.records_to_rows([(0, _pending("binary", 20, 0, 0, 2)[0])])
        assert len(_lib.moments_since(0)) == 2
    finally:
        _lib.moments_swap(prev)


def test_a_table_that_does_not_fix_the_order_is_replayed(numpy_mode):
    """the tie-replay decision, the same from both readers: with a table of K rows, K + 1 chi^2 that do not strictly
    increase send the call to the operator chain"""
    for reader in ("result", "rows"):
        p, _ = _pending("planet", 20, K_TABLE, 0, 0)
        p.table.numpy()[0].reshape(15, K_TABLE + 1)[14, 2] = 5.0
        with pytest.raises(AssertionError, match="replayed"):
            p.result() if reader == "result" else fused.records_to_rows([(0, p)])
