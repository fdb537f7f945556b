"""softmin_rows_kernel<J> (trxt_softmin_rows, include/trx_shift.h): the soft minimum of J candidate
values per row, T = -ln sum_j exp(lnc_j - cand[j][r]), against _numerics.t0_mix_halfchi2 in long double.

Shapes: n in {1, 2, 63, 64, 65, 257, 100 003} (one lane, a partial wave, the wave and block seams, more than one block, 391
blocks; the cap of 4096 blocks is crossed once, at 4096 x 256 + 5 rows, for one J), J in {1, 2, 3, 8}, the rows of `cand`
packed (stride = n) and three
doubles apart (stride = n + 3, the gap filled with NaN), values of size 0, about 50 and about 5000, the log-weights a
normalised grid's own and a set that makes the J terms equal at row 0.

Bar, not chosen from results: |d T| <= 16 eps (1 + |T| + max_j |lnc_j|).  a_j = cand_j - lnc_j and m - a_j carry eps |a| each,
at most 8 exponentials and one log a couple of ulp each, the soft minimum is 1-Lipschitz in a; 16 is twice that count.
Where the statement says bits -- one node, nodes that cannot reach the sum, the same row elsewhere -- bits are compared."""
import numpy as np
import pytest
import torch

from triceratops_amd import _lib, _numerics

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
INF = float("inf")
NAN = float("nan")
SIZES = (1, 2, 63, 64, 65, 257, 100003)
NODES = (1, 2, 3, 8)
SCALES = (0.0, 50.0, 5000.0)
_worst = [0.0]


def _values(J, n, scale, seed):
    rng = np.random.default_rng(seed)
    return np.abs(scale + 3.0 * rng.normal(size=(J, n))) if scale else np.zeros((J, n))


def _weights(J, h, kind, seed):
    if kind == "grid":
        w = np.random.default_rng(seed).uniform(0.1, 1.0, J)
        return np.log(w / w.sum())
    return h[:, 0] - h[:, 0].min() - 1.0                  # (cand_j - lnc_j the same for every node at row 0)


def _on_device(h, stride):
    """[J][n] view of a [J][stride] device buffer whose gap holds NaN"""
    J, n = h.shape
    buf = torch.full((J, stride), NAN, dtype=torch.float64, device="cuda")
    view = buf[:, :n]
    view.copy_(torch.from_numpy(np.ascontiguousarray(h)))
    assert view.stride(0) == stride or J == 1
    return view


def _run(h, lnc, stride=None, out=None):
    got = _lib.softmin_rows(_on_device(h, h.shape[1] if stride is None else stride), lnc, out=out)
    torch.cuda.synchronize()
    return got.cpu().numpy()


def _same(a, b):
    """the same bits; a NaN matches a NaN (its payload is not part of the statement)"""
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and a[~nan].tobytes() == b[~nan].tobytes()


def _check(got, h, lnc, what):
    want = _numerics.t0_mix_halfchi2(h.astype(np.longdouble), lnc)
    bar = 16 * EPS * (1.0 + np.abs(want) + np.abs(lnc).max())
    err = np.abs(got - want)
    frac = float(np.max(err / bar))
    _worst[0] = max(_worst[0], frac)
    print("%s: max |d T| / bar %.3g (largest so far %.3g)" % (what, frac, _worst[0]))
    assert (err <= bar).all(), what
    assert (got >= 0).all(), what


@pytest.mark.parametrize("J", NODES)
@pytest.mark.parametrize("n", SIZES)
def test_against_the_long_double_statement(n, J):
    for scale in SCALES:
        h = _values(J, n, scale, 1000 * J + n)
        for kind in ("grid", "balanced"):
            lnc = _weights(J, h, kind, n + J)
            packed = _run(h, lnc)
            _check(packed, h, lnc, "n %d J %d h ~ %g %s" % (n, J, scale, kind))
            apart = _run(h, lnc, stride=n + 3)
            assert apart.tobytes() == packed.tobytes(), "the stride entered a row's bits"


def test_rows_beyond_the_capped_grid():
    n, J = 4096 * 256 + 5, 3
    h = _values(J, n, 50.0, 7)
    lnc = _weights(J, h, "grid", 7)
    got = _run(h, lnc)
    _check(got, h, lnc, "n %d J %d" % (n, J))
    # a lane's second trip computes what its first would: the last rows' values at the front give the last rows' bits
    assert _run(np.ascontiguousarray(h[:, -5:]), lnc).tobytes() == got[-5:].tobytes()


def _with_specials(h):
    h = h.copy()
    if h.shape[1] > 1:
        h[:, 1] = INF
    if h.shape[1] > 2:
        h[0, 2] = NAN
    return h


@pytest.mark.parametrize("n", SIZES)
def test_one_node_at_zero_returns_the_input_bits(n):
    h = _with_specials(_values(1, n, 50.0, n))
    for stride in (n, n + 3):
        assert _same(_run(h, np.zeros(1), stride=stride), h[0])


@pytest.mark.parametrize("J", NODES[1:])
@pytest.mark.parametrize("n", (1, 65, 100003))
def test_nodes_that_cannot_reach_the_sum_leave_the_other_nodes_bits(n, J):
    for scale in SCALES:
        h = _values(J, n, scale, 31 * J + n)
        for node in (0, J - 1):
            for far in (-800.0, -INF):
                lnc = np.full(J, far)
                lnc[node] = 0.0
                assert _run(h, lnc).tobytes() == h[node].tobytes(), (scale, node, far)
    # ... also where that node is excluded (a NaN there meets m = +inf of the others: the statement stores m)
    h = _values(J, max(n, 3), 50.0, n)
    h[:, 1] = INF
    h[0, 2] = INF
    lnc = np.full(J, -INF)
    lnc[0] = 0.0
    assert _run(h, lnc).tobytes() == h[0].tobytes()


@pytest.mark.parametrize("J", NODES[1:])
def test_permuted_nodes_agree_within_the_bar(J):
    n = 257
    for scale in SCALES:
        h = _values(J, n, scale, 77 + J)
        lnc = _weights(J, h, "grid", J)
        a = _run(h, lnc)
        for perm in (np.arange(J)[::-1], np.roll(np.arange(J), 1)):
            b = _run(np.ascontiguousarray(h[perm]), lnc[perm])
            bar = 16 * EPS * (1.0 + np.abs(a) + np.abs(lnc).max())
            print("J %d h ~ %g: permuted, max |d T| / bar %.3g" % (J, scale, float(np.max(np.abs(a - b) / bar))))
            assert (np.abs(a - b) <= bar).all()


@pytest.mark.parametrize("J", NODES)
def test_a_rows_bits_do_not_depend_on_where_it_stands(J):
    rng = np.random.default_rng(J)
    row = np.abs(50.0 + 3.0 * rng.normal(size=J))
    lnc = _weights(J, row[:, None], "grid", J)
    alone = _run(row[:, None].copy(), lnc)
    assert alone.shape == (1,)
    for n in (257, 100003):
        h = _values(J, n, 5000.0, n + J)
        h[:, 0] = row
        h[:, n - 1] = row
        h[:, 100] = row
        for stride in (n, n + 3):
            got = _run(h, lnc, stride=stride)
            assert got[0].tobytes() == got[n - 1].tobytes() == got[100].tobytes() == alone[0].tobytes()
            assert _run(h, lnc, stride=stride).tobytes() == got.tobytes(), "a second run gave other bits"


@pytest.mark.parametrize("J", NODES)
def test_accumulate_excluded_rows_and_nan_rows(J):
    n = 300
    h = _values(J, n, 50.0, 9 * J)
    h[:, 5] = INF                                            # every node excluded
    h[0, 6] = NAN                                            # a NaN among a row's values
    h[:, 7] = NAN
    if J > 1:
        h[1:, 8] = INF                                       # one node left
        h[0, 9] = INF                                        # one node excluded
    lnc = _weights(J, h, "grid", J)
    t = _run(h, lnc)
    assert t[5] == INF and np.isnan(t[6]) and np.isnan(t[7])
    ok = np.ones(n, dtype=bool)
    ok[[5, 6, 7]] = False
    assert np.isfinite(t[ok]).all()
    _check(t[ok], h[:, ok], lnc, "J %d with excluded nodes" % J)
    if J > 1:
        one = _numerics.t0_mix_halfchi2(h[:1, 8:9].astype(np.longdouble), lnc[:1])[0]
        assert abs(t[8] - one) <= 16 * EPS * (1.0 + abs(one) + np.abs(lnc).max())
    # added to what is there: finite, +inf and NaN
    before = np.abs(np.random.default_rng(J).normal(size=n)) * 100.0
    before[10], before[11], before[5], before[6] = INF, NAN, 3.0, 4.0
    out = torch.from_numpy(before.copy()).cuda()
    got = _run(h, lnc, out=out)
    assert _same(out.cpu().numpy(), got), "out is the tensor given"
    with np.errstate(invalid="ignore"):
        want = before + t
    assert _same(got, want)
    assert got[10] == INF and np.isnan(got[11]) and got[5] == INF and np.isnan(got[6])
    # +inf stays +inf also where the row's own value is +inf
    out = torch.full((n,), INF, dtype=torch.float64, device="cuda")
    got = _run(h, lnc, out=out)
    assert np.array_equal(np.isnan(got), np.isnan(t)) and (got[~np.isnan(t)] == INF).all()
    # no rows: nothing to do, no address to pass
    empty = _lib.softmin_rows(torch.empty((J, 0), dtype=torch.float64, device="cuda"), lnc)
    assert empty.shape == (0,)
