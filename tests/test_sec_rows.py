"""The design of tests/sec_rows.py holds, on the CPU oracle alone: the replay of the 25 points is the oracle's secondary
depth, the scan-decided rows have the limit between their centre depth and their scan depth with the stated margin on
either side, every position of the minimum but the centre is there, and O.lnl_batch excludes exactly the kinds that are
designed to be excluded.  Conditions, not measurements: a generator that drifted fails here, before a GPU is asked."""
import numpy as np
import pytest

import sec_rows as S
from oracle import oracle as O
from triceratops_amd import synth

N_MIN = 256            # rows of each scan-decided kind
N_CENTRE_OUT = 8       # ... of which the centre point is exactly out of eclipse (m = 1: the quick test sees depth 0)
REPLAY_TOL = 1e-14     # replay + depth_of against O.flux_grid's secdepth (the same arithmetic: measured 0)


@pytest.mark.parametrize("variant", sorted(S.VARIANTS))
def test_the_replay_is_the_oracles_secondary_depth(variant):
    b = S.blocks(variant)
    for kind in ("scan-excluded", "scan-kept"):
        rows, m = b[kind]["rows"], b[kind]["m"]
        assert np.array_equal(S.replay(rows), m)                       # EB_fr and comp_fr do not enter the curve
        want = S.oracle_depth(rows, b["host"])
        got = S.depth_of(m.min(axis=1), rows[1], rows[10], b["host"])
        assert np.abs(got - want).max() <= REPLAY_TOL, np.abs(got - want).max()
    for kind in ("centre-excluded", "faint"):
        rows = b[kind]["rows"]
        got = S.depth_of(S.replay(rows).min(axis=1), rows[1], rows[10], b["host"])
        assert np.abs(got - S.oracle_depth(rows, b["host"])).max() <= REPLAY_TOL


@pytest.mark.parametrize("variant", sorted(S.VARIANTS))
def test_the_limit_lies_between_centre_and_scan_with_the_margin(variant):
    b = S.blocks(variant)
    has_comp, host = S.VARIANTS[variant]
    assert b["host"] == host
    for kind in S.KINDS:
        rows = b[kind]["rows"]
        assert rows.shape[0] == 11 and np.isfinite(rows).all()
        assert ((rows[1] > 0.0) & (rows[1] < S.EB_FR_MAX)).all(), kind
        assert (np.abs(rows[0] / rows[5] - 1.0) >= 1e-3).all()          # clear of R_EB = R_s
        assert (rows[10] > 0.0).all() if has_comp else (rows[10] == 0.0).all()
    for kind in ("scan-excluded", "scan-kept"):
        rows, m = b[kind]["rows"], b[kind]["m"]
        n = rows.shape[1]
        assert n >= N_MIN, (kind, n)
        argmin = m.argmin(axis=1)
        assert set(argmin) == set(range(S.N_POINTS)) - {S.CENTRE}, sorted(set(argmin))
        assert (m[:, S.CENTRE] == 1.0).sum() >= N_CENTRE_OUT
        dmin, dcen = 1.0 - m.min(axis=1), 1.0 - m[:, S.CENTRE]
        assert (dmin >= S.KEEP_RATIO * dcen).all() and (dmin >= 4.0 * S.L).all()
        scan = S.oracle_depth(rows, host)
        centre = S.depth_of(m[:, S.CENTRE], rows[1], rows[10], host)
        assert (centre <= S.L / S.MARGIN).all(), (kind, centre.max() / S.L)         # open after the quick test
        if kind == "scan-excluded":
            assert (scan >= S.MARGIN * S.L).all(), scan.min() / S.L
        else:
            assert (scan <= S.L / S.MARGIN).all() and (scan >= 0.49 * S.L).all(), (scan.min() / S.L, scan.max() / S.L)
    # the two scan-decided kinds are the same geometries: EB_fr alone moves the verdict
    a, k = b["scan-excluded"]["rows"], b["scan-kept"]["rows"]
    assert np.array_equal(np.delete(a, 1, axis=0), np.delete(k, 1, axis=0)) and (a[1] > k[1]).all()
    # the plain populations: settled by the centre point / far below the limit
    rows = b["centre-excluded"]["rows"]
    centre = S.depth_of(S.replay(rows)[:, S.CENTRE], rows[1], rows[10], host)
    assert rows.shape[1] >= N_MIN and (centre >= 10.0 * S.L).all() and ((rows[1] >= 0.3) & (rows[1] <= 0.5)).all()
    rows = b["faint"]["rows"]
    assert rows.shape[1] >= N_MIN and (rows[1] == 1e-5).all() and (S.oracle_depth(rows, host) <= 0.1 * S.L).all()


@pytest.mark.parametrize("variant", sorted(S.VARIANTS))
def test_the_oracle_excludes_exactly_the_excluded_kinds(variant):
    rows, kind = S.all_rows(variant)
    t = synth.time_grid(48)
    flux = synth.noisy_light_curve(np.random.default_rng(synth.SEED), np.ones(48))
    h = O.lnl_batch(O.MODEL_EB, t, flux, synth.SIGMA, rows, companion_is_host=S.blocks(variant)["host"])
    assert not np.isnan(h).any()
    want = np.isin(kind, [S.KINDS.index(k) for k in S.EXCLUDED_KINDS])
    assert np.array_equal(np.isposinf(h), want)
    assert (h[~want] > 0.0).all()


def test_the_same_seed_gives_the_same_bytes():
    first = {v: S.all_rows(v) for v in S.VARIANTS}
    arranged = S.arrange(S.KINDS, 513, 3, "host")
    S._pool.clear()
    S._blocks.clear()
    for v, (rows, kind) in first.items():
        again, kind2 = S.all_rows(v)
        assert again.tobytes() == rows.tobytes() and np.array_equal(kind, kind2), v
    assert all(np.array_equal(x, y) for x, y in zip(arranged, S.arrange(S.KINDS, 513, 3, "host")))
    assert not np.array_equal(arranged[2], S.arrange(S.KINDS, 513, 4, "host")[2])


@pytest.mark.parametrize("n", [1, 7, 8, 9, 63, 64, 65, 511, 513, 4099])
def test_arrange_deals_every_kind_and_points_into_the_block(n):
    block, block_kind = S.all_rows("companion")
    for kinds in (S.KINDS, S.OPEN_KINDS):
        rows, kind, at = S.arrange(kinds, n, 0, "companion")
        assert rows.shape == (11, n) and kind.shape == at.shape == (n,)
        assert np.array_equal(rows, block[:, at]) and np.array_equal(kind, block_kind[at])
        want = np.bincount([S.KINDS.index(kinds[i % len(kinds)]) for i in range(n)], minlength=len(S.KINDS))
        assert np.array_equal(np.bincount(kind, minlength=len(S.KINDS)), want)
        if n >= 63:
            assert (np.diff(kind) != 0).sum() > n // 4                 # interleaved, not in runs of a kind
    assert S.KINDS[S.arrange(S.KINDS, 1, 0)[1][0]] == "scan-excluded"
