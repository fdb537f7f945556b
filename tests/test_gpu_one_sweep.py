"""One row per wave, full evaluation: pass 2 of cells_kernel takes a row's in-window list in ONE sweep -- a cell next to a
limb contact (no Gauss tier admissible: all S sub-exposures) is evaluated and finalised in the chunk that planned it
instead of being filed for a second sweep (trx_cells.hpp, cells_body; DESIGN 4.1, "one sweep").

Every case runs with the switch on and off (trx_set_one_sweep, testing library) and is compared with the CPU oracle at the
project's bars: 1e-9 relative in chi^2/2, 5e-13 in flux.  "On" is the switch's mode 2, which sends the flux grid and its
evaluation census through the one sweep as well, so that the code can be checked cell by cell; the production library and
the switch's default (mode 1) take one sweep in the likelihood kernels only, because the flux grid's values are on record
bit for bit (tests/golden/window_trips.npz) and a contact cell's last bit can move.  At the default chi^2/2 has the bits
of mode 2 and the flux grid and census those of mode 0.  Between on and off
  * the evaluation census (TRX_FLAG_COUNT_EVALUATIONS) is equal cell for cell;
  * the flux grid is equal bit for bit on every cell that is no contact cell (census neither S nor S + 1);
  * a contact cell may move by CONTACT_ATOL: its sub-exposures step from a centre solution that another plan trip gave
    (kepler_step_wide without FREEZE: a lane takes the steps its trip-mates need), so sin E and cos E of the centre differ
    by a few ulp, 1e-15 at most.  The flux of a sub-exposure on the limb moves by |dF/dz| |dz/dE| dE with dz/dE <= a / R <
    10 on these rows and dF/dz of order k^(1/2) (1 - z^2)^(-1/2) averaged over the S = 20 sub-exposures of which one or two
    sit on the limb: below 1e-13 with room to spare, a fifth of the oracle bar.  chi^2/2 of a row then moves by at most
    sum |f - m| CONTACT_ATOL / sigma^2 over its contact cells plus the reordering of its terms: 1e-11 relative is
    generous and two orders inside the oracle bar.  (Measured on an MI355X, DESIGN 4.1: no cell of these rows' flux
    grids moved at all, chi^2/2 by 2e-16; 5.6e-15 in chi^2/2 over bench.py's 1.8e6 rows);
  * NaN and +inf sit in the same places.

Grids of 400 uniform stamps (seven chunks of 58 owned cells past cells_below = 320), the same 400 stamps jittered (no
stencil: chunks of 64) and 2112 uniform stamps (a window-pass seam at cell 2048), all at 0.05 exposures per step, so that
a contact's run of contact cells is some tens of cells long.  Rows, designed from the window's own rule (a circular
orbit's window is the arc asin((1 + k) / a) either side of conjunction plus half an exposure; contact 2 -- the inner one
of the ingress -- lies where a sin(n t) = 1 - k):
  flat, mid-transit      no contact cell: the body passes the star by / both pairs of contacts beyond the curve
  boundary               k chosen so that contact 2 lies 2.5 cells behind the first chunk boundary of the stencil
                         instantiation (list position 58 + 2.5).  At this cadence the contact cells of contacts 1 and 2
                         form one run (83 cells) from the window's first cell past contact 2: it covers list positions
                         56 .. 64 -- the last owned lanes of chunk 0, its six lent lanes (chunk 1's first) and chunk 1's
                         lane 6 -- and every cell of it is evaluated exactly once (census S, not 2 S).  On the 2112-point
                         grid the grid's conjunction is placed so that the same row's contact 3 lies at cell 2047.5:
                         contact cells either side of the seam
  both-contacts          k = 0.02: contacts 1 and 2 in the first chunk, whose pairs exceed the pair table (checked from
                         the census: more than 640 + one centre per lent lane)
  graze                  b = 1 - k: the disc touches the limb from inside at mid-transit, a run of >= 33 contact cells
  graze-outer            b just inside 1 + k: what is on the disc at all is a contact cell
  nan-dilution, nan-period
  eb-kept, eb-excluded   either side of the secondary rule
and all of them again under TRX_FLAG_ALL_SUBEXPOSURES (every in-window cell S: cell-wise passes throughout) and
TRX_FLAG_NO_STENCIL.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import oracle as O
from triceratops_amd import _lib, synth
from triceratops_amd.constants import Rearth, Rsun

pytestmark = pytest.mark.gpu

CADENCE = 0.05
S = synth.NSAMPLES
PAIRS = 640                    # kCellsPairs
OWNED = 58                     # 64 - kStM: the cells a chunk of the stencil instantiation owns
PASS = 2048
HALF = 150                     # half width of the designed windows, in cells
TWO_PI = 6.283185307179586
RTOL_ORACLE = 1e-9
ATOL_FLUX = 5e-13
CONTACT_ATOL = 1e-13           # see the module's docstring
CONTACT_RTOL_H = 1e-11
K_MID, K_BOTH, K_GRAZE, K_EB, K_EB_DEEP = 0.05, 0.02, 0.1, 0.3, 0.8
BOUNDARY_AT = OWNED + 2.5      # list position of contact 2 of the boundary row

# (name, points, uniform)
GRIDS = (("u400", 400, True), ("i400", 400, False), ("u2112", 2112, True))
IDS = [g[0] for g in GRIDS]
FLAG_SETS = ((0, "plain"), (_lib.FLAG_ALL_SUBEXPOSURES, "all-subexposures"), (_lib.FLAG_NO_STENCIL, "no-stencil"))


def _orbit_for(half_width, k):
    """(P, a / R_s) of a circular orbit whose window has this half width in time: n W = asin((1 + k) / a) + margin."""
    period = TWO_PI * half_width / 0.2
    n = TWO_PI / period
    arc = n * half_width - (0.5 * n * synth.EXPTIME * (1.0 + 1e-9) + 1e-11)
    assert 0.0 < arc < 0.5 * np.pi
    return period, ((1.0 + k) * (1.0 + 1e-9) + 1e-12) / np.sin(arc)


def _contact2(half_width, k):
    """time from contact 2 to conjunction on the orbit _orbit_for gives"""
    per, a_R = _orbit_for(half_width, k)
    return np.arcsin((1.0 - k) / a_R) * per / TWO_PI


def _k_for_contact2(half_width, want):
    lo, hi = 1e-3, 0.9                       # _contact2 falls with k
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if _contact2(half_width, mid) > want:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def _tp_row(k, per, b, a_R, fr=0.0):
    inc = np.degrees(np.arccos(b / a_R))
    return np.array([k * Rsun / Rearth, per, inc, a_R * Rsun, 1.0, 0.4, 0.25, 0.0, 0.0, fr])


def _eb_row(k, eb_fr, per, a_R):
    return np.array([k, eb_fr, per, 90.0, a_R * Rsun, 1.0, 0.4, 0.25, 0.0, 0.0, 0.0])


def _build(n_time, uniform, seed):
    dt = CADENCE * synth.EXPTIME
    hw = HALF * dt
    k_b = _k_for_contact2(hw, (HALF - BOUNDARY_AT) * dt)
    # conjunction in cells: the middle of the short grids; on the long one the boundary row's contact 3 at 2047.5
    centre = 199.5 if n_time < PASS else (PASS - 0.5) - _contact2(hw, k_b) / dt
    t = (np.arange(n_time) - centre) * dt
    if not uniform:
        t = np.sort(t + np.random.default_rng(seed).uniform(-0.3, 0.3, n_time) * dt)
    tp, names = [], []

    def add(name, k, b, half=hw, fr=0.0, per=None):
        p, a_R = _orbit_for(half, k)
        tp.append(_tp_row(k, p if per is None else per, b, a_R, fr))
        names.append(name)

    add("flat", K_MID, 1.5)
    # (contact 2 at (1 - k) / (1 + k) of the window's half width: beyond the curve's end with a third to spare)
    add("mid-transit", K_MID, 0.0, half=1.5 * max(centre, n_time - 1 - centre) * dt)
    add("boundary", k_b, 0.0)
    add("both-contacts", K_BOTH, 0.0)
    add("graze", K_GRAZE, 1.0 - K_GRAZE)
    add("graze-outer", K_GRAZE, (1.0 + K_GRAZE) * (1.0 - 2e-3))
    add("nan-dilution", K_MID, 0.0, fr=np.nan)
    add("nan-period", K_MID, 0.0, per=np.nan)
    eb = []
    for k, eb_fr in ((K_EB, 1e-5), (K_EB_DEEP, 0.4)):
        per, a_R = _orbit_for(hw, k)
        eb.append(_eb_row(k, eb_fr, per, a_R))
    return {"t": t, "dt": dt, "centre": centre, "n": n_time, "uniform": uniform, "k_boundary": k_b,
            "tp": np.ascontiguousarray(np.stack(tp, axis=1)), "tp_names": names,
            "eb": np.ascontiguousarray(np.stack(eb, axis=1)), "eb_names": ["eb-kept", "eb-excluded"]}


@pytest.fixture(scope="module")
def grids():
    """Built once and never changed: per grid the stamps, the rows, a noisy light curve of the boundary row, and what the
    oracle says about all of it."""
    _lib.require_gpu()
    out = {}
    for gi, (name, n_time, uniform) in enumerate(GRIDS):
        g = _build(n_time, uniform, synth.SEED + 1300 + gi)
        r = g["tp_names"].index("boundary")
        curve = O.flux_grid(O.MODEL_TP, g["t"], g["tp"][:, r:r + 1], exptime=synth.EXPTIME, nsamples=S)[0][0]
        g["flux"] = synth.noisy_light_curve(np.random.default_rng(synth.SEED + 1310 + gi), curve)
        for key, omodel in (("tp", O.MODEL_TP), ("eb", O.MODEL_EB)):
            g["oracle_h_" + key] = O.lnl_batch(omodel, g["t"], g["flux"], synth.SIGMA, g[key], exptime=synth.EXPTIME, nsamples=S)
            g["oracle_grid_" + key] = O.flux_grid(omodel, g["t"], g[key], exptime=synth.EXPTIME, nsamples=S)[0]
        g["t_d"], g["f_d"] = _lib.dev(g["t"]), _lib.dev(g["flux"])
        out[name] = g
    return out


BLOCKS = (("tp", _lib.MODEL_TP), ("eb", _lib.MODEL_EB))


def _one_sweep(on):
    """True: one sweep in the likelihood kernels and in the flux grid's (mode 2); False: two sweeps in both (mode 0);
    None: the default, which is what the production library does -- one sweep in the likelihood kernels only (mode 1)"""
    assert _lib.lib().trx_set_one_sweep(1 if on is None else (2 if on else 0)) == 0


def _lnl(g, model, flags, rows_d, out=None):
    return _lib.lnl_batch(model, flags, g["t_d"], g["f_d"], synth.SIGMA, rows_d, synth.EXPTIME, S, out=out)


def _grid(g, model, flags, rows_d):
    return _lib.flux_grid(model, flags, g["t_d"], rows_d, synth.EXPTIME, S, False)[0].cpu().numpy()


def _three(g, model, flags, rows_d):
    """chi^2/2, the flux grid and the evaluation census of one block of rows"""
    return (_lnl(g, model, flags, rows_d).cpu().numpy(), _grid(g, model, flags, rows_d),
            _grid(g, model, flags | _lib.FLAG_COUNT_EVALUATIONS, rows_d))


def _same_bits(a, b):
    return np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _longest_run(mask):
    best = run = 0
    for m in mask:
        run = run + 1 if m else 0
        best = max(best, run)
    return best


def _check_design(g, gname, count):
    """the census of the TP rows (default flags, one sweep) against what the rows were designed for"""
    names = g["tp_names"]
    row = lambda name: count[names.index(name)]
    assert row("flat").max() == 0.0
    mid = row("mid-transit")
    assert mid.min() >= 1.0 and mid.max() < S, "mid-transit: a contact cell after all"
    contact = {name: (row(name) == S) for name in names}
    for name in ("boundary", "both-contacts", "graze", "graze-outer"):
        assert row(name).max() == S, (gname, name)                # contact cells, each evaluated once: never S + 1 or 2 S
        print("%s %s: %d cells evaluated, %d contact cells, longest run %d"
              % (gname, name, (row(name) > 0).sum(), contact[name].sum(), _longest_run(contact[name])))
    assert _longest_run(contact["graze"]) >= 33, (gname, _longest_run(contact["graze"]))
    if g["n"] < PASS:
        first = int(np.ceil(g["centre"] - HALF))                  # the designed windows' first cell: list position 0
        b = contact["boundary"]
        if g["uniform"]:
            # (the window's first cell, from the census: the row's first evaluated cell is list position 0)
            assert np.flatnonzero(row("boundary") > 0)[0] == first, (gname, np.flatnonzero(row("boundary") > 0)[0], first)
            assert b[first + OWNED - 2:first + OWNED + 7].all(), (gname, np.flatnonzero(b) - first)
        # contacts 1 and 2 in the first chunk, and more pairs than the table holds (a lent lane's centre counts on the
        # neighbour's side: at most six of the sum are not this chunk's)
        both = row("both-contacts")
        chunk0 = both[first:first + (OWNED if g["uniform"] else 64)]
        print("%s both-contacts: %d pairs in the first chunk" % (gname, chunk0.sum()))
        assert chunk0.sum() > PAIRS + 6, (gname, chunk0.sum())
        at2 = g["centre"] - _contact2(HALF * g["dt"], K_BOTH) / g["dt"] - first
        assert 0 < at2 < OWNED - 8 and chunk0[0] == S and chunk0[int(at2)] == S, (gname, at2)
    else:
        b = contact["boundary"]
        assert b[PASS - 1] and b[PASS], (gname, np.flatnonzero(b))      # a contact cell on either side of the seam


@pytest.mark.parametrize("flags,fname", FLAG_SETS, ids=[f[1] for f in FLAG_SETS])
@pytest.mark.parametrize("gname", IDS)
def test_one_sweep_against_two_and_the_oracle(grids, gname, flags, fname):
    g = grids[gname]
    try:
        for key, model in BLOCKS:
            r_d = _lib.dev(g[key])
            got = {}
            for on in (True, False):
                _one_sweep(on)
                got[on] = _three(g, model, flags, r_d)
            _one_sweep(True)
            again = _three(g, model, flags, r_d)
            for what, a, b in zip(("chi2/2", "flux grid", "census"), got[True], again):
                assert _same_bits(a, b), (gname, fname, key, what, "two runs with one sweep")
            # the default: the likelihood as with one sweep, the flux grid and its census as with two
            _one_sweep(None)
            dflt = _three(g, model, flags, r_d)
            assert _same_bits(dflt[0], got[True][0]), (gname, fname, key, "chi2/2 at the default")
            assert _same_bits(dflt[1], got[False][1]) and _same_bits(dflt[2], got[False][2]), (gname, fname, key, "grid at the default")
            (h1, f1, c1), (h2, f2, c2) = got[True], got[False]
            assert _same_bits(c1, c2), (gname, fname, key, "census", np.argwhere(c1 != c2)[:8])
            contact = (c1 == S) | (c1 == S + 1)
            if key == "tp" and flags == 0:
                _check_design(g, gname, c1)
            same = (f1.view(np.uint64) == f2.view(np.uint64))
            moved = np.abs(f1 - f2)[contact & ~same]
            fin_h = np.isfinite(h1) & np.isfinite(h2)
            rel_h = np.abs(h1[fin_h] - h2[fin_h]) / np.abs(h2[fin_h])
            print("%s %s %s: %d contact cells, %d of them moved, by %.3g at most; chi2/2 moved by %.3g relative at most"
                  % (gname, fname, key, contact.sum(), moved.size, moved.max() if moved.size else 0.0,
                     rel_h.max() if rel_h.size else 0.0))
            assert same[~contact].all(), (gname, fname, key, "a cell that is no contact cell moved",
                                           np.argwhere(~same & ~contact)[:8])
            assert np.array_equal(np.isnan(f1), np.isnan(f2)) and np.array_equal(np.isnan(h1), np.isnan(h2))
            assert np.array_equal(np.isposinf(h1), np.isposinf(h2))
            assert moved.size == 0 or moved.max() <= CONTACT_ATOL, (gname, fname, key, moved.max())
            assert rel_h.size == 0 or rel_h.max() <= CONTACT_RTOL_H, (gname, fname, key, rel_h.max())
            want, wgrid = g["oracle_h_" + key], g["oracle_grid_" + key]
            known = np.ones(wgrid.shape[0], dtype=bool)
            if key == "tp":
                # (which cells of its flux grid a NaN phase leaves at 1 is not the oracle's to say)
                known[g["tp_names"].index("nan-period")] = False
            fin, gfin = np.isfinite(want), np.isfinite(wgrid)
            for on, (h, flux, count) in got.items():
                assert np.array_equal(np.isnan(want), np.isnan(h)) and np.array_equal(np.isposinf(want), np.isposinf(h))
                assert np.array_equal(np.isnan(wgrid[known]), np.isnan(flux[known]))
                rel = np.abs(h[fin] - want[fin]) / np.abs(want[fin])
                err = np.abs(flux[gfin] - wgrid[gfin]).max()
                print("%s %s %s one sweep %d: chi2/2 vs oracle %.3g, flux vs oracle %.3g" % (gname, fname, key, on, rel.max(), err))
                assert rel.max() < RTOL_ORACLE, (gname, fname, key, on, rel.max())
                assert err < ATOL_FLUX, (gname, fname, key, on, err)
            if key == "tp":
                names = g["tp_names"]
                assert np.isnan(h1[names.index("nan-dilution")]) and np.isnan(h1[names.index("nan-period")])
                if flags & _lib.FLAG_ALL_SUBEXPOSURES:
                    assert set(np.unique(c1)) <= {0.0, float(S)}
            else:
                assert np.isfinite(h1[0]) and np.isposinf(h1[1])
    finally:
        _one_sweep(None)


def test_a_captured_call_replays_to_the_bits_of_an_eager_one(grids):
    g = grids["u2112"]
    r_d = _lib.dev(g["tp"])
    n = g["tp"].shape[1]
    _one_sweep(None)
    eager = _lnl(g, _lib.MODEL_TP, 0, r_d).cpu().numpy()
    out = torch.empty(n, dtype=torch.float64, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _lnl(g, _lib.MODEL_TP, 0, r_d, out=out)             # warm-up
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _lnl(g, _lib.MODEL_TP, 0, r_d, out=out)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert _same_bits(out.cpu().numpy(), eager)
