"""Stencil instantiation of the one-row likelihood kernels: every chunk of pass 2 takes 64 NEW entries of the in-window list
(trx_cells.hpp, cells_body, "full chunks") instead of 56 plus 8 lent lanes that the next chunk plans and
evaluates again.  A stencil cell of a chunk's last 8 lanes is "pending": it is finalised by the next chunk, which owes it
a centre value for each of its first cells, whatever their kind.

Every case runs with trx_set_full_chunks at 0 (the one-sided halo) and at 2 (full chunks in the flux grid and its evaluation
census too, so that the code can be checked cell by cell), both with trx_set_one_sweep(2) so that the chunking is the only
difference, and is compared with the CPU oracle at the project's bars (tests/test_gpu_one_sweep.py: 1e-9 relative in
chi^2/2, 5e-13 in flux).  The census (TRX_FLAG_COUNT_EVALUATIONS) tells a cell's kind: 1 or 2 a stencil cell (2: the halo
path's lent lanes, whose centre two chunks evaluate), 3 .. 10 Gauss nodes (+ 1 with a centre for a neighbour), S a contact
cell (S + 1: one that delivered an owed centre).

Between the modes
  * a cell that changes kind (stencil <-> own nodes: only within 8 lanes of a chunk edge of either chunking) is left out
    of the cell-by-cell comparison -- never out of the oracle's --, at most 16 per full-chunk edge (asserted);
  * every other cell may differ by its neighbours' trip-mates in the plan's Kepler step only: MOVED_FLUX below is four
    times what one run on one MI355X measured on these cases (1.11e-16, see the constant), far inside CONTACT_ATOL;
  * chi^2/2 moves by its terms' order and the seam cells' kind: MOVED_H, four times the measured 2.76e-15 relative, far
    inside the project's CONTACT_RTOL_H;
  * no cell costs more with full chunks than with the halo, except the first cells of a chunk whose left neighbours left
    no centre value (the named cases).

Grids at 0.25 exposures per step (a stencil cell is >= 36 cells from a limb contact, a contact cell within 4), conjunction
at a half-integer cell so that a designed window of half width H cells holds exactly 2 H cells and list position = cell -
first:
  wide-N     N = 384 + r stamps, r = 0, 1, 7, 8, 9, 56, 63, one row whose window is wider than the curve: the list is the
             whole curve, every cell but the first and last 8 a stencil cell; r = 0 has pending candidates in the list's
             last lanes and no next chunk; the 384 grid also holds a row whose whole list is 60 cells
  main       1024 stamps, windows of 400 cells (7 chunks): sixteen rows whose contact 2 moves through the list in steps
             of 4 cells -- the contact run's end, the first st_ok cell, the last one and the egress run's start each visit
             every lane of a chunk, lanes 56 .. 63 and 0 .. 7 among them --, an eccentric row and the wide row
  epochs     2048 stamps, period 1700 cells (long enough for the stencil's radius test to pass between the contacts): two
             windows in one list, the jump at a chunk edge (192) and inside one (200)
  seam       4097 stamps, conjunction at cell 2047.5: stencil cells either side of the window-pass seam
"""
import os

import numpy as np
import pytest

from oracle import oracle as O
from test_build_resources import READELF, instantiations, kernel_resources
from test_gpu_one_sweep import CONTACT_ATOL, CONTACT_RTOL_H, RTOL_ORACLE, ATOL_FLUX
from triceratops_amd import _lib, synth
from triceratops_amd.constants import Rearth, Rsun

CADENCE = 0.25                 # within [1 / 9, 0.3] exposures per step, where the stencil applies (rowc_kernel)
S = synth.NSAMPLES
DT = CADENCE * synth.EXPTIME
TWO_PI = 6.283185307179586
PASS = 2048
ST_M = 8                       # kStM
# Measured on one MI355X, one run, over all cases below: the largest |flux(full chunks) - flux(halo)| of a cell that keeps
# its kind is 1.11e-16 (one ulp, on the eccentric row of `main`; 0 on every circular row), the largest relative change of
# chi^2/2 2.76e-15 (the weighted case; 6.6e-16 unweighted).  Asserted at four times that: lane placement varies with the list.
MEASURED_FLUX = 1.11e-16
MEASURED_H = 2.76e-15
MOVED_FLUX = 4.0 * MEASURED_FLUX
MOVED_H = 4.0 * MEASURED_H
assert MOVED_FLUX <= CONTACT_ATOL and MOVED_H <= CONTACT_RTOL_H


def _orbit(half_width, k, period=None):
    """(P, a / R_s) of a circular orbit whose window has this half width in time (the window's own rule, as in
    tests/test_gpu_one_sweep.py), at a period of the caller's choice"""
    if period is None:
        period = TWO_PI * half_width / 0.2
    n = TWO_PI / period
    arc = n * half_width - (0.5 * n * synth.EXPTIME * (1.0 + 1e-9) + 1e-11)
    assert 0.0 < arc < 0.5 * np.pi
    return period, ((1.0 + k) * (1.0 + 1e-9) + 1e-12) / np.sin(arc)


def _contact2(half_width, k):
    per, a_R = _orbit(half_width, k)
    return np.arcsin((1.0 - k) / a_R) * per / TWO_PI


def _k_for_contact2(half_width, want):
    lo, hi = 1e-3, 0.9
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if _contact2(half_width, mid) > want:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def _tp_row(k, per, a_R, ecc=0.0, argp=0.0):
    return np.array([k * Rsun / Rearth, per, 90.0, a_R * Rsun, 1.0, 0.4, 0.25, ecc, argp, 0.0])


def _windows(n_time, centres, half):
    """the designed list of a row: (first cell, cells) of each window, clipped to the curve"""
    out = []
    for c in centres:
        lo, hi = int(np.ceil(c - half)), int(np.floor(c + half))
        lo, hi = max(lo, 0), min(hi, n_time - 1)
        if hi >= lo:
            out.append((lo, hi - lo + 1))
    return out


def _positions(n_time, windows):
    """list position of every cell in its window pass (-1: not in the list)"""
    pos = np.full(n_time, -1)
    for p0 in range(0, n_time, PASS):
        at = 0
        for lo, cnt in windows:
            for cell in range(max(lo, p0), min(lo + cnt, p0 + PASS, n_time)):
                pos[cell] = at
                at += 1
    return pos


def _case(name, n_time, centre, rows):
    """rows: (name, k, half width in cells or None = wider than the curve, period in cells or None, ecc, argp)"""
    t = (np.arange(n_time) - centre) * DT
    params, names, lists = [], [], []
    for rname, k, half, pcells, ecc, argp in rows:
        if half is None:
            per, a_R = _orbit(1.5 * max(centre, n_time - 1 - centre) * DT, k)
            wins = [(0, n_time)]
        else:
            per, a_R = _orbit(half * DT, k, None if pcells is None else pcells * DT)
            centres = [centre] if pcells is None else [centre + m * pcells for m in range(-1, 3)]
            wins = _windows(n_time, centres, half)
        params.append(_tp_row(k, per, a_R, ecc, argp))
        names.append(rname)
        lists.append(None if ecc else _positions(n_time, wins))          # (an eccentric row's window is the library's to say)
    return {"name": name, "n": n_time, "t": t, "names": names, "pos": lists,
            "tp": np.ascontiguousarray(np.stack(params, axis=1))}


HALF_MAIN = 200
SHIFTS = tuple(20 + 4 * i for i in range(16))          # list position of contact 2


def _cases():
    out = []
    for r in (0, 1, 7, 8, 9, 56, 63):
        rows = [("wide", 0.05, None, None, 0.0, 0.0)]
        if r == 0:
            rows.append(("short", 0.05, 30, None, 0.0, 0.0))
        out.append(_case("wide-%d" % (384 + r), 384 + r, 191.5, rows))
    rows = [("shift-%d" % p2, _k_for_contact2(HALF_MAIN * DT, (HALF_MAIN - p2) * DT), HALF_MAIN, None, 0.0, 0.0)
            for p2 in SHIFTS]
    rows.append(("eccentric", 0.05, None, None, 0.3, 90.0))
    rows.append(("wide", 0.05, None, None, 0.0, 0.0))
    out.append(_case("main", 1024, 511.5, rows))
    out.append(_case("epochs", 2048, 150.5, [("edge", 0.05, 96, 1700, 0.0, 0.0), ("inside", 0.05, 100, 1700, 0.0, 0.0)]))
    out.append(_case("seam", 4097, 2047.5, [("seam", 0.05, 150, None, 0.0, 0.0), ("wide", 0.05, None, None, 0.0, 0.0)]))
    return out


CASE_NAMES = ["wide-%d" % (384 + r) for r in (0, 1, 7, 8, 9, 56, 63)] + ["main", "epochs", "seam"]


@pytest.fixture(scope="module")
def cases():
    """Built once and never changed: per case the stamps, the rows, a noisy light curve of its first row and the oracle's
    chi^2/2 and flux grid."""
    _lib.require_gpu()
    out = {}
    for ci, c in enumerate(_cases()):
        c["oracle_grid"] = O.flux_grid(O.MODEL_TP, c["t"], c["tp"], exptime=synth.EXPTIME, nsamples=S)[0]
        c["flux"] = synth.noisy_light_curve(np.random.default_rng(synth.SEED + 1700 + ci), c["oracle_grid"][0])
        c["oracle_h"] = O.lnl_batch(O.MODEL_TP, c["t"], c["flux"], synth.SIGMA, c["tp"], exptime=synth.EXPTIME, nsamples=S)
        c["t_d"], c["f_d"], c["tp_d"] = _lib.dev(c["t"]), _lib.dev(c["flux"]), _lib.dev(c["tp"])
        out[c["name"]] = c
    assert list(out) == CASE_NAMES
    return out


def _chunks(full):
    """True: full chunks in the likelihood kernels and the flux grid's (mode 2); False: the halo in both (mode 0); None:
    the defaults of both switches.  One sweep everywhere but at the defaults, so that only the chunking differs."""
    L = _lib.lib()
    assert L.trx_set_one_sweep(1 if full is None else 2) == 0
    assert L.trx_set_full_chunks(1 if full is None else (2 if full else 0)) == 0


def _three(c, flags):
    h = _lib.lnl_batch(_lib.MODEL_TP, flags, c["t_d"], c["f_d"], synth.SIGMA, c["tp_d"], synth.EXPTIME, S).cpu().numpy()
    f = _lib.flux_grid(_lib.MODEL_TP, flags, c["t_d"], c["tp_d"], synth.EXPTIME, S, False)[0].cpu().numpy()
    n = _lib.flux_grid(_lib.MODEL_TP, flags | _lib.FLAG_COUNT_EVALUATIONS, c["t_d"], c["tp_d"], synth.EXPTIME, S, False)[0].cpu().numpy()
    return h, f, n


def _both(c, flags=0):
    """(chi^2/2, flux grid, census) with the halo and with full chunks: trx_set_full_chunks 0 and 2, see _chunks"""
    try:
        got = {}
        for full in (False, True):
            _chunks(full)
            got[full] = _three(c, flags)
        return got
    finally:
        _chunks(None)


def _same_bits(a, b):
    return np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _stencil(count):
    return (count >= 1.0) & (count <= 2.0)


def _edges(pos):
    """full-chunk edges of a designed list: one per 64 entries of a window pass that has more behind them"""
    n = 0
    for p0 in range(0, pos.size, PASS):
        cnt = int((pos[p0:p0 + PASS] >= 0).sum())
        n += max(0, (cnt - 1) // 64)
    return n


def _check(c, got, costlier_ok=None):
    """what holds for every case: the oracle's bars in both modes, the modes against each other, the cost"""
    (h0, f0, n0), (h2, f2, n2) = got[False], got[True]
    want_h, want_f = c["oracle_h"], c["oracle_grid"]
    for full, (h, f, _) in got.items():
        rel = np.abs(h - want_h) / np.abs(want_h)
        err = np.abs(f - want_f).max()
        print("%s full chunks %d: chi2/2 vs oracle %.3g, flux vs oracle %.3g" % (c["name"], full, rel.max(), err))
        assert rel.max() < RTOL_ORACLE, (c["name"], full, rel)
        assert err < ATOL_FLUX, (c["name"], full, err)
    changed = _stencil(n0) != _stencil(n2)
    moved = np.abs(f2 - f0)
    rel_h = np.abs(h2 - h0) / np.abs(h0)
    print("%s: %d cells changed kind; the others moved by %.3g at most; chi2/2 by %.3g relative; evaluations %d -> %d"
          % (c["name"], changed.sum(), moved[~changed].max(), rel_h.max(), n0.sum(), n2.sum()))
    for r, pos in enumerate(c["pos"]):
        if pos is None:
            continue
        assert np.array_equal(n2[r] > 0, n0[r] > 0), (c["name"], c["names"][r], "the evaluated cells")
        assert changed[r].sum() <= 16 * _edges(pos), (c["name"], c["names"][r], changed[r].sum(), _edges(pos))
        at = np.flatnonzero(changed[r])
        lane = pos[at] % 64
        near56 = np.minimum(pos[at] % 56, 56 - pos[at] % 56) <= ST_M
        assert ((lane < ST_M) | (lane >= 64 - ST_M) | near56).all(), (c["name"], c["names"][r], pos[at])
    assert moved[~changed].max() <= MOVED_FLUX, (c["name"], moved[~changed].max(), np.argwhere(~changed & (moved > MOVED_FLUX))[:8])
    assert rel_h.max() <= MOVED_H, (c["name"], rel_h)
    dearer = n2 > n0
    for r, pos in enumerate(c["pos"]):
        if pos is None:
            dearer[r] = False          # (no designed list to name its chunks' first cells by)
    if costlier_ok is not None:
        dearer &= ~costlier_ok
    assert not dearer.any(), (c["name"], "cells that cost more with full chunks", np.argwhere(dearer)[:8], n0[dearer][:8], n2[dearer][:8])
    return changed


@pytest.mark.gpu
@pytest.mark.parametrize("r", (0, 1, 7, 8, 9, 56, 63))
def test_list_lengths_mod_64(cases, r):
    c = cases["wide-%d" % (384 + r)]
    n = c["n"]
    got = _both(c)
    _check(c, got)
    n0, n2 = got[False][2][0], got[True][2][0]
    # the list is the curve: every cell but the first and the last 8 takes the stencil, each at ONE evaluation ...
    assert (n2[ST_M:n - ST_M] == 1.0).all(), np.flatnonzero(n2[ST_M:n - ST_M] != 1.0) + ST_M
    assert (n2[:ST_M] >= 3.0).all() and (n2[n - ST_M:] >= 3.0).all()
    # ... where the halo spends two on every lent lane (list positions 56 m .. 56 m + 7 of a chunk that is not the last)
    lent = np.zeros(n, dtype=bool)
    for w0 in range(0, n, 56):
        if w0 + 64 < n:
            lent[w0 + 56:w0 + 64] = True
    assert np.array_equal(n0 == 2.0, lent), np.flatnonzero((n0 == 2.0) != lent)
    assert n0.sum() - n2.sum() == lent.sum()
    if r == 0:
        short = c["names"].index("short")
        assert (got[True][2][short] > 0).sum() == 60


def _main_masks(c, n2):
    """main case, full chunks: where a first cell of a chunk (lanes 0 .. 7) took its own nodes because a left neighbour
    had left no centre value -- the cells full chunks may pay more for than the halo"""
    ok = np.zeros(n2.shape, dtype=bool)
    for r, pos in enumerate(c["pos"]):
        if pos is not None:
            ok[r] = (pos >= 64) & (pos % 64 < ST_M) & (n2[r] >= 3.0) & (n2[r] < S)
    return ok


@pytest.mark.gpu
def test_stencil_cells_and_contact_runs_across_chunk_edges(cases):
    c = cases["main"]
    got = _both(c)
    n0, n2 = got[False][2], got[True][2]
    fallback = _main_masks(c, n2)
    _check(c, got, costlier_ok=fallback)
    wide = c["names"].index("wide")
    # >= 4 chunks of stencil cells: ONE evaluation at list positions 56 .. 71 (mod 64), two on the halo's lent lanes
    edge = np.zeros(c["n"], dtype=bool)
    for e in range(64, c["n"] - 64, 64):
        edge[e - ST_M:e + ST_M] = True
    assert (n2[wide][edge] == 1.0).all() and (n0[wide] == 2.0).sum() > 0 and (n2[wide] == 2.0).sum() == 0
    shifts = [r for r, name in enumerate(c["names"]) if name.startswith("shift-")]
    first_cells = runs_low = runs_high = 0
    for r in shifts:
        pos = c["pos"][r]
        lane = np.where(pos >= 0, pos % 64, -1)
        contact = n2[r] >= S
        # (a contact cell that delivers an owed centre value would show S + 1 in a chunk's first lanes; on a uniform grid
        # a stencil cell's radius keeps every contact cell out of its reach, so none does)
        assert ((n2[r] == S + 1) <= ((lane >= 0) & (lane < ST_M))).all()
        # the first st_ok cells in lanes 0 .. 7: own nodes with full chunks, the stencil with the halo
        first_cells += int((fallback[r] & _stencil(n0[r])).sum())
        runs_high += int((contact & (lane >= 64 - ST_M)).any())
        runs_low += int((contact & (lane >= 0) & (lane < ST_M)).any())
    print("main: %d first cells on their own nodes, contact cells in lanes 56..63 on %d rows, in lanes 0..7 on %d"
          % (first_cells, runs_high, runs_low))
    assert first_cells > 0 and runs_high > 0 and runs_low > 0
    # no contact cell is evaluated twice, in either mode
    assert n2.max() <= S + 1 and n0.max() <= S


@pytest.mark.gpu
def test_two_epochs_in_one_list(cases):
    c = cases["epochs"]
    got = _both(c)
    _check(c, got, costlier_ok=_main_masks(c, got[True][2]))
    for r, half in ((0, 96), (1, 100)):
        assert (got[True][2][r] > 0).sum() == 4 * half, (c["names"][r], (got[True][2][r] > 0).sum())
        assert c["pos"][r][int(150.5 + 1700 - half + 1)] == 2 * half         # the second window's first cell follows the first's last
        assert (got[True][2][r] == 1.0).sum() >= 2 * 64, (c["names"][r], "stencil cells in both windows")


@pytest.mark.gpu
def test_transit_on_the_window_pass_seam(cases):
    c = cases["seam"]
    got = _both(c)
    _check(c, got, costlier_ok=_main_masks(c, got[True][2]))
    n2 = got[True][2][c["names"].index("wide")]
    # the last 8 cells of a pass have no next chunk in it and the next pass's first 8 no left neighbours: own nodes
    assert (n2[PASS - ST_M:PASS + ST_M] >= 3.0).all() and (n2[PASS - 2 * ST_M:PASS - ST_M] == 1.0).all()
    assert (n2[PASS + ST_M:PASS + 2 * ST_M] == 1.0).all()


@pytest.mark.gpu
def test_weights_on_edge_cells_only(cases):
    c = cases["main"]
    pos = c["pos"][c["names"].index("wide")]
    w = np.where((pos % 64 < ST_M) | (pos % 64 >= 64 - ST_M), 1.0 / synth.SIGMA ** 2, 0.0)
    w_d = _lib.dev(w)
    want = 0.5 * ((c["flux"][None, :] - c["oracle_grid"]) ** 2 * w[None, :]).sum(axis=1)
    try:
        got = {}
        for full in (False, True):
            _chunks(full)
            got[full] = _lib.lnl_batch_weighted(_lib.MODEL_TP, 0, c["t_d"], c["f_d"], w_d, c["tp_d"], synth.EXPTIME, S).cpu().numpy()
    finally:
        _chunks(None)
    for full, h in got.items():
        rel = np.abs(h - want) / np.abs(want)
        print("weighted, full chunks %d: chi2/2 vs oracle %.3g" % (full, rel.max()))
        assert rel.max() < RTOL_ORACLE, (full, rel)
    rel_h = np.abs(got[True] - got[False]) / np.abs(got[False])
    print("weighted: chi2/2 moved by %.3g relative" % rel_h.max())
    assert rel_h.max() <= MOVED_H, rel_h


@pytest.mark.gpu
@pytest.mark.parametrize("flags", (_lib.FLAG_NO_STENCIL, _lib.FLAG_ALL_SUBEXPOSURES), ids=("no-stencil", "all-subexposures"))
def test_same_bits_where_the_changed_code_does_not_run(cases, flags):
    c = cases["main"]
    got = _both(c, flags)
    for what, a, b in zip(("chi2/2", "flux grid", "census"), got[False], got[True]):
        assert _same_bits(a, b), what
    h, f, _ = got[True]
    assert (np.abs(h - c["oracle_h"]) / np.abs(c["oracle_h"])).max() < RTOL_ORACLE
    assert np.abs(f - c["oracle_grid"]).max() < ATOL_FLUX


@pytest.mark.gpu
def test_the_default_is_full_chunks_in_the_likelihood_and_the_halo_in_the_flux_grid(cases):
    c = cases["main"]
    got = _both(c)
    _chunks(None)
    h, f, n = _three(c, 0)
    assert _same_bits(h, got[True][0])
    assert _lib.lib().trx_set_one_sweep(1) == 0 and _lib.lib().trx_set_full_chunks(0) == 0
    try:
        _, f0, n0 = _three(c, 0)
    finally:
        _chunks(None)
    assert _same_bits(f, f0) and _same_bits(n, n0)
    for bad in (-1, 3):
        assert _lib.lib().trx_set_full_chunks(bad) == 1          # TRX_ERR_ARG
    _chunks(None)


@pytest.mark.skipif(not os.path.exists(READELF), reason="llvm-readelf not installed")
def test_resources_of_the_full_chunk_instantiations():
    """BASELINE config 1's instantiation and its weighted twin: four waves per SIMD (<= 128 VGPRs), no scratch, and sixteen
    one-wave workgroups' LDS per CU (<= 10 240 B, from the function the launch plan uses).  No GPU needed."""
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libtrx.so not built")
    res = kernel_resources(_lib.LIB_PATH)
    found = {name: r for name, r in instantiations(res, "cells_kernel").items()
             if "cells_kernelILi0ELb1ELb0ELb1ELb1ELb0ELb0EE" in name or "cells_kernelILi0ELb1ELb0ELb1ELb1ELb0ELb1EE" in name}
    assert len(found) == 2, sorted(found)
    for name, (vgprs, _, scratch, static_lds) in found.items():
        assert vgprs <= 128 and scratch == 0 and static_lds == 0, (name, vgprs, scratch, static_lds)
    lds = _lib.lib().trx_debug_cells_lds_one_row()
    assert 0 < lds <= 10240, lds
