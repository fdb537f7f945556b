#!/usr/bin/env python3
"""Fixture of tests/test_gpu_window_trips.py: uniform time grids on which cells_kernel's stencil instantiation walks only
the window trips that can hold an in-window cell (trx_cells.hpp, window_trips), with what the library computed on them
BEFORE that change -- every trip walked, every out-of-window cell's chi^2 term summed by the row's own lanes.

Needs an MI355X and a build of the parent of the commit that introduced window_trips:

    TRX_LIB=/path/to/parent/libtrx.so python tests/golden/make_window_trips.py [OUT.npz]

Per case (a grid length, a spacing in exposures, an offset of the grid against conjunction at t = 0) the file holds the
inputs -- stamps, a noisy light curve, a block of TP rows and one of EB rows -- and the parent's chi^2/2 of every row, its
flux grid of a few rows and its per-cell evaluation census of the same rows.  Only DATA leaves this script.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(HERE, "window_trips.npz")

RSUN, REARTH = 69570000000.0, 637810000.0
# (grid length, spacing / exposure, offset of the grid's centre in days).  0.18 is BASELINE config 1's spacing; the stencil
# takes spacings between 0.112 and 0.3 exposures; 2049 = one window pass of 2048 cells and one cell more.
CASES = [(478, 0.18, 0.0), (478, 0.29, 0.021), (478, 0.12, -0.013),
         (2000, 0.18, 0.0), (2000, 0.12, 0.07), (2000, 0.29, -0.19), (2000, 0.18, 0.37),
         (2049, 0.18, 0.0), (2049, 0.29, 0.11), (2049, 0.12, -0.02)]
GRID_ROWS = 5             # rows per block whose flux grid and census are stored: the first two and the last three


def tp_block(rng, n):
    """TP rows [10][n] (R_p P inc a R_s u1 u2 ecc argp comp_fr) with periods from a twentieth of a day -- many epochs on
    every grid above -- to 40 d -- one or none --, orbits from 1.3 stellar radii (windows that wrap round the orbit) to 40,
    eccentricities up to 0.92 (two near-side passages); then a flat row, a second one, and a row whose dilution is NaN"""
    R_s = rng.uniform(0.3, 2.0, n)
    k = rng.uniform(0.02, 0.4, n)
    per = 10 ** rng.uniform(np.log10(0.05), np.log10(40.0), n)
    a_R = 10 ** rng.uniform(np.log10(1.3), np.log10(40.0), n)
    ecc = np.where(rng.random(n) < 0.5, 0.0, rng.uniform(0.0, 0.92, n))
    argp = rng.uniform(0.0, 360.0, n)
    inc = rng.uniform(78.0, 90.0, n)
    rows = np.stack([k * R_s * RSUN / REARTH, per, inc, a_R * R_s * RSUN, R_s, rng.uniform(0.1, 0.6, n),
                     rng.uniform(0.05, 0.4, n), ecc, argp, np.where(rng.random(n) < 0.5, 0.0, rng.uniform(0.01, 0.5, n))])
    rows = rows[:, a_R * (1.0 - ecc) > 1.0 + k]
    special = rows[:, :3].copy()
    special[1] = (3.0, 17.0, 3.0)                 # periods
    special[2] = (60.0, 55.0, 89.0)               # inclinations: the first two pass the star by
    special[3] = 12.0 * special[4] * RSUN
    special[7] = 0.0
    special[9] = (0.0, 0.2, 1.0)                  # companion flux ratio 1: an infinite dilution, NaN
    return np.ascontiguousarray(np.concatenate([rows, special], axis=1))


def eb_block(rng, n):
    """EB rows of the bench's generator (both sides of the secondary-eclipse rule) and the e = 0.9 row with a second
    near-side passage of tests/test_gpu_kernels.py"""
    from triceratops_amd import synth
    rows = synth.eb_rows(rng, n, has_companion=True)
    hull = np.array([[9.62080439e-01], [2.93357695e-05], [1.23513199e+01], [6.48158862e+01], [1.59025933e+12],
                     [1.38005527e+00], [1.52880035e-01], [5.74606889e-02], [9.00000000e-01], [1.05234974e+02],
                     [2.09587868e-01]])
    return np.ascontiguousarray(np.concatenate([rows, hull], axis=1))


def main():
    from oracle import oracle as O
    from triceratops_amd import _lib, synth
    _lib.require_gpu()
    out = {"n_cases": np.array(len(CASES)), "exptime": np.array(synth.EXPTIME), "nsamples": np.array(synth.NSAMPLES), "sigma": np.array(synth.SIGMA)}
    for ci, (n_time, ratio, offset) in enumerate(CASES):
        rng = np.random.default_rng(synth.SEED + 500 + ci)
        half = 0.5 * (n_time - 1) * ratio * synth.EXPTIME
        t = np.linspace(offset - half, offset + half, n_time)
        ref = synth.reference_tp_row()
        ref[1] = 0.31                     # (a transit on every grid, whatever its offset)
        flux = synth.noisy_light_curve(rng, O.flux_grid(O.MODEL_TP, t, ref)[0][0])
        tp, eb = tp_block(rng, 160), eb_block(rng, 64)
        t_d, f_d = _lib.dev(t), _lib.dev(flux)
        p = "c%d_" % ci
        out.update({p + "t": t, p + "flux": flux, p + "tp": tp, p + "eb": eb})
        for key, model, rows in (("tp", _lib.MODEL_TP, tp), ("eb", _lib.MODEL_EB, eb)):
            r_d = _lib.dev(rows)
            out[p + "h_" + key] = _lib.lnl_batch(model, 0, t_d, f_d, synth.SIGMA, r_d, synth.EXPTIME, synth.NSAMPLES).cpu().numpy()
            pick = np.unique(np.concatenate([np.arange(GRID_ROWS - 3), np.arange(rows.shape[1] - 3, rows.shape[1])]))
            sub = _lib.dev(np.ascontiguousarray(rows[:, pick]))
            out[p + "pick_" + key] = pick
            out[p + "grid_" + key] = _lib.flux_grid(model, 0, t_d, sub, synth.EXPTIME, synth.NSAMPLES, False)[0].cpu().numpy()
            c = _lib.flux_grid(model, _lib.FLAG_COUNT_EVALUATIONS, t_d, sub, synth.EXPTIME, synth.NSAMPLES, False)[0].cpu().numpy()
            assert np.array_equal(c, np.round(c)) and c.min() >= 0 and c.max() < 256
            out[p + "count_" + key] = c.astype(np.uint8)
    dst = sys.argv[1] if len(sys.argv) > 1 else OUT
    np.savez_compressed(dst, **out)
    print("wrote", dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
