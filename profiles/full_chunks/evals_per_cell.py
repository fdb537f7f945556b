"""Model evaluations per cell on BASELINE config 1's grid (2000 uniform points, 512 rows of each of the 18 families, as
bench.py's census takes them) with the stencil's one-sided halo and with full chunks: the evaluation census
of trx_flux_grid (TRX_FLAG_COUNT_EVALUATIONS) on the TESTING library, trx_set_one_sweep(2) and trx_set_full_chunks 0 / 2.
bench.py's own roofline.model_evaluations_per_cell prices the production flux grid, which keeps the halo, and does not move.
    python profiles/full_chunks/evals_per_cell.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from triceratops_amd import _lib, synth  # noqa: E402

_lib.use_testing_library(True)
L = _lib.lib()
rng = np.random.default_rng(synth.SEED)
t_d = _lib.dev(synth.time_grid(2000))
rows = [_lib.dev(synth.family_rows(rng, fam, 512)) for fam in synth.FAMILIES]
assert L.trx_set_one_sweep(2) == 0
for mode in (0, 2):
    assert L.trx_set_full_chunks(mode) == 0
    total = cells = 0.0
    for (name, model, is_host, has_comp), r in zip(synth.FAMILIES, rows):
        flags = (_lib.FLAG_COMPANION_IS_HOST if is_host else 0) | _lib.FLAG_COUNT_EVALUATIONS
        c, _ = _lib.flux_grid(model, flags, t_d, r, synth.EXPTIME, synth.NSAMPLES, False)
        total += float(c.sum())
        cells += float(c.numel())
    print("trx_set_full_chunks(%d): %.6f model evaluations per cell (%d families x 512 rows x 2000 points)"
          % (mode, total / cells, len(rows)))
assert L.trx_set_one_sweep(1) == 0 and L.trx_set_full_chunks(1) == 0
