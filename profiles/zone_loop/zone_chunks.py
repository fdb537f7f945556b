"""Chunks per row that the zone loop takes on BASELINE config 1's grid (2000 uniform points, 512 rows of each of the 18
families, as bench.py's census takes them): the testing library's trx_debug_zone_chunks around the likelihood launches,
with the loop on and, as a check of the counter, off.  (First-sweep chunks per row: 14.099, profiles/full_chunks/results.txt.)
    python profiles/zone_loop/zone_chunks.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from oracle import oracle as O  # noqa: E402
from triceratops_amd import _lib, synth  # noqa: E402

_lib.use_testing_library(True)
L = _lib.lib()
rng = np.random.default_rng(synth.SEED)
t = synth.time_grid(2000)
flux = synth.noisy_light_curve(rng, O.flux_grid(O.MODEL_TP, t, synth.reference_tp_row())[0][0])
t_d, f_d = _lib.dev(t), _lib.dev(flux)
rows = [_lib.dev(synth.family_rows(rng, fam, 512)) for fam in synth.FAMILIES]
for on in (1, 0):
    assert L.trx_set_zone_loop(on) == 0
    _lib.debug_zone_chunks(reset=True)
    per_family = []
    for (name, model, is_host, has_comp), r in zip(synth.FAMILIES, rows):
        flags = _lib.FLAG_COMPANION_IS_HOST if is_host else 0
        _lib.lnl_batch(model, flags, t_d, f_d, synth.SIGMA, r, synth.EXPTIME, synth.NSAMPLES)
        per_family.append(_lib.debug_zone_chunks(reset=True) / 512.0)
    print("trx_set_zone_loop(%d): %.3f zone chunks per row (18 families x 512 rows x 2000 points); per family %s"
          % (on, float(np.mean(per_family)), " ".join("%.2f" % v for v in per_family)))
assert L.trx_set_zone_loop(1) == 0
