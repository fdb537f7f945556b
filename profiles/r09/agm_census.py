"""AGM trips of cel_pair per lane against trips per wave on config 1 (2000 uniform points, 10^5 rows, the 18 families),
from a library built with -DTRX_CENSUS:  TRX_LIB=<census build> python profiles/r09/agm_census.py
A wave stays in the AGM loop until its last lane has converged; a lane that is done sits the other trips out."""
import ctypes
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
import torch  # noqa: E402
from triceratops_amd import _lib, synth  # noqa: E402

n_time, n_rows = 2000, 100_000
L = _lib.lib()
L.trx_debug_census.restype = ctypes.c_int
L.trx_debug_census.argtypes = [ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int]
rng = np.random.default_rng(synth.SEED)
t_d = _lib.dev(synth.time_grid(n_time))
curve, _ = _lib.flux_grid(_lib.MODEL_TP, 0, t_d, _lib.dev(synth.reference_tp_row()), synth.EXPTIME, synth.NSAMPLES, False)
f_d = _lib.dev(synth.noisy_light_curve(rng, curve[0].cpu().numpy()))
rows = [_lib.dev(synth.family_rows(rng, fam, n_rows)) for fam in synth.FAMILIES]
out = torch.empty(n_rows, dtype=torch.float64, device="cuda")


def step():
    for (name, model, is_host, has_comp), r in zip(synth.FAMILIES, rows):
        flags = (_lib.FLAG_COMPANION_IS_HOST if is_host else 0) | _lib.FLAG_EVALUATE_EXCLUDED
        _lib.lnl_batch(model, flags, t_d, f_d, synth.SIGMA, r, synth.EXPTIME, synth.NSAMPLES, out=out)


step()
buf = (ctypes.c_ulonglong * 32)()
_lib.check(L.trx_debug_census(buf, 1))
step()
_lib.check(L.trx_debug_census(buf, 1))
agm_trip, agm_lanes, cel_call, cel_lanes = (buf[i] / len(synth.FAMILIES) for i in (8, 15, 16, 17))
print("per launch: cel_pair entered by %.4g waves with %.4g lanes (%.1f lanes a wave); AGM trips (two steps each) %.4g by "
      "waves, %.4g by lanes" % (cel_call, cel_lanes, cel_lanes / cel_call, agm_trip, agm_lanes))
print("AGM trips per wave %.3f, per lane %.3f: a lane is active in %.1f %% of the lane slots of its wave's trips"
      % (agm_trip / cel_call, agm_lanes / cel_lanes, 100.0 * agm_lanes / (agm_trip * cel_lanes / cel_call)))
