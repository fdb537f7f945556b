"""One pass of the 18 families through the likelihood path on BASELINE config 1's grid (2000 uniform points, 10^5 rows,
every row evaluated: TRX_FLAG_EVALUATE_EXCLUDED), production library, for a counters-only rocprofv3 run:
TRX_LIB=<build> rocprofv3 --pmc ... -- python profiles/r07/cells2000_once.py"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np, torch
from triceratops_amd import _lib, synth
n_time, n_rows = 2000, 100000
rng = np.random.default_rng(synth.SEED)
t_d = _lib.dev(synth.time_grid(n_time))
curve, _ = _lib.flux_grid(0, 0, t_d, _lib.dev(synth.reference_tp_row()), synth.EXPTIME, synth.NSAMPLES, False)
f_d = _lib.dev(synth.noisy_light_curve(rng, curve[0].cpu().numpy()))
out = torch.empty(n_rows, dtype=torch.float64, device="cuda")
for fam in synth.FAMILIES:
    r_d = _lib.dev(synth.family_rows(rng, fam, n_rows))
    flags = (_lib.FLAG_COMPANION_IS_HOST if fam[2] else 0) | _lib.FLAG_EVALUATE_EXCLUDED
    _lib.lnl_batch(fam[1], flags, t_d, f_d, synth.SIGMA, r_d, synth.EXPTIME, synth.NSAMPLES, out=out)
torch.cuda.synchronize()
