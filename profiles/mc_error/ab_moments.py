"""Cost of the Monte-Carlo moments: timing of the tree in the working directory -- run it from the
root of each tree, this one and the one before the change, alternately:  python <path>/profiles/mc_error/ab_moments.py TAG
(TAG ending in -nomoments: this tree with fused.MOMENTS = False).  The 64-TOI calc_probs_many step (N = 1e6, device
mode, 13 steps, the first 3 dropped) and the 75-scenario calc_probs of TOI-465.01 (N = 1e6, device mode, 30 calls, the
first 2 dropped); one JSON line with the medians and digests of the results (equal digests = the same bits)."""
import hashlib
import json
import os
import sys
import time

sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import numpy as np
import pandas as pd
import torch
import triceratops_amd
from triceratops_amd import synth
from triceratops_amd.triceratops import target

GOLD = os.path.join(os.getcwd(), "tests", "golden")
tag = sys.argv[1]
if tag.endswith("-nomoments"):
    from triceratops_amd import fused
    fused.MOMENTS = False
triceratops_amd.set_sampling("device")
jobs = synth.toi_jobs(64, n_time=200, N=1_000_000, seed=synth.SEED + 4,
                      trilegal_fname=os.path.join(GOLD, "trilegal_synth.csv"),
                      contrast_curve_file=os.path.join(GOLD, "contrast_curve_synth.csv"))
steps = []
for s in range(13):
    torch.manual_seed(100 + s)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = triceratops_amd.calc_probs_many(jobs)
    for tg in out:
        tg.FPP
    torch.cuda.synchronize()
    steps.append(time.perf_counter() - t0)
batch_lnz = np.concatenate([tg.lnZ for tg in out])
batch_fpp = np.array([tg.FPP for tg in out])
g = np.load(os.path.join(GOLD, "toi465_calc_probs.npz"))
cols = ("ID", "Tmag", "Jmag", "Hmag", "Kmag", "ra", "dec", "mass", "rad", "Teff", "plx", "fluxratio", "tdepth")
st = pd.DataFrame({c: g["blend_stars_%s" % c] for c in cols})
st["ID"] = st["ID"].astype(np.int64)
tg = target(270380593, np.array([4]), stars=st.copy(), trilegal_fname=os.path.join(GOLD, "trilegal_synth.csv"))
e2e = []
for rep in range(30):
    np.random.seed(465)
    torch.manual_seed(465)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    tg.calc_probs(g["time"], g["flux"], float(g["sigma"][0]), float(g["P_orb"][0]),
                  contrast_curve_file=os.path.join(GOLD, "toi465_cc.csv"), N=1_000_000, parallel=True, verbose=0)
    torch.cuda.synchronize()
    e2e.append(time.perf_counter() - t0)


def digest(a):
    return hashlib.sha1(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


print(json.dumps({"tag": tag, "batch_step_median_s": float(np.median(steps[3:])), "batch_steps": steps[3:],
                  "calc75_median_s": float(np.median(e2e[2:])), "calc75": e2e[2:], "n_scen75": len(tg.lnZ),
                  "batch_lnz_digest": digest(batch_lnz), "batch_fpp_digest": digest(batch_fpp),
                  "calc75_lnz_digest": digest(tg.lnZ), "calc75_FPP": float(tg.FPP)}))
