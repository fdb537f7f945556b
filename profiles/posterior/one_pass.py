"""one calc_posteriors(n_samples=1000) of the 75-scenario TOI-465.01 blend after a warm-up pass, for a kernel trace"""
import os
import sys

import numpy as np
import pandas as pd
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import triceratops_amd  # noqa: E402
from triceratops_amd.triceratops import target  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")
G = np.load(os.path.join(GOLD, "toi465_calc_probs.npz"), allow_pickle=True)
COLS = ("ID", "Tmag", "Jmag", "Hmag", "Kmag", "ra", "dec", "mass", "rad", "Teff", "plx", "fluxratio", "tdepth")
st = pd.DataFrame({c: G["blend_stars_%s" % c] for c in COLS})
st["ID"] = st["ID"].astype(np.int64)
tg = target(270380593, np.array([4]), stars=st, trilegal_fname=os.path.join(GOLD, "trilegal_synth.csv"))
triceratops_amd.set_sampling("device")
for seed in (1, 2):
    torch.manual_seed(seed)
    tg.calc_posteriors(G["time"], G["flux"], float(G["sigma"][0]), float(G["P_orb"][0]), n_samples=1000,
                       contrast_curve_file=os.path.join(GOLD, "toi465_cc.csv"), N=1000000, parallel=True, verbose=0)
torch.cuda.synchronize()
print("done", tg.FPP)
