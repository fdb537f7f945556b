"""calc_probs against calc_posteriors(n_samples=1000) on TOI-465.01 (15 and 75 scenarios, N = 1e6, device sampling):
wall-clock per pass, median and spread of REPS passes after a warm-up.  Prints the lines of results.txt.  Where the
tree has calc_posteriors_many: the same pair for a batch of 16 synthetic TOIs (synth.toi_jobs, N = 2e5)."""
import os
import sys
import time

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
REPS = int(os.environ.get("REPS", "7"))


def make(tag):
    st = pd.DataFrame({c: G["%s_stars_%s" % (tag, c)] for c in COLS})
    st["ID"] = st["ID"].astype(np.int64)
    return target(270380593, np.array([4]), stars=st, trilegal_fname=os.path.join(GOLD, "trilegal_synth.csv"))


def timed(fn):
    out = []
    for r in range(REPS + 1):
        torch.manual_seed(465 + r)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    out = np.array(out[1:]) * 1e3
    return np.median(out), out.min(), out.max()


triceratops_amd.set_sampling("device")
args = (G["time"], G["flux"], float(G["sigma"][0]), float(G["P_orb"][0]))
kw = dict(contrast_curve_file=os.path.join(GOLD, "toi465_cc.csv"), N=1000000, parallel=True, verbose=0)
for tag in ("real", "blend"):
    tg = make(tag)
    for label, fn in (("calc_probs", lambda: tg.calc_probs(*args, **kw)),
                      ("calc_posteriors(1000)", lambda: tg.calc_posteriors(*args, n_samples=1000, **kw)),
                      ("calc_probs (again)", lambda: tg.calc_probs(*args, **kw))):
        med, lo, hi = timed(fn)
        print("%-5s %2d scenarios  %-22s median %7.2f ms  (min %7.2f, max %7.2f, %d passes)"
              % (tag, len(tg.lnZ), label, med, lo, hi, REPS), flush=True)

if hasattr(triceratops_amd, "calc_posteriors_many"):
    from triceratops_amd import synth  # noqa: E402
    jobs = synth.toi_jobs(16, n_time=200, N=200000, seed=synth.SEED, trilegal_fname=os.path.join(GOLD, "trilegal_synth.csv"),
                          contrast_curve_file=os.path.join(GOLD, "contrast_curve_synth.csv"))
    for label, fn in (("calc_probs_many", lambda: triceratops_amd.calc_probs_many(jobs)),
                      ("calc_posteriors_many(1000)", lambda: triceratops_amd.calc_posteriors_many(jobs, n_samples=1000)),
                      ("... keep='summary'", lambda: triceratops_amd.calc_posteriors_many(jobs, n_samples=1000, keep="summary"))):
        med, lo, hi = timed(fn)
        print("batch %d TOIs x %d rows  %-26s median %7.2f ms  (min %7.2f, max %7.2f, %d passes)"
              % (len(jobs), len(jobs[0][0].lnZ), label, med, lo, hi, REPS), flush=True)
