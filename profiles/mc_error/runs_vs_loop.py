"""target.calc_probs_runs(n_runs=20) against the tutorial's loop of 20 calc_probs calls: TOI-465.01
with its contrast curve and the notebook's star table, N = 1e6, device mode, after a warm-up; two rounds of both, the
same seed, one JSON line (same_fpp: the runs equal the loop's calls bit for bit).  Run from the root of the tree."""
import json
import os
import sys
import time

sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import numpy as np
import torch
import anchors
import triceratops_amd
from triceratops_amd.triceratops import target

triceratops_amd.set_sampling("device")
c = anchors.CASES["toi465_cc"]
stars, t, f, sigma, P = anchors.inputs("toi465_cc")
tg = target(c["ID"], np.array([1]), mission=c["mission"], stars=stars, trilegal_fname=anchors.TRILEGAL)
kw = dict(contrast_curve_file=c["cc"], N=1_000_000, parallel=True)
tg.calc_probs(t, f, sigma, P, verbose=0, **kw)            # warm-up: tables, allocator
tg.calc_probs_runs(t, f, sigma, P, n_runs=2, **kw)
res = {}
for rep in range(2):
    torch.manual_seed(7)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fpp = []
    for _ in range(20):
        tg.calc_probs(t, f, sigma, P, verbose=0, **kw)
        fpp.append(tg.FPP)
    torch.cuda.synchronize()
    res.setdefault("loop_s", []).append(time.perf_counter() - t0)
    torch.manual_seed(7)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    runs = tg.calc_probs_runs(t, f, sigma, P, n_runs=20, **kw)
    torch.cuda.synchronize()
    res.setdefault("runs_s", []).append(time.perf_counter() - t0)
    res["same_fpp"] = bool(np.array_equal(np.array(fpp), runs["FPP"]))
res.update(FPP_mean=runs["FPP_mean"], FPP_std=runs["FPP_std"], FPP_err_median=float(np.median(runs["FPP_err"])),
           n_scen=int(runs["lnZ"].shape[1]))
print(json.dumps(res))
