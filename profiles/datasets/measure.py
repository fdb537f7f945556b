"""Measurements of DESIGN.md section 14 (several light curves, per-point errors).

  python profiles/datasets/measure.py            the whole job: each GPU step a child process under its own time
                                                 limit, the next one only after the last ended well; writes
                                                 profiles/datasets/results.txt (or --out FILE)
  python profiles/datasets/measure.py kernels    (a) chi2_grid_weighted_kernel and chi2_grid_kernel on the same 3.2 GB
                                                 grid (200 000 rows x 2000 stamps, bench.py's size), timed with events
  python profiles/datasets/measure.py e2e        (b) TOI-465.01, 75 scenarios, N = 1e6: calc_probs against
                                                 calc_probs_datasets with one and with two datasets

The job runs `kernels` twice: plainly, and under `rocprofv3 --kernel-trace --stats`, whose kernel trace gives the
per-launch times quoted (the event timings include the launch gaps of five back-to-back calls).
"""
import csv
import glob
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
N_GRID, N_TIME = 200_000, 2000
GB = (N_GRID * N_TIME * 8 + N_GRID * 8) / 1e9


def kernels():
    import numpy as np
    import torch
    from triceratops_amd import _lib, synth
    rng = np.random.default_rng(synth.SEED)
    f_d = _lib.dev(1.0 + rng.normal(0.0, synth.SIGMA, N_TIME))
    w_d = _lib.dev(1.0 / (rng.uniform(0.5, 2.0, N_TIME) * synth.SIGMA) ** 2)
    grid = torch.rand((N_GRID, N_TIME), dtype=torch.float64, device="cuda")
    out = torch.zeros(N_GRID, dtype=torch.float64, device="cuda")

    def timed(fn, reps=5):
        fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e-3 / reps

    for name, fn in (("chi2_grid_kernel", lambda: _lib.chi2_grid(f_d, grid, synth.SIGMA)),
                     ("chi2_grid_weighted_kernel", lambda: _lib.chi2_grid_weighted(f_d, w_d, grid)),
                     ("chi2_grid_weighted_kernel (accumulate)", lambda: _lib.chi2_grid_weighted(f_d, w_d, grid, out=out))):
        dt = timed(fn)
        print("events  %-40s %.3f ms  %.2f TB/s  (%.2f GB)" % (name, dt * 1e3, GB / dt / 1e3, GB), flush=True)
    # the shape of the end-to-end path: 1e6 rows of 100 stamps
    small = torch.rand((1_000_000, 100), dtype=torch.float64, device="cuda")
    dt = timed(lambda: _lib.chi2_grid_weighted(f_d[:100].contiguous(), w_d[:100].contiguous(), small))
    print("events  %-40s %.3f ms  %.2f TB/s  (0.81 GB: 1e6 rows x 100 stamps)" % ("chi2_grid_weighted_kernel", dt * 1e3, 0.808 / dt / 1e3), flush=True)


def e2e():
    import numpy as np
    import pandas as pd
    import torch
    from helpers import GOLD, gold
    import triceratops_amd as ta
    from triceratops_amd.triceratops import target
    G = gold("toi465_calc_probs.npz")
    cols = ("ID", "Tmag", "Jmag", "Hmag", "Kmag", "ra", "dec", "mass", "rad", "Teff", "plx", "fluxratio", "tdepth")
    st = pd.DataFrame({c: G["blend_stars_%s" % c] for c in cols})
    st["ID"] = st["ID"].astype(np.int64)
    tg = target(270380593, np.array([4]), stars=st, trilegal_fname=os.path.join(GOLD, "trilegal_synth.csv"))
    ta.set_sampling("device")
    t, f, s, P = G["time"], G["flux"], float(G["sigma"][0]), float(G["P_orb"][0])
    kw = dict(contrast_curve_file=os.path.join(GOLD, "toi465_cc.csv"), N=1_000_000, parallel=True, verbose=0)
    one = [{"time": t, "flux": f, "flux_err": s}]
    two = [{"time": t[k::2], "flux": f[k::2], "flux_err": s} for k in (0, 1)]
    runs = (("calc_probs", lambda: tg.calc_probs(t, f, s, P, **kw)),
            ("calc_probs_datasets, 1 dataset of 100 points", lambda: tg.calc_probs_datasets(one, P, **kw)),
            ("calc_probs_datasets, 2 datasets of 50 points", lambda: tg.calc_probs_datasets(two, P, **kw)))
    for name, fn in runs:
        best = None
        for rep in range(3):                 # (the first run of each warms caches and scratch)
            torch.manual_seed(1)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            best = dt if rep and (best is None or dt < best) else best
        print("e2e     %-48s %.3f s  (%d scenarios, FPP %.4g)" % (name, best, tg.lnZ.size, tg.FPP), flush=True)


def trace_summary(trace):
    """per-launch kernel times of the `kernels` step from rocprofv3's kernel trace, by launch shape, each shape's first
    (warm-up) launch left out -- the --stats averages would mix the shapes"""
    lines = []
    for f in glob.glob(os.path.join(trace, "**", "*kernel_trace.csv"), recursive=True):
        groups = {}
        for row in csv.DictReader(open(f)):
            if "chi2_grid" in row["Kernel_Name"]:
                name = "chi2_grid_weighted_kernel" if "weighted" in row["Kernel_Name"] else "chi2_grid_kernel"
                groups.setdefault((name, row["Grid_Size_X"]), []).append(int(row["End_Timestamp"]) - int(row["Start_Timestamp"]))
        for (name, grid), ns in groups.items():
            big = len(ns) != 6 or name == "chi2_grid_kernel"      # (12 launches: six that write, then six that accumulate)
            parts = ((name, ns),) if len(ns) == 6 else ((name, ns[:6]), (name + " (accumulate)", ns[6:]))
            for label, part in parts:
                avg = sum(part[1:]) / max(len(part) - 1, 1)
                gb = GB if big else 0.808
                lines.append("rocprofv3 %-40s %d launches  %.1f us  %.2f TB/s  (%.2f GB)\n"
                             % (label, len(part) - 1, avg * 1e-3, gb / (avg * 1e-9) / 1e3, gb))
    return "".join(lines)


def _step(out, limit, cmd):
    """one child under its own time limit; its output goes to `out`; False ends the job"""
    print("+ " + " ".join(cmd), flush=True)
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, cwd=ROOT, capture_output=True, text=True)
    out.write(r.stdout)
    if r.returncode != 0:
        out.write("step failed with status %d: %s\n%s\n" % (r.returncode, " ".join(cmd), r.stderr[-2000:]))
    out.flush()
    return r.returncode == 0


def job(path):
    me, trace = os.path.abspath(__file__), os.path.join(os.path.dirname(path) or ".", "rocprof_datasets")
    with open(path, "w") as out:
        out.write("# profiles/datasets/measure.py on one MI355X; %.2f GB per chi2 launch\n" % GB)
        ok = _step(out, 240, [sys.executable, me, "kernels"])
        ok = ok and _step(out, 300, ["rocprofv3", "--kernel-trace", "--stats", "-d", trace, "-o", "chi2", "--output-format",
                                     "csv", "--", sys.executable, me, "kernels"])
        if ok:
            out.write(trace_summary(trace))
        ok = ok and _step(out, 420, [sys.executable, me, "e2e"])
        out.write("job %s\n" % ("complete" if ok else "ended early"))
    return 0 if ok else 1


if __name__ == "__main__":
    if sys.argv[1:2] == ["kernels"]:
        kernels()
    elif sys.argv[1:2] == ["e2e"]:
        e2e()
    else:
        dest = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(os.path.dirname(os.path.abspath(__file__)), "results.txt")
        sys.exit(job(dest))
