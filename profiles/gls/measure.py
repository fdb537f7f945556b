"""Measurements of DESIGN.md section 14, baseline terms marginalised under red noise (`red_baseline` next to `red_sigma` /
`red_timescale`, scan_rows_kernel<ONE, OuColsFilter<K>>).

  python profiles/gls/measure.py            the whole job: each GPU step a child process under its own time limit, the next
                                            one only after the last ended well; writes profiles/gls/results.txt (or --out FILE)
  python profiles/gls/measure.py kernels    (a) the OuColsFilter<K> kernel (_lib.chi2_grid_ou_baseline) at K = 1, 2, 4 columns on a
                                            512 MiB grid at n_time = 100 and 2048 against the OuFilter kernel (_lib.chi2_grid_ou) on
                                            the same grid and tables: the same bytes, K more fmas a value and K more butterflies
                                            a row.  Nothing else in the library computes the column sums, so there is no operator
                                            alternative to hold against.  One warm-up of each, then five rounds in which the four
                                            take turns, each run timed with device events; the best of the five
  python profiles/gls/measure.py e2e        (b) TOI-465.01, N = 1e6, two datasets of 50 points: calc_probs_datasets with
                                            red_sigma / red_timescale on the second dataset, and with two columns (1, u) next to
                                            them; wall clock of whole calls, taking turns
"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
GRID_BYTES = 512 << 20
ROUNDS = 5
KS = (1, 2, 4)


def kernels():
    import numpy as np
    import torch
    from triceratops_amd import _lib
    from triceratops_amd import datasets as D

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e-3

    for n_time in (100, 2048):
        n = GRID_BYTES // (8 * n_time)
        rng = np.random.default_rng(n_time)
        t = np.cumsum(rng.uniform(0.3, 1.7, n_time))
        err = 1e-3 * rng.uniform(0.6, 1.8, n_time)
        d = D.validate([{"time": t, "flux": np.ones(n_time), "flux_err": err, "red_sigma": 3e-3, "red_timescale": 10.0}])[0]
        u = (t - 0.5 * (t[0] + t[-1])) / (0.5 * (t[-1] - t[0]))
        systems = {K: D.ou_baseline_system(d, np.stack([u ** p for p in range(K)]), np.inf) for K in KS}
        abw = tuple(_lib.dev(v) for v in D.ou_system(d))
        cols = {K: _lib.dev(s.c) for K, s in systems.items()}
        torch.manual_seed(n_time)
        flux = _lib.dev(1.0 + err * rng.normal(0.0, 1.0, n_time))
        grid = 1.0 + 3e-4 * torch.randn((n, n_time), dtype=torch.float64, device="cuda")
        out = torch.zeros(n, dtype=torch.float64, device="cuda")

        def plain():
            return _lib.chi2_grid_ou(flux, grid, *abw, out=out)

        def gls(K):
            return lambda: _lib.chi2_grid_ou_baseline(flux, grid, *abw, cols[K], systems[K].minv, out=out)

        runs = [("ou", plain)] + [("K=%d" % K, gls(K)) for K in KS]
        # (M = 0 gives the OU kernel's bits: the two read the same grid the same way)
        same = torch.equal(_lib.chi2_grid_ou_baseline(flux, grid, *abw, cols[4], np.zeros(10)), _lib.chi2_grid_ou(flux, grid, *abw))
        for _, fn in runs:
            fn()
        torch.cuda.synchronize()
        times = {name: [] for name, _ in runs}
        for _ in range(ROUNDS):
            for name, fn in runs:
                times[name].append(timed(fn))
        best = {name: min(v) for name, v in times.items()}
        moved = n * n_time * 8
        print("events  %d rows x %d stamps (%.0f MiB)  chi2_ou_kernel %.4f ms (%.2f TB/s)   %s   (best of %d, taking turns; %s; "
              "M = 0 gives chi2_ou_kernel's bits: %s)"
              % (n, n_time, moved / 2 ** 20, best["ou"] * 1e3, moved / best["ou"] / 1e12,
                 "   ".join("gls_ou_kernel %s %.4f ms (%.2f TB/s, %.2f x)" % (name, best[name] * 1e3, moved / best[name] / 1e12,
                                                                            best[name] / best["ou"]) for name, _ in runs[1:]),
                 ROUNDS, "; ".join("%s %s ms" % (name, " ".join("%.4f" % (v * 1e3) for v in times[name])) for name, _ in runs),
                 same), flush=True)
        del grid


def e2e():
    """wall clock of whole calls, each ended by a device synchronise: one warm-up of every case, then ROUNDS rounds in which
    they take turns"""
    import numpy as np
    import pandas as pd
    import torch
    from helpers import GOLD, gold
    import triceratops_amd as ta
    from triceratops_amd.lightcurve import trend_columns
    from triceratops_amd.triceratops import target
    G = gold("toi465_calc_probs.npz")
    cols = ("ID", "Tmag", "Jmag", "Hmag", "Kmag", "ra", "dec", "mass", "rad", "Teff", "plx", "fluxratio", "tdepth")
    st = pd.DataFrame({c: G["blend_stars_%s" % c] for c in cols})
    st["ID"] = st["ID"].astype(np.int64)
    tg = target(270380593, np.array([4]), stars=st, trilegal_fname=os.path.join(GOLD, "trilegal_synth.csv"))
    ta.set_sampling("device")
    t, f, s, P = G["time"], G["flux"], float(G["sigma"][0]), float(G["P_orb"][0])
    kw = dict(contrast_curve_file=os.path.join(GOLD, "toi465_cc.csv"), N=1_000_000, parallel=True, verbose=0)
    two = [{"time": t[k::2], "flux": f[k::2], "flux_err": s} for k in (0, 1)]
    cadence = float(np.median(np.diff(two[1]["time"])))
    red = [two[0], dict(two[1], red_sigma=2.0 * s, red_timescale=20.0 * cadence)]
    keyed = [two[0], dict(red[1], red_baseline=trend_columns(two[1]["time"], 1))]
    names = ("2 datasets of 50 points, red_sigma on the second", "the same + red_baseline (1, u)")
    runs = [(names[0], lambda: tg.calc_probs_datasets(red, P, **kw)),
            (names[1], lambda: tg.calc_probs_datasets(keyed, P, **kw))]

    def timed_pass(fn):
        torch.manual_seed(1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    times, fpp = {name: [] for name, _ in runs}, {}
    for name, fn in runs:
        timed_pass(fn)
    for _ in range(ROUNDS):
        for name, fn in runs:
            times[name].append(timed_pass(fn))
            fpp[name] = tg.FPP
    med = {}
    for name, _ in runs:
        v = np.sort(times[name])
        med[name] = float(np.median(v))
        print("e2e     %-52s median %.4f s  min %.4f s  max %.4f s  (%d rounds, FPP %.6g)"
              % (name, med[name], v[0], v[-1], v.size, fpp[name]), flush=True)
    print("e2e     the two columns cost %.4f s (%.1f %%) more than red_sigma alone"
          % (med[names[1]] - med[names[0]], 100.0 * (med[names[1]] / med[names[0]] - 1.0)), flush=True)


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
    me = os.path.abspath(__file__)
    with open(path, "w") as out:
        out.write("# profiles/gls/measure.py on one MI355X: a 512 MiB grid per kernel case, device events, best of %d runs, the "
                  "variants taking turns; wall clock of whole calls end to end, median of %d rounds\n" % (ROUNDS, ROUNDS))
        out.flush()
        ok = _step(out, 180, [sys.executable, me, "kernels"])
        ok = ok and _step(out, 300, [sys.executable, me, "e2e"])
        out.write("job %s\n" % ("complete" if ok else "ended early"))
    return 0 if ok else 1


if __name__ == "__main__":
    if sys.argv[1:2] == ["kernels"]:
        kernels()
    elif sys.argv[1:2] == ["e2e"]:
        e2e()
    else:
        dest = (sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv
                else os.path.join(os.path.dirname(os.path.abspath(__file__)), "results.txt"))
        sys.exit(job(dest))
