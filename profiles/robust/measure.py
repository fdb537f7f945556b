"""Measurements of DESIGN.md section 14, the outlier-tolerant likelihood per dataset (`outlier_frac` / `outlier_scale`,
chi2_robust_kernel).

  python profiles/robust/measure.py            the whole job: each GPU step a child process under its own time limit, the
                                               next one only after the last ended well; writes profiles/robust/results.txt
                                               (or --out FILE)
  python profiles/robust/measure.py kernels    (a) chi2_robust_kernel (_lib.chi2_grid_robust) on a 512 MiB grid at
                                               n_time = 100 and 2048 against chi2_rows_kernel<STAGE, Chi2Plain>
                                               (_lib.chi2_grid_weighted) on the same grid -- the difference is the price of the
                                               exp and the log1p per value -- and against the same statement written in torch
                                               operators on the same buffer, the only alternative a user has.  One warm-up of
                                               each, then five rounds in which the three take turns, each run timed with device
                                               events; the best of the five
  python profiles/robust/measure.py e2e        (b) TOI-465.01, N = 1e6, two datasets of 50 points: calc_probs_datasets without
                                               the keys and with them on the second dataset; wall clock of whole calls, taking
                                               turns
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
PAIR = (0.05, 10.0)


def kernels():
    import torch
    from triceratops_amd import _lib
    from triceratops_amd.datasets import robust_constants
    c0, c1, k2 = robust_constants(*PAIR)

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
        torch.manual_seed(n_time)
        sigma = 1e-3 * (1.0 + torch.rand(n_time, dtype=torch.float64, device="cuda"))
        w = 1.0 / (sigma * sigma)
        flux = 1.0 + sigma * torch.randn(n_time, dtype=torch.float64, device="cuda")
        flux[n_time // 2] += 8.0 * sigma[n_time // 2]
        grid = 1.0 + 3e-4 * torch.randn((n, n_time), dtype=torch.float64, device="cuda")
        out = torch.zeros(n, dtype=torch.float64, device="cuda")

        def robust():
            return _lib.chi2_grid_robust(flux, w, grid, c0, c1, k2, out=out)

        def plain():
            return _lib.chi2_grid_weighted(flux, w, grid, out=out)

        def composed():
            d = flux - grid
            a = 0.5 * (w * d) * d
            A, B = a + c0, a * k2 + c1
            return out.add_((torch.minimum(A, B) - torch.log1p(torch.exp(-(A - B).abs()))).sum(dim=1))

        x = _lib.chi2_grid_robust(flux, w, grid, c0, c1, k2)
        out.zero_()
        y = composed().clone()
        robust()
        plain()
        torch.cuda.synchronize()
        diff = float(((x - y).abs() / (1.0 + x)).max().cpu())
        times = {"robust": [], "plain": [], "composed": []}
        for _ in range(ROUNDS):
            for name, fn in (("robust", robust), ("plain", plain), ("composed", composed)):
                times[name].append(timed(fn))
        tr, tp, tc = (min(times[k]) for k in ("robust", "plain", "composed"))
        moved = n * n_time * 8
        print("events  %d rows x %d stamps (%.0f MiB)  chi2_robust_kernel %.4f ms (%.2f TB/s, %.2f ns per 1000 values)   "
              "chi2_rows_kernel<Chi2Plain> %.4f ms (%.2f TB/s)   robust / plain = %.2f   torch operators %.4f ms   "
              "torch / robust = %.2f   (best of %d, taking turns; robust %s ms; plain %s ms; torch %s ms; max relative "
              "difference of the two results %.2g)"
              % (n, n_time, moved / 2 ** 20, tr * 1e3, moved / tr / 1e12, tr * 1e12 / (n * n_time), tp * 1e3,
                 moved / tp / 1e12, tr / tp, tc * 1e3, tc / tr, ROUNDS, " ".join("%.4f" % (t * 1e3) for t in times["robust"]),
                 " ".join("%.4f" % (t * 1e3) for t in times["plain"]), " ".join("%.4f" % (t * 1e3) for t in times["composed"]),
                 diff), flush=True)
        del grid, x, y


def e2e():
    """wall clock of whole calls, each ended by a device synchronise: one warm-up of every case, then ROUNDS rounds in which
    they take turns"""
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
    two = [{"time": t[k::2], "flux": f[k::2], "flux_err": s} for k in (0, 1)]
    keyed = [two[0], dict(two[1], outlier_frac=PAIR[0], outlier_scale=PAIR[1])]
    names = ("2 datasets of 50 points, no keys", "2 datasets of 50 points, the keys on the second")
    runs = [(names[0], lambda: tg.calc_probs_datasets(two, P, **kw)),
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
    print("e2e     the keys on the second dataset cost %.4f s (%.1f %%) more than none"
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
        out.write("# profiles/robust/measure.py on one MI355X: a 512 MiB grid per kernel case, device events, best of %d runs, the "
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
