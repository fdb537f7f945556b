"""Measurements of DESIGN.md section 14, correlated noise with a two-dimensional state (`red_kernel` = "matern32" / "ou2" next
to `red_sigma` / `red_timescale`, scan_rows_kernel<ONE, Ss2Filter>).

  python profiles/ss2/measure.py            the whole job: each GPU step a child process under its own time limit, the next
                                            one only after the last ended well; writes profiles/ss2/results.txt (or --out FILE)
  python profiles/ss2/measure.py kernels    (a) the Ss2Filter kernel (_lib.chi2_grid_ss2) with a Matern-3/2 and a two-term table on
                                            a 512 MiB grid at n_time = 100 and 2048 against the OuFilter kernel (_lib.chi2_grid_ou) on
                                            the same grid: the same bytes, about four times the scan's arithmetic.  One warm-up
                                            of each, then five rounds in which they take turns, each run timed with device
                                            events; the best of the five
  python profiles/ss2/measure.py dense      (b) the only alternative without the kernel: torch.linalg.cholesky of K once, then
                                            torch.cholesky_solve on the residual matrix of the same grid and the row sums of
                                            r * K^-1 r; the factorisation is not timed
  python profiles/ss2/measure.py pmc        (d) which resource bounds the Ss2Filter kernel: one rocprofv3 --pmc child (counters alone, no
                                            tracing) of `once` -- every kernel of (a) launched twice on the same grids --, the
                                            SQ counters per dispatch summed by kernel.  Not part of the whole job: run it on
                                            its own (--out FILE appends the lines to FILE)
  python profiles/ss2/measure.py e2e        (c) TOI-465.01, N = 1e6, two datasets of 50 points: calc_probs_datasets with
                                            red_kernel = "matern32" on the second dataset against the same run with the plain
                                            red_sigma / red_timescale keys; wall clock of whole calls, taking turns
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
N_TIMES = (100, 2048)


def _timed(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3


def _light_curve(n_time):
    """stamps, errors, the three datasets (one OU term, Matern-3/2, two OU terms) and the flux of one shape"""
    import numpy as np
    from triceratops_amd import datasets as D
    rng = np.random.default_rng(n_time)
    t = np.cumsum(rng.uniform(0.3, 1.7, n_time))
    err = 1e-3 * rng.uniform(0.6, 1.8, n_time)
    base = {"time": t, "flux": np.ones(n_time), "flux_err": err}
    sets = D.validate([dict(base, red_sigma=3e-3, red_timescale=10.0),
                       dict(base, red_kernel="matern32", red_sigma=3e-3, red_timescale=10.0),
                       dict(base, red_kernel="ou2", red_sigma=(3e-3, 1.5e-3), red_timescale=(2.0, 70.0))])
    return t, err, sets, 1.0 + err * rng.normal(0.0, 1.0, n_time)


def kernels():
    import numpy as np
    import torch
    from triceratops_amd import _lib
    from triceratops_amd import datasets as D

    for n_time in N_TIMES:
        n = GRID_BYTES // (8 * n_time)
        t, err, (d_ou, d_m32, d_ou2), f = _light_curve(n_time)
        abw = tuple(_lib.dev(v) for v in D.ou_system(d_ou))
        m32 = tuple(_lib.dev(np.ascontiguousarray(v)) for v in D.ss2_system(d_m32))
        ou2 = tuple(_lib.dev(np.ascontiguousarray(v)) for v in D.ss2_system(d_ou2))
        torch.manual_seed(n_time)
        flux = _lib.dev(f)
        grid = 1.0 + 3e-4 * torch.randn((n, n_time), dtype=torch.float64, device="cuda")
        out = torch.zeros(n, dtype=torch.float64, device="cuda")
        runs = [("ou", lambda: _lib.chi2_grid_ou(flux, grid, *abw, out=out)),
                ("matern32", lambda: _lib.chi2_grid_ss2(flux, grid, *m32, out=out)),
                ("ou2", lambda: _lib.chi2_grid_ss2(flux, grid, *ou2, out=out))]
        for _, fn in runs:
            fn()
        torch.cuda.synchronize()
        times = {name: [] for name, _ in runs}
        for _ in range(ROUNDS):
            for name, fn in runs:
                times[name].append(_timed(fn))
        best = {name: min(v) for name, v in times.items()}
        moved = n * n_time * 8
        print("events  %d rows x %d stamps (%.0f MiB)  chi2_ou_kernel %.4f ms (%.2f TB/s)   %s   (best of %d, taking turns; %s)"
              % (n, n_time, moved / 2 ** 20, best["ou"] * 1e3, moved / best["ou"] / 1e12,
                 "   ".join("ss2_kernel %s %.4f ms (%.2f TB/s, %.2f x)" % (name, best[name] * 1e3, moved / best[name] / 1e12,
                                                                         best[name] / best["ou"]) for name, _ in runs[1:]),
                 ROUNDS, "; ".join("%s %s ms" % (name, " ".join("%.4f" % (v * 1e3) for v in times[name])) for name, _ in runs)),
              flush=True)
        del grid


PMC = ("SQ_WAVE_CYCLES", "SQ_BUSY_CYCLES", "SQ_ACTIVE_INST_ANY", "SQ_ACTIVE_INST_VALU", "SQ_ACTIVE_INST_LDS", "SQ_WAIT_ANY",
       "SQ_WAIT_INST_ANY", "SQ_INSTS_VALU")


def once():
    """the launches the counter run looks at: per shape chi2_ou_kernel and ss2_kernel (Matern-3/2 tables), twice each"""
    import numpy as np
    import torch
    from triceratops_amd import _lib
    from triceratops_amd import datasets as D
    for n_time in N_TIMES:
        n = GRID_BYTES // (8 * n_time)
        _, _, (d_ou, d_m32, _), f = _light_curve(n_time)
        abw = tuple(_lib.dev(v) for v in D.ou_system(d_ou))
        m32 = tuple(_lib.dev(np.ascontiguousarray(v)) for v in D.ss2_system(d_m32))
        torch.manual_seed(n_time)
        flux = _lib.dev(f)
        grid = 1.0 + 3e-4 * torch.randn((n, n_time), dtype=torch.float64, device="cuda")
        for _ in range(2):
            _lib.chi2_grid_ou(flux, grid, *abw)
            _lib.chi2_grid_ss2(flux, grid, *m32)
        torch.cuda.synchronize()
        del grid


def pmc(path=None):
    import csv
    import glob
    import shutil
    import tempfile
    d = tempfile.mkdtemp(prefix="ss2_pmc_")
    cmd = ["rocprofv3", "--pmc"] + list(PMC) + ["--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
                                                "once"]
    r = subprocess.run(["timeout", "-k", "10", "240"] + cmd, cwd=ROOT, capture_output=True, text=True)
    if r.returncode != 0:
        print("pmc     the counter run failed with status %d\n%s" % (r.returncode, r.stderr[-2000:]))
        return 1
    total, count = {}, {}
    for name in glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True):
        for row in csv.DictReader(open(name)):
            kernel = row["Kernel_Name"]
            # (scan_rows_kernel<ONE, Ss2Filter> and <ONE, OuFilter>; the lines keep the names results.txt has)
            which = "ss2_kernel" if "Ss2Filter" in kernel else "chi2_ou_kernel" if "OuFilter" in kernel else None
            if which is None or "scan_rows_kernel" not in kernel:
                continue
            key = (which + ("<ONE> 100 stamps" if ("<true" in kernel or "ILb1E" in kernel) else " 2048 stamps"))
            total.setdefault(key, {}).setdefault(row["Counter_Name"], 0.0)
            total[key][row["Counter_Name"]] += float(row["Counter_Value"])
            count.setdefault(key, set()).add(row["Dispatch_Id"])
    lines = []
    for key in sorted(total):
        c, k = total[key], len(count[key])
        wave = c.get("SQ_WAVE_CYCLES", 0.0)
        lines.append("pmc     %-30s %d dispatches  %s   of the wave cycles: an instruction issued %.2f (VALU %.2f, LDS %.2f), waiting "
                     "on a count or barrier %.2f, issue stalled %.2f" % (
                         key, k, "  ".join("%s %.4g" % (name, c.get(name, float("nan")) / k) for name in PMC),
                         c.get("SQ_ACTIVE_INST_ANY", 0.0) / wave, c.get("SQ_ACTIVE_INST_VALU", 0.0) / wave,
                         c.get("SQ_ACTIVE_INST_LDS", 0.0) / wave, c.get("SQ_WAIT_ANY", 0.0) / wave,
                         c.get("SQ_WAIT_INST_ANY", 0.0) / wave))
    shutil.rmtree(d, ignore_errors=True)
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    if path:
        with open(path, "a") as out:
            out.write("# rocprofv3 --pmc (counters alone) over `measure.py once`: per dispatch, summed over the chip\n" + text)
    return 0 if lines else 1


def dense():
    import numpy as np
    import torch
    from triceratops_amd import _lib
    from triceratops_amd import datasets as D

    for n_time in N_TIMES:
        n = GRID_BYTES // (8 * n_time)
        t, err, (_, d_m32, _), f = _light_curve(n_time)
        m32 = tuple(_lib.dev(np.ascontiguousarray(v)) for v in D.ss2_system(d_m32))
        x = np.sqrt(3.0) * np.abs(t[:, None] - t[None, :]) / d_m32.red_timescale
        K = _lib.dev(np.diag(err ** 2) + d_m32.red_sigma ** 2 * (1.0 + x) * np.exp(-x))
        L = torch.linalg.cholesky(K)
        torch.manual_seed(n_time)
        flux = _lib.dev(f)
        grid = 1.0 + 3e-4 * torch.randn((n, n_time), dtype=torch.float64, device="cuda")

        def solve():
            r = (flux[None, :] - grid).T                          # [n_time][n]: the right-hand sides as columns
            return 0.5 * torch.sum(r * torch.cholesky_solve(r, L), dim=0)

        def kernel():
            return _lib.chi2_grid_ss2(flux, grid, *m32)

        want, got = solve(), kernel()
        rel = float(((got - want).abs() / want).max())
        runs = [("ss2", kernel), ("dense", solve)]
        times = {name: [] for name, _ in runs}
        for _ in range(ROUNDS):
            for name, fn in runs:
                times[name].append(_timed(fn))
        best = {name: min(v) for name, v in times.items()}
        print("dense   %d rows x %d stamps  ss2_kernel matern32 %.4f ms   cholesky_solve + row sums %.4f ms (%.0f x)   (best of %d, "
              "taking turns; %s; largest relative difference of the two results %.3g)"
              % (n, n_time, best["ss2"] * 1e3, best["dense"] * 1e3, best["dense"] / best["ss2"], ROUNDS,
                 "; ".join("%s %s ms" % (name, " ".join("%.4f" % (v * 1e3) for v in times[name])) for name, _ in runs), rel),
              flush=True)
        del grid


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
    cadence = float(np.median(np.diff(two[1]["time"])))
    red = [two[0], dict(two[1], red_sigma=2.0 * s, red_timescale=20.0 * cadence)]
    keyed = [two[0], dict(red[1], red_kernel="matern32")]
    names = ("2 datasets of 50 points, red_sigma on the second", "the same + red_kernel = matern32")
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
    print("e2e     the Matern-3/2 kernel costs %.4f s (%.1f %%) more than the one exponential term"
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
        out.write("# profiles/ss2/measure.py on one MI355X: a 512 MiB grid per kernel case, device events, best of %d runs, the "
                  "variants taking turns; wall clock of whole calls end to end, median of %d rounds\n" % (ROUNDS, ROUNDS))
        out.flush()
        ok = _step(out, 180, [sys.executable, me, "kernels"])
        ok = ok and _step(out, 240, [sys.executable, me, "dense"])
        ok = ok and _step(out, 300, [sys.executable, me, "e2e"])
        out.write("job %s\n" % ("complete" if ok else "ended early"))
    return 0 if ok else 1


if __name__ == "__main__":
    if sys.argv[1:2] == ["kernels"]:
        kernels()
    elif sys.argv[1:2] == ["dense"]:
        dense()
    elif sys.argv[1:2] == ["e2e"]:
        e2e()
    elif sys.argv[1:2] == ["once"]:
        once()
    elif sys.argv[1:2] == ["pmc"]:
        sys.exit(pmc(sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None))
    else:
        dest = (sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv
                else os.path.join(os.path.dirname(os.path.abspath(__file__)), "results.txt"))
        sys.exit(job(dest))
