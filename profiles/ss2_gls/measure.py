"""Measurements of DESIGN.md section 14, baseline columns marginalised under correlated noise with a two-dimensional state
(`red_kernel_baseline` next to `red_kernel` = "matern32" / "ou2", scan_rows_kernel<ONE, Ss2ColsFilter<K>>).

  python profiles/ss2_gls/measure.py            the whole job: each GPU step a child process under its own time limit, the
                                                next one only after the last ended well; writes profiles/ss2_gls/results.txt
                                                (or --out FILE)
  python profiles/ss2_gls/measure.py kernels    (a) _lib.chi2_grid_ss2_baseline with K = 1, 2, 4 columns u^p, flat priors, under
                                                a Matern-3/2 and a two-term table on a 512 MiB grid at n_time = 100 and 2048
                                                against the Ss2Filter kernel (_lib.chi2_grid_ss2) on the same grid and tables:
                                                the same bytes and the same scan, K x 2 fma a pair and K wave totals a row
                                                more, and fewer resident waves where the registers say so.  One warm-up of
                                                each, then five rounds in which they take turns, each run timed with device
                                                events; the best of the five
  python profiles/ss2_gls/measure.py dense      (b) the only alternative without the kernel, for finite priors: torch.linalg.cholesky
                                                of K + B diag(s^2) B^T once, then torch.cholesky_solve on the residual matrix of
                                                the same grid and the row sums of r * C^-1 r; the factorisation is not timed
  python profiles/ss2_gls/measure.py e2e        (c) TOI-465.01, N = 1e6, two datasets of 50 points: calc_probs_datasets with
                                                red_kernel = "matern32" on the second dataset, with and without the columns
                                                [1, u] next to it; wall clock of whole calls, taking turns
  python profiles/ss2_gls/measure.py ab LIB     (d) three against four resident waves a SIMD on the same code: LIB is a build of
                                                the same sources whose kSs2ColsBlocksPerCu says 3 for every single-trip
                                                instantiation (trx_ss2_cols.hpp: {3, 3, 3, 3} in the ONE row; build()'s flags).
                                                K = 1 and K = 3 at 100 stamps -- 116 and 124 VGPRs, resident four times -- through
                                                both libraries in one process, taking turns; K = 2 (three either way) as the
                                                control.  Not part of the whole job (--out FILE appends the lines to FILE)
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
KS = (1, 2, 4)


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
    """stamps, errors, the two datasets (Matern-3/2, two OU terms), the flux and the columns u^0 .. u^3 of one shape"""
    import numpy as np
    from triceratops_amd import datasets as D
    rng = np.random.default_rng(n_time)
    t = np.cumsum(rng.uniform(0.3, 1.7, n_time))
    err = 1e-3 * rng.uniform(0.6, 1.8, n_time)
    base = {"time": t, "flux": np.ones(n_time), "flux_err": err}
    sets = D.validate([dict(base, red_kernel="matern32", red_sigma=3e-3, red_timescale=10.0),
                       dict(base, red_kernel="ou2", red_sigma=(3e-3, 1.5e-3), red_timescale=(2.0, 70.0))])
    u = (t - 0.5 * (t[0] + t[-1])) / (0.5 * (t[-1] - t[0]))
    return t, err, sets, 1.0 + err * rng.normal(0.0, 1.0, n_time), np.stack([u ** p for p in range(4)])


def _on_device(system):
    import numpy as np
    from triceratops_amd import _lib
    return tuple(_lib.dev(np.ascontiguousarray(v)) for v in (system.A, system.g, system.omega, system.c))


def kernels():
    import torch
    from triceratops_amd import _lib
    from triceratops_amd import datasets as D

    for n_time in N_TIMES:
        n = GRID_BYTES // (8 * n_time)
        _, _, sets, f, B = _light_curve(n_time)
        torch.manual_seed(n_time)
        flux = _lib.dev(f)
        grid = 1.0 + 3e-4 * torch.randn((n, n_time), dtype=torch.float64, device="cuda")
        out = torch.zeros(n, dtype=torch.float64, device="cuda")
        for d in sets:
            systems = {K: D.ss2_baseline_system(d, B[:K], float("inf")) for K in KS}
            dev = {K: _on_device(s) for K, s in systems.items()}
            plain = dev[KS[0]][:3]
            runs = [("ss2", lambda: _lib.chi2_grid_ss2(flux, grid, *plain, out=out))]
            for K in KS:
                runs.append(("K=%d" % K, lambda K=K: _lib.chi2_grid_ss2_baseline(flux, grid, *dev[K], systems[K].minv, out=out)))
            for _, fn in runs:
                fn()
            torch.cuda.synchronize()
            times = {name: [] for name, _ in runs}
            for _ in range(ROUNDS):
                for name, fn in runs:
                    times[name].append(_timed(fn))
            best = {name: min(v) for name, v in times.items()}
            moved = n * n_time * 8
            print("events  %d rows x %d stamps (%.0f MiB) %-8s  Ss2Filter %.4f ms (%.2f TB/s)   %s   (best of %d, taking turns; %s)"
                  % (n, n_time, moved / 2 ** 20, d.red_kernel, best["ss2"] * 1e3, moved / best["ss2"] / 1e12,
                     "   ".join("Ss2ColsFilter %s %.4f ms (%.2f TB/s, %.2f x, %d blocks a CU)"
                                % (name, best[name] * 1e3, moved / best[name] / 1e12, best[name] / best["ss2"],
                                   _lib.ss2_baseline_blocks(10 ** 9, n_time, int(name[2:])) // 256) for name, _ in runs[1:]),
                     ROUNDS, "; ".join("%s %s ms" % (name, " ".join("%.4f" % (v * 1e3) for v in times[name])) for name, _ in runs)),
                  flush=True)
        del grid


def ab(variant, path=None):
    import torch
    from triceratops_amd import _lib
    from triceratops_amd import datasets as D

    libs = {"as built": _lib.lib(), "three": _lib._load(os.path.abspath(variant), False)}
    n_time = 100
    n = GRID_BYTES // (8 * n_time)
    _, _, sets, f, B = _light_curve(n_time)
    torch.manual_seed(n_time)
    flux = _lib.dev(f)
    grid = 1.0 + 3e-4 * torch.randn((n, n_time), dtype=torch.float64, device="cuda")
    outs = {name: torch.zeros(n, dtype=torch.float64, device="cuda") for name in libs}
    lines = []
    for K in (1, 2, 3):
        system = D.ss2_baseline_system(sets[0], B[:K], float("inf"))
        dev = _on_device(system)

        def call(name, K=K, dev=dev, system=system):
            _lib._lib = libs[name]                                 # (the wrapper calls the library in use)
            try:
                _lib.chi2_grid_ss2_baseline(flux, grid, *dev, system.minv, out=outs[name])
            finally:
                _lib._lib = libs["as built"]
        for name in libs:
            outs[name].zero_()
            call(name)
        torch.cuda.synchronize()
        same = torch.equal(outs["as built"], outs["three"])
        times = {name: [] for name in libs}
        for _ in range(ROUNDS):
            for name in libs:
                times[name].append(_timed(lambda: call(name)))
        best = {name: min(v) for name, v in times.items()}
        lines.append("ab      %d rows x %d stamps matern32 K=%d  as built (%d blocks a CU) %.4f ms   capped at 3 blocks a CU %.4f ms "
                     "(%.3f x)   the same bits: %s   (best of %d, taking turns; %s)"
                     % (n, n_time, K, _lib.ss2_baseline_blocks(10 ** 9, n_time, K) // 256, best["as built"] * 1e3,
                        best["three"] * 1e3, best["three"] / best["as built"], same, ROUNDS,
                        "; ".join("%s %s ms" % (name, " ".join("%.4f" % (v * 1e3) for v in times[name])) for name in libs)))
        print(lines[-1], flush=True)
    if path:
        with open(path, "a") as out:
            out.write("# measure.py ab: the same sources built with {3, 3, 3, 3} in the ONE row of kSs2ColsBlocksPerCu\n"
                      + "\n".join(lines) + "\n")
    return 0


def dense():
    import numpy as np
    import torch
    from triceratops_amd import _lib
    from triceratops_amd import datasets as D

    K = 2
    for n_time in N_TIMES:
        n = GRID_BYTES // (8 * n_time)
        t, err, (d_m32, _), f, B = _light_curve(n_time)
        flat = D.ss2_baseline_system(d_m32, B[:K], float("inf"))
        sig = 1.0 / np.sqrt(flat.D)                                    # A~ + I
        system = D.ss2_baseline_system(d_m32, B[:K], sig)
        dev = _on_device(system)
        x = np.sqrt(3.0) * np.abs(t[:, None] - t[None, :]) / d_m32.red_timescale
        C = np.diag(err ** 2) + d_m32.red_sigma ** 2 * (1.0 + x) * np.exp(-x) + B[:K].T @ np.diag(sig ** 2) @ B[:K]
        L = torch.linalg.cholesky(_lib.dev(C))
        torch.manual_seed(n_time)
        flux = _lib.dev(f)
        grid = 1.0 + 3e-4 * torch.randn((n, n_time), dtype=torch.float64, device="cuda")

        def solve():
            r = (flux[None, :] - grid).T                          # [n_time][n]: the right-hand sides as columns
            return 0.5 * torch.sum(r * torch.cholesky_solve(r, L), dim=0)

        def kernel():
            return _lib.chi2_grid_ss2_baseline(flux, grid, *dev, system.minv)

        want, got = solve(), kernel()
        rel = float(((got - want).abs() / want).max())
        runs = [("kernel", kernel), ("dense", solve)]
        times = {name: [] for name, _ in runs}
        for _ in range(ROUNDS):
            for name, fn in runs:
                times[name].append(_timed(fn))
        best = {name: min(v) for name, v in times.items()}
        print("dense   %d rows x %d stamps  Ss2ColsFilter matern32 K=%d, finite priors %.4f ms   cholesky_solve + row sums %.4f ms "
              "(%.0f x)   (best of %d, taking turns; %s; largest relative difference of the two results %.3g)"
              % (n, n_time, K, best["kernel"] * 1e3, best["dense"] * 1e3, best["dense"] / best["kernel"], ROUNDS,
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
    from triceratops_amd import lightcurve as lc
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
    red = [two[0], dict(two[1], red_kernel="matern32", red_sigma=2.0 * s, red_timescale=20.0 * cadence)]
    keyed = [two[0], dict(red[1], red_kernel_baseline=lc.trend_columns(two[1]["time"], 1))]
    names = ("2 datasets of 50 points, red_kernel = matern32 on the second", "the same + red_kernel_baseline [1, u]")
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
        print("e2e     %-62s median %.4f s  min %.4f s  max %.4f s  (%d rounds, FPP %.6g)"
              % (name, med[name], v[0], v[-1], v.size, fpp[name]), flush=True)
    print("e2e     the two columns cost %.4f s (%.1f %%) more than the kernel alone"
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
        out.write("# profiles/ss2_gls/measure.py on one MI355X: a 512 MiB grid per kernel case, device events, best of %d runs, "
                  "the variants taking turns; wall clock of whole calls end to end, median of %d rounds\n" % (ROUNDS, ROUNDS))
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
    elif sys.argv[1:2] == ["ab"]:
        sys.exit(ab(sys.argv[2], sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None))
    else:
        dest = (sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv
                else os.path.join(os.path.dirname(os.path.abspath(__file__)), "results.txt"))
        sys.exit(job(dest))
