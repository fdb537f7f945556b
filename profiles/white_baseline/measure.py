"""Measurements of DESIGN.md section 14, baseline terms marginalised next to white-noise candidates (`white_baseline` next to
`white_grid`, chi2_white_lin_kernel).

  python profiles/white_baseline/measure.py          the whole job: each GPU step a child process under its own time limit,
                                                     the next one only after the last ended well; writes
                                                     profiles/white_baseline/results.txt (or --out FILE)
  python profiles/white_baseline/measure.py kernels  chi2_white_lin_kernel (_lib.chi2_grid_white_baseline, one pass over the
                                                     grid) on a 512 MiB grid, n_time = 100 and 2048, J = 2, 4, 8, K = 1, 2, 4,
                                                     against
                                                     (b) the only alternative without the kernel: J calls of
                                                         _lib.chi2_grid_baseline, each on its candidate's own system, into a
                                                         [J][n] buffer and one _lib.softmin_rows;
                                                     (c) _lib.chi2_grid_white_mix at the same J: the price of the columns.
                                                     One warm-up of each, then five rounds in which they take turns, each run
                                                     timed with device events; the best of the five
  python profiles/white_baseline/measure.py e2e      TOI-465.01, N = 1e6, two datasets of 50 points: calc_probs_datasets
                                                     without a key, with eight candidates on the second dataset, and with a
                                                     constant and a slope marginalised next to them; wall clock of whole
                                                     calls, taking turns, the median of five
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
SCALES, JITTERS = (1.0, 1.5, 2.0, 3.0), (0.0, 0.5)           # jitters in units of the mean error


def _tables(nt, J, K, rng, sigma):
    import numpy as np
    from triceratops_amd.datasets import linear_system, validate, white_baseline_system, white_baselines, white_grids
    from triceratops_amd.lightcurve import white_noise_grid
    err = rng.uniform(0.5, 2.0, nt) * sigma
    u = np.linspace(-1.0, 1.0, nt)
    B = np.stack([u ** p for p in range(K)])
    dicts = [{"time": np.arange(nt, dtype=np.float64), "flux": np.ones(nt), "flux_err": err,
              "white_grid": white_noise_grid(SCALES, [s * sigma for s in JITTERS])[:J], "white_baseline": B}]
    sets = validate(dicts)
    system = white_baseline_system(sets[0], white_grids(dicts, sets)[0], *white_baselines(dicts, sets)[0])
    per = [linear_system(system.w[j], B, np.inf) for j in range(J)]
    return 1.0 + rng.normal(0.0, sigma, nt) + 3.0 * sigma * u ** (K - 1), system, per


def kernels():
    import numpy as np
    import torch
    from triceratops_amd import _lib, synth
    rng = np.random.default_rng(synth.SEED)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e-3

    for nt in (100, 2048):
        n = GRID_BYTES // (8 * nt)
        grid = 1.0 - 2e-3 * torch.rand((n, nt), dtype=torch.float64, device="cuda")
        one_pass = n * nt * 8 + n * 8
        for J in (2, 4, 8):
            for K in (1, 2, 4):
                f, system, per = _tables(nt, J, K, rng, synth.SIGMA)
                f_d, w_d, B_d = _lib.dev(f), _lib.dev(system.w), _lib.dev(system.B)
                g_d = [_lib.dev(p.g) for p in per]
                bufs = torch.empty((J, n), dtype=torch.float64, device="cuda")
                out = torch.empty(n, dtype=torch.float64, device="cuda")

                def lin():
                    return _lib.chi2_grid_white_baseline(f_d, grid, w_d, B_d, system.minv, system.lnc, out=out.zero_())

                def composed():
                    for j in range(J):
                        _lib.chi2_grid_baseline(f_d, w_d[j], grid, g_d[j], per[j].minv, out=bufs[j].zero_())
                    return _lib.softmin_rows(bufs, system.lnc, out=out.zero_())

                def mix():
                    return _lib.chi2_grid_white_mix(f_d, grid, w_d, system.lnc, out=out.zero_())

                x = lin().clone()
                y = composed().clone()
                mix()
                runs = [("lin", lin), ("composed", composed), ("mix", mix)]
                torch.cuda.synchronize()
                diff = float(((x - y).abs() / (1.0 + x)).max().cpu())
                times = {name: [] for name, _ in runs}
                for _ in range(ROUNDS):
                    for name, fn in runs:
                        times[name].append(timed(fn))
                t = {name: min(v) for name, v in times.items()}
                line = ("events  %d x %d  J = %d  K = %d  chi2_white_lin_kernel %.3f ms (%.2f TB/s of %.2f GB)   "
                        "(b) %d x chi2_rows_kernel<Chi2Baseline> + softmin_rows %.3f ms: (b) / lin = %.2f   "
                        "(c) chi2_white_mix_kernel %.3f ms: lin / (c) = %.2f"
                        % (n, nt, J, K, t["lin"] * 1e3, one_pass / t["lin"] / 1e12, one_pass / 1e9, J, t["composed"] * 1e3,
                           t["composed"] / t["lin"], t["mix"] * 1e3, t["lin"] / t["mix"]))
                line += ("   (best of %d, taking turns; %s; max |lin - (b)| / (1 + T) %.2g)"
                         % (ROUNDS, "; ".join("%s %s ms" % (name, " ".join("%.3f" % (v * 1e3) for v in times[name]))
                                              for name, _ in runs), diff))
                print(line, flush=True)
        del grid


def e2e():
    """wall clock of whole calls, each ended by a device synchronise: one warm-up of every case, then ROUNDS rounds in which
    they take turns"""
    import numpy as np
    import pandas as pd
    import torch
    from helpers import GOLD, gold
    import triceratops_amd as ta
    from triceratops_amd.lightcurve import trend_columns, white_noise_grid
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
    grid = white_noise_grid([1.0, 1.5, 2.0, 3.0], [0.0, 0.5 * s])
    eight = [two[0], dict(two[1], white_grid=grid)]
    trend = [two[0], dict(two[1], white_grid=grid, white_baseline=trend_columns(two[1]["time"], 1),
                          white_baseline_sigma=[np.inf, 5.0 * s])]
    runs = [("2 datasets of 50 points, no key", lambda: tg.calc_probs_datasets(two, P, **kw)),
            ("2 datasets of 50 points, eight candidates on the second", lambda: tg.calc_probs_datasets(eight, P, **kw)),
            ("... and a constant and a slope marginalised next to them", lambda: tg.calc_probs_datasets(trend, P, **kw))]

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
    for name, _ in runs:
        v = np.sort(times[name])
        print("e2e     %-58s median %.4f s  min %.4f s  max %.4f s  (%d rounds, %d scenarios, FPP %.6g)"
              % (name, np.median(v), v[0], v[-1], v.size, tg.lnZ.size, fpp[name]), flush=True)
    best = int(np.nanargmax(tg.lnZ))
    print("e2e     at the most probable scenario's best draw: candidates' weights %s, mean coefficients %s"
          % (np.array2string(tg.dataset_white_noise[best][1]["weight"], precision=3),
             np.array2string(tg.dataset_white_baselines[best][1]["mean"], precision=3)), flush=True)


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
        out.write("# profiles/white_baseline/measure.py on one MI355X: a 512 MiB grid per kernel case, device events, best of %d "
                  "runs, the variants taking turns; wall clock of whole calls end to end\n" % ROUNDS)
        out.flush()
        ok = _step(out, 400, [sys.executable, me, "kernels"])
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
