"""Measurements of DESIGN.md section 14, white-noise candidates marginalised per draw (`white_grid`, chi2_white_mix_kernel).

  python profiles/white_mix/measure.py          the whole job: each GPU step a child process under its own time limit, the
                                                next one only after the last ended well; writes profiles/white_mix/results.txt
                                                (or --out FILE)
  python profiles/white_mix/measure.py kernels  chi2_white_mix_kernel (_lib.chi2_grid_white_mix, one pass over the grid) on a
                                                512 MiB grid, n_time = 100 and 2048, J = 1, 2, 4, 8, against
                                                (a) chi2_rows_kernel<STAGE, Chi2Plain> (_lib.chi2_grid_weighted) on the same
                                                    grid: the floor, one pass of the same bytes;
                                                (b) the only alternative without the kernel: J calls of
                                                    _lib.chi2_grid_weighted into a [J][n] buffer and one _lib.softmin_rows;
                                                (c) what a user had to do before: _lib.chi2_grid_ou_mix with tau = 1e-6
                                                    cadences and the jitters as s_r.
                                                One warm-up of each, then five rounds in which the four take turns, each run
                                                timed with device events; the best of the five
  python profiles/white_mix/measure.py e2e      TOI-465.01, N = 1e6, two datasets of 50 points: calc_probs_datasets without the
                                                key and with an 8-row grid (4 scales x 2 jitters) on the second dataset, wall
                                                clock of whole calls, taking turns, the median of five
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
RED_JITTERS = (0.25, 0.5, 0.75, 1.0, 1.5, 2.0, 2.5, 3.0)     # (c): s_r > 0 for every candidate


def _tables(nt, J, rng, sigma):
    import numpy as np
    from triceratops_amd.datasets import ou_mix_system, validate, white_grids, white_mix_system
    from triceratops_amd.lightcurve import red_noise_grid, white_noise_grid
    err = rng.uniform(0.5, 2.0, nt) * sigma
    base = {"time": np.arange(nt, dtype=np.float64), "flux": np.ones(nt), "flux_err": err}
    dicts = [dict(base, white_grid=white_noise_grid(SCALES, [s * sigma for s in JITTERS])[:J])]
    sets = validate(dicts)
    white = white_mix_system(sets[0], white_grids(dicts, sets)[0])
    red = validate([dict(base, red_grid=red_noise_grid([s * sigma for s in RED_JITTERS[:J]], [1e-6]))])[0]
    return 1.0 + rng.normal(0.0, sigma, nt), err, white, ou_mix_system(red)


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
        for J in (1, 2, 4, 8):
            f, err, (w, lnc), (alpha, beta, omega, lnc_red) = _tables(nt, J, rng, synth.SIGMA)
            f_d, w_d, iv_d = _lib.dev(f), _lib.dev(w), _lib.dev(1.0 / (err * err))
            a_d, b_d, o_d = (_lib.dev(v) for v in (alpha, beta, omega))
            bufs = torch.empty((J, n), dtype=torch.float64, device="cuda")
            out = torch.empty(n, dtype=torch.float64, device="cuda")

            def white():
                return _lib.chi2_grid_white_mix(f_d, grid, w_d, lnc, out=out.zero_())

            def plain():
                return _lib.chi2_grid_weighted(f_d, iv_d, grid, out=out.zero_())

            def composed():
                for j in range(J):
                    _lib.chi2_grid_weighted(f_d, w_d[j], grid, out=bufs[j].zero_())
                return _lib.softmin_rows(bufs, lnc, out=out.zero_())

            def red():
                return _lib.chi2_grid_ou_mix(f_d, grid, a_d, b_d, o_d, lnc_red, out=out.zero_())

            x = white().clone()
            y = composed().clone()
            plain(), red()
            torch.cuda.synchronize()
            diff = float((x - y).abs().max().cpu())
            runs = (("white", white), ("plain", plain), ("composed", composed), ("red", red))
            times = {name: [] for name, _ in runs}
            for _ in range(ROUNDS):
                for name, fn in runs:
                    times[name].append(timed(fn))
            t = {name: min(v) for name, v in times.items()}
            print("events  %d x %d  J = %d  chi2_white_mix_kernel %.3f ms (%.2f TB/s of %.2f GB)   (a) chi2_rows_kernel<Chi2Plain> "
                  "%.3f ms: white / (a) = %.2f   (b) %d x chi2_rows_kernel + softmin_rows %.3f ms: (b) / white = %.2f   "
                  "(c) ou_mix_kernel at tau = 1e-6 %.3f ms: (c) / white = %.2f   (best of %d, taking turns; white %s ms; "
                  "(a) %s ms; (b) %s ms; (c) %s ms; max |white - (b)| %.2g)"
                  % (n, nt, J, t["white"] * 1e3, one_pass / t["white"] / 1e12, one_pass / 1e9, t["plain"] * 1e3,
                     t["white"] / t["plain"], J, t["composed"] * 1e3, t["composed"] / t["white"], t["red"] * 1e3,
                     t["red"] / t["white"], ROUNDS, *(" ".join("%.3f" % (v * 1e3) for v in times[name]) for name, _ in runs),
                     diff), flush=True)
        del grid


def e2e():
    """wall clock of whole calls, each ended by a device synchronise: one warm-up of either case, then ROUNDS rounds in which
    they take turns"""
    import numpy as np
    import pandas as pd
    import torch
    from helpers import GOLD, gold
    import triceratops_amd as ta
    from triceratops_amd.lightcurve import white_noise_grid
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
    eight = [two[0], dict(two[1], white_grid=white_noise_grid([1.0, 1.5, 2.0, 3.0], [0.0, 0.5 * s]))]
    runs = [("2 datasets of 50 points, no key", lambda: tg.calc_probs_datasets(two, P, **kw)),
            ("2 datasets of 50 points, eight candidates on the second", lambda: tg.calc_probs_datasets(eight, P, **kw))]

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
    print("e2e     posterior weights of the eight candidates at the most probable scenario's best draw: %s"
          % np.array2string(tg.dataset_white_noise[int(np.nanargmax(tg.lnZ))][1]["weight"], precision=3), flush=True)


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
        out.write("# profiles/white_mix/measure.py on one MI355X: a 512 MiB grid per kernel case, device events, best of %d runs, "
                  "the variants taking turns; wall clock of whole calls end to end\n" % ROUNDS)
        out.flush()
        ok = _step(out, 240, [sys.executable, me, "kernels"])
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
