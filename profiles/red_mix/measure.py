"""Measurements of DESIGN.md section 14, red-noise candidates marginalised per draw (`red_grid`, ou_mix_kernel).

  python profiles/red_mix/measure.py            the whole job: each GPU step a child process under its own time limit, the
                                                next one only after the last ended well; writes profiles/red_mix/results.txt
                                                (or --out FILE)
  python profiles/red_mix/measure.py kernels    (a) ou_mix_kernel (_lib.chi2_grid_ou_mix, one pass over the grid) against its
                                                only alternative, J calls of _lib.chi2_grid_ou into J buffers and one
                                                torch.logsumexp over them, on the same 512 MiB grid: n_time = 100 and 2048,
                                                J = 2, 4, 8.  One warm-up of each, then five rounds in which the two take
                                                turns, each run timed with device events; the best of the five and the bytes
                                                of the grid it has to read (once, or J times) over that time
  python profiles/red_mix/measure.py e2e        (b) TOI-465.01, N = 1e6, two datasets of 50 points: calc_probs_datasets with
                                                one pair (red_sigma / red_timescale) and with a grid of six candidates on the
                                                second dataset, wall clock of whole calls, taking turns
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
SIGMAS, TAUS = (0.5, 1.0, 2.0, 3.0), (3.0, 30.0)          # s_r in units of the mean error, tau in cadences


def _tables(nt, J, rng, sigma):
    import numpy as np
    from triceratops_amd.datasets import ou_mix_system, validate
    from triceratops_amd.lightcurve import red_noise_grid
    err = rng.uniform(0.5, 2.0, nt) * sigma
    grid = red_noise_grid([s * sigma for s in SIGMAS], TAUS)[:J]
    d = validate([{"time": np.arange(nt, dtype=np.float64), "flux": np.ones(nt), "flux_err": err, "red_grid": grid}])[0]
    return 1.0 + rng.normal(0.0, sigma, nt), ou_mix_system(d)


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
            f, (alpha, beta, omega, lnc) = _tables(nt, J, rng, synth.SIGMA)
            f_d, a_d, b_d, w_d = (_lib.dev(v) for v in (f, alpha, beta, omega))
            lnc_d = _lib.dev(lnc)
            bufs = torch.empty((J, n), dtype=torch.float64, device="cuda")
            out = torch.empty(n, dtype=torch.float64, device="cuda")

            def mix():
                _lib.chi2_grid_ou_mix(f_d, grid, a_d, b_d, w_d, lnc, out=out.zero_())
                return out

            def composed():
                for j in range(J):
                    _lib.chi2_grid_ou(f_d, grid, a_d[j], b_d[j], w_d[j], out=bufs[j].zero_())
                return -torch.logsumexp(lnc_d[:, None] - bufs, dim=0)

            x, y = mix().clone(), composed()
            torch.cuda.synchronize()
            diff = float((x - y).abs().max().cpu())
            times = {"mix": [], "composed": []}
            for _ in range(ROUNDS):
                times["mix"].append(timed(mix))
                times["composed"].append(timed(composed))
            tm, tc = min(times["mix"]), min(times["composed"])
            print("events  %d x %d  J = %d  ou_mix_kernel %.3f ms (%.2f TB/s of %.2f GB)   %d x chi2_ou_kernel + logsumexp "
                  "%.3f ms (%.2f TB/s of %.2f GB)   composed / mix = %.2f   (best of %d, taking turns; mix %s ms; composed %s ms;"
                  " max |difference| of the two results %.2g)"
                  % (n, nt, J, tm * 1e3, one_pass / tm / 1e12, one_pass / 1e9, J, tc * 1e3, J * one_pass / tc / 1e12,
                     J * one_pass / 1e9, tc / tm, ROUNDS, " ".join("%.3f" % (t * 1e3) for t in times["mix"]),
                     " ".join("%.3f" % (t * 1e3) for t in times["composed"]), diff), flush=True)
        del grid


def e2e():
    """wall clock of whole calls, each ended by a device synchronise: one warm-up of either case, then ROUNDS rounds in which
    they take turns"""
    import numpy as np
    import pandas as pd
    import torch
    from helpers import GOLD, gold
    import triceratops_amd as ta
    from triceratops_amd.lightcurve import red_noise_grid
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
    pair = [two[0], dict(two[1], red_sigma=3.0 * s, red_timescale=10.0 * cadence)]
    six = [two[0], dict(two[1], red_grid=red_noise_grid([1.0 * s, 3.0 * s], [3.0 * cadence, 10.0 * cadence, 30.0 * cadence]))]
    runs = [("2 datasets of 50 points, one pair on the second", lambda: tg.calc_probs_datasets(pair, P, **kw)),
            ("2 datasets of 50 points, six candidates on the second", lambda: tg.calc_probs_datasets(six, P, **kw))]

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
        print("e2e     %-56s median %.4f s  min %.4f s  max %.4f s  (%d rounds, %d scenarios, FPP %.6g)"
              % (name, np.median(v), v[0], v[-1], v.size, tg.lnZ.size, fpp[name]), flush=True)
    weights = [row[1]["weight"] for row, z in zip(tg.dataset_red_noise, tg.lnZ) if np.isfinite(z)]
    print("e2e     posterior weights of the six candidates at the most probable scenario's best draw: %s"
          % np.array2string(tg.dataset_red_noise[int(np.nanargmax(tg.lnZ))][1]["weight"], precision=3), flush=True)
    assert len(weights) > 0


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
        out.write("# profiles/red_mix/measure.py on one MI355X: a 512 MiB grid per kernel case, device events, best of %d runs, "
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
