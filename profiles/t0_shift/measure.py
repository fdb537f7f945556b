"""Measurements of DESIGN.md section 14, a transit-time shift marginalised per dataset (`t0_grid`, softmin_rows_kernel).

  python profiles/t0_shift/measure.py            the whole job: each GPU step a child process under its own time limit, the
                                                 next one only after the last ended well; writes profiles/t0_shift/results.txt
                                                 (or --out FILE)
  python profiles/t0_shift/measure.py kernels    (a) softmin_rows_kernel (_lib.softmin_rows) against its alternative,
                                                 -torch.logsumexp(lnc[:, None] - cand, dim=0), on the same [J][1e6] buffer,
                                                 J = 2, 4, 8.  One warm-up of each, then five rounds in which the two take
                                                 turns, each run timed with device events; the best of the five and the bytes
                                                 it has to move (J reads, and `out` read and written, per row) over that time.  In the same
                                                 job lme_partial_kernel (_lib.log_mean_exp) over the same J x 1e6 doubles: a
                                                 pass that only streams, the floor for this one
  python profiles/t0_shift/measure.py e2e        (b) TOI-465.01, N = 1e6, two datasets of 50 points: calc_probs_datasets with
                                                 no key, with a five-node grid on the second dataset, on the first dataset alone
                                                 (what is left when the second's share is taken away), with the second dataset's
                                                 stamps moved and no key, and with one node of weight 1; wall clock of whole calls,
                                                 taking turns
"""
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
ROWS = 1_000_000
ROUNDS = 5


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

    for J in (2, 4, 8):
        cand = (50.0 + 3.0 * torch.randn((J, ROWS), dtype=torch.float64, device="cuda")).abs()
        w = rng.uniform(0.1, 1.0, J)
        lnc = np.log(w / w.sum())
        lnc_d = _lib.dev(lnc)
        out = torch.zeros(ROWS, dtype=torch.float64, device="cuda")
        flat = (-cand).reshape(-1).contiguous()
        moved = (J + 2) * ROWS * 8                      # (J reads, and out read and written: the path accumulates)

        def softmin():
            return _lib.softmin_rows(cand, lnc, out=out)

        def composed():
            return -torch.logsumexp(lnc_d[:, None] - cand, dim=0)

        def lme():
            return _lib.log_mean_exp(flat, flat.numel())

        x, y = _lib.softmin_rows(cand, lnc), composed()
        softmin()
        lme()
        torch.cuda.synchronize()
        diff = float((x - y).abs().max().cpu())
        times = {"softmin": [], "composed": [], "lme": []}
        for _ in range(ROUNDS):
            for name, fn in (("softmin", softmin), ("composed", composed), ("lme", lme)):
                times[name].append(timed(fn))
        ts, tc, tl = (min(times[k]) for k in ("softmin", "composed", "lme"))
        print("events  %d rows  J = %d  softmin_rows_kernel %.4f ms (%.2f TB/s of %.1f MB)   torch.logsumexp %.4f ms   "
              "logsumexp / softmin = %.2f   lme_partial_kernel + final over the same %d doubles %.4f ms (%.2f TB/s of %.1f MB)   "
              "(best of %d, taking turns; softmin %s ms; logsumexp %s ms; lme %s ms; max |difference| of the two results %.2g)"
              % (ROWS, J, ts * 1e3, moved / ts / 1e12, moved / 1e6, tc * 1e3, tc / ts, J * ROWS, tl * 1e3,
                 J * ROWS * 8 / tl / 1e12, J * ROWS * 8 / 1e6, ROUNDS, " ".join("%.4f" % (t * 1e3) for t in times["softmin"]),
                 " ".join("%.4f" % (t * 1e3) for t in times["composed"]), " ".join("%.4f" % (t * 1e3) for t in times["lme"]),
                 diff), flush=True)


def e2e():
    """wall clock of whole calls, each ended by a device synchronise: one warm-up of every case, then ROUNDS rounds in which
    they take turns"""
    import numpy as np
    import pandas as pd
    import torch
    from helpers import GOLD, gold
    import triceratops_amd as ta
    from triceratops_amd.lightcurve import t0_shift_grid
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
    five = [two[0], dict(two[1], t0_grid=t0_shift_grid(cadence, n=5, span=3.0))]
    moved = [two[0], dict(two[1], time=two[1]["time"] + 1.5 * cadence)]
    one = [two[0], dict(two[1], t0_grid=[(1.5 * cadence, 1.0)])]
    names = ("2 datasets of 50 points, no key", "2 datasets of 50 points, five nodes on the second", "the first dataset alone",
             "no key, the second on time + 1.5 cadences", "one node (1.5 cadences, 1) on the second")
    runs = [(names[0], lambda: tg.calc_probs_datasets(two, P, **kw)),
            (names[1], lambda: tg.calc_probs_datasets(five, P, **kw)),
            (names[2], lambda: tg.calc_probs_datasets(two[:1], P, **kw)),
            (names[3], lambda: tg.calc_probs_datasets(moved, P, **kw)),
            (names[4], lambda: tg.calc_probs_datasets(one, P, **kw))]

    def timed_pass(fn):
        torch.manual_seed(1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    times, fpp, t0 = {name: [] for name, _ in runs}, {}, None
    for name, fn in runs:
        timed_pass(fn)
    for _ in range(ROUNDS):
        for name, fn in runs:
            times[name].append(timed_pass(fn))
            fpp[name] = tg.FPP
            if name == names[1]:
                t0 = tg.dataset_t0[int(np.nanargmax(tg.lnZ))][1]
    med = {}
    for name, _ in runs:
        v = np.sort(times[name])
        med[name] = float(np.median(v))
        print("e2e     %-52s median %.4f s  min %.4f s  max %.4f s  (%d rounds, FPP %.6g)"
              % (name, med[name], v[0], v[-1], v.size, fpp[name]), flush=True)
    share = med[names[0]] - med[names[2]]
    extra = med[names[1]] - med[names[0]]
    print("e2e     the second dataset's share (two datasets less the first alone) %.4f s; five nodes cost %.4f s more than none: "
          "%.2f shares (expected: about 4)" % (share, extra, extra / share if share > 0 else float("nan")), flush=True)
    print("e2e     the same stamps moved by 1.5 cadences, no key: %.4f s more than unmoved (what a node's stamps cost beyond the "
          "dataset's own); one node of weight 1 in place of the moved stamps: %.4f s more (the zeroed buffer, the soft minimum "
          "and the best draw's second evaluation)" % (med[names[3]] - med[names[0]], med[names[4]] - med[names[3]]), flush=True)
    print("e2e     posterior weights of the five nodes at the most probable scenario's best draw: %s, mean shift %.3g cadences"
          % (np.array2string(t0["weight"], precision=3), t0["mean"] / cadence), flush=True)


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
        out.write("# profiles/t0_shift/measure.py on one MI355X: 1e6 rows per kernel case, device events, best of %d runs, the "
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
