"""Measurements of calc_probs_datasets_refined and trxw_hist_from_halfchi2 (DESIGN.md sections 12 and 14).

  python profiles/warp/measure_datasets.py         the whole job: each GPU step a child process under its own time limit,
                                                   the next one only after the last ended well; APPENDS to
                                                   profiles/warp/results.txt (or --out FILE)
  python profiles/warp/measure_datasets.py e2e     TOI-465.01, 75 scenarios, two cadences (50 points with per-point errors,
                                                   21 points at the FFI cadence), N = 1e6: calc_probs_datasets_refined
                                                   (n_adapt=2) against three calc_probs_datasets passes, taking turns
  python profiles/warp/measure_datasets.py hist    the export on 1e5 and 1e6 synthetic rows, six calls each, timed with
                                                   events; the job runs it under rocprofv3 --kernel-trace --stats and
                                                   quotes the kernels' own times from the trace

warp_hist_kernel is the kernel the library's own chain launches per call (warp_hist_chain_kernel: the same body per
branch of a chain); the export runs it behind post_max_kernel and post_x_kernel, which find the largest log-weight, and a
3.6 KB memset."""
import csv
import glob
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "profiles", "datasets"))
ROUNDS = 7
HIST_ROWS = (100_000, 1_000_000)
HIST_CALLS = 6


def _two_cadences(t, f, sigma):
    """tests/test_gpu_datasets.py::_two_cadences"""
    import numpy as np
    ia, ib = np.arange(0, 100, 2), np.arange(2, 100, 4)[:21]
    a = {"time": t[ia], "flux": f[ia], "flux_err": sigma * np.linspace(0.6, 1.8, 50), "exptime": 0.00139, "nsamples": 20}
    b = {"time": t[ib], "flux": f[ib], "flux_err": 1.4 * sigma, "exptime": 0.0208, "nsamples": 5}
    return [a, b]


def e2e():
    """wall clock of whole calls, each ended by a device synchronise: one warm-up of both, then ROUNDS rounds in which the
    two take turns"""
    import numpy as np
    import torch
    from measure import _toi465
    tg, (t, f, s, P), kw, _ = _toi465()
    data = _two_cadences(t, f, s)

    def timed(fn):
        torch.manual_seed(1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0

    for ev in ("grid", "fused"):
        runs = [("3 x calc_probs_datasets, %s" % ev, lambda: [tg.calc_probs_datasets(data, P, evaluation=ev, **kw) for _ in range(3)]),
                ("calc_probs_datasets_refined(n_adapt=2), %s" % ev,
                 lambda: tg.calc_probs_datasets_refined(data, P, n_adapt=2, evaluation=ev, **kw))]
        times = {name: [] for name, _ in runs}
        for name, fn in runs:
            timed(fn)
        for _ in range(ROUNDS):
            for name, fn in runs:
                times[name].append(timed(fn))
        med = {}
        for name, _ in runs:
            v = np.sort(times[name])
            med[name] = np.median(v)
            print("e2e     %-52s median %.4f s  min %.4f s  max %.4f s  (%d rounds, TOI-465.01, 75 scenarios, two cadences, N = 1e6)"
                  % (name, med[name], v[0], v[-1], v.size), flush=True)
        print("e2e     refined / three plain passes, %s: %.2f" % (ev, med[runs[1][0]] / med[runs[0][0]]), flush=True)
    fin = np.isfinite(tg.lnZ)
    print("e2e     last refined call: ess per pass, median over the %d finite rows: %s"
          % (fin.sum(), ", ".join("%.0f" % np.median(h["ess"][fin]) for h in tg.refine_history)), flush=True)


def hist():
    import numpy as np
    import torch
    from triceratops_amd import _lib, fused
    a = fused.DrawArgs()
    a.N, a.use_philox, a.planet, a.seed = 10_000_000, 1, 1, 12345          # a planet call: slots R_p, inc, ecc, argp
    rng = np.random.default_rng(7)
    for n in HIST_ROWS:
        h = _lib.dev(rng.uniform(0.0, 60.0, n))
        lp = _lib.dev(rng.normal(0.0, 2.0, n))
        idx = torch.from_numpy(np.sort(rng.choice(a.N, size=n, replace=False))).cuda()
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(HIST_CALLS + 1)]
        ev[0].record()
        for k in range(HIST_CALLS):
            out = _lib.warp_hist_from_halfchi2(a, h, lp, idx, -7.0)
            ev[k + 1].record()
        torch.cuda.synchronize()
        dt = [ev[k].elapsed_time(ev[k + 1]) * 1e3 for k in range(1, HIST_CALLS)]
        words = out.cpu().numpy()
        print("events  trxw_hist_from_halfchi2  n = %8d  %.1f us per call, launch gaps included (%d calls after a warm-up; "
              "%d rows with weight)" % (n, sum(dt) / len(dt), len(dt), int(words[1])), flush=True)


def hist_summary(trace):
    """the kernels' own times from the trace: HIST_CALLS launches of each per row count, the first left out"""
    lines = []
    for f in glob.glob(os.path.join(trace, "**", "*kernel_trace.csv"), recursive=True):
        groups = {}
        for row in csv.DictReader(open(f)):
            name = row["Kernel_Name"].replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "")
            if any(k in name for k in ("warp_hist_kernel", "post_max_kernel", "post_x_kernel")):
                groups.setdefault(name, []).append(int(row["End_Timestamp"]) - int(row["Start_Timestamp"]))
        for i, n in enumerate(HIST_ROWS):
            total = 0.0
            for name, ns in sorted(groups.items()):
                part = ns[i * HIST_CALLS:(i + 1) * HIST_CALLS][1:]
                if part:
                    avg = sum(part) / len(part) * 1e-3
                    total += avg
                    lines.append("rocprofv3 %-28s n = %8d  %d launches  %7.2f us each\n" % (name[-28:], n, len(part), avg))
            lines.append("rocprofv3 %-28s n = %8d  %7.2f us of kernels per call\n" % ("the export", n, total))
    return "".join(lines)


def _step(out, limit, cmd):
    print("+ " + " ".join(cmd), flush=True)
    r = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, cwd=ROOT, capture_output=True, text=True)
    out.write(r.stdout)
    if r.returncode != 0:
        out.write("step failed with status %d: %s\n%s\n" % (r.returncode, " ".join(cmd), r.stderr[-2000:]))
    out.flush()
    return r.returncode == 0


def job(path):
    me, base = os.path.abspath(__file__), os.path.dirname(path) or "."
    trace = os.path.join(base, "rocprof_warp_hist")
    with open(path, "a") as out:
        out.write("\n== calc_probs_datasets_refined and trxw_hist_from_halfchi2 (profiles/warp/measure_datasets.py, 1 x MI355X) ==\n")
        ok = _step(out, 420, [sys.executable, me, "e2e"])
        ok = ok and _step(out, 300, ["rocprofv3", "--kernel-trace", "--stats", "-d", trace, "-o", "hist", "--output-format", "csv",
                                     "--", sys.executable, me, "hist"])
        if ok:
            out.write(hist_summary(trace))
        out.write("job %s\n" % ("complete" if ok else "ended early"))
    return 0 if ok else 1


if __name__ == "__main__":
    if sys.argv[1:2] == ["e2e"]:
        e2e()
    elif sys.argv[1:2] == ["hist"]:
        hist()
    else:
        dest = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(os.path.dirname(os.path.abspath(__file__)), "results.txt")
        sys.exit(job(dest))
