"""Measurements of DESIGN.md section 14 (several light curves, per-point errors).

  python profiles/datasets/measure.py            the whole job: each GPU step a child process under its own time
                                                 limit, the next one only after the last ended well; writes
                                                 profiles/datasets/results.txt (or --out FILE)
  python profiles/datasets/measure.py kernels    (a) the weighted reduction and chi2_grid_kernel on the same 3.2 GB
                                                 grid (200 000 rows x 2000 stamps, bench.py's size), timed with events
  python profiles/datasets/measure.py e2e        (b) TOI-465.01, 75 scenarios, N = 1e6: calc_probs against
                                                 calc_probs_datasets with one and with two datasets, each with
                                                 evaluation="grid" and evaluation="fused", alternating
  python profiles/datasets/measure.py routes     (c) the two calc_probs_datasets cases alone, both evaluations, three
                                                 passes each: the run the job traces for the kernel times of a pass
  python profiles/datasets/measure.py rates      (d) chi2_rows_kernel with Chi2Plain, Chi2Offset and Chi2Baseline<K>
                                                 at K = 1 and 4 (labelled as in earlier results: chi2_grid_weighted_kernel,
                                                 _offset_, _baseline_) on the same 200 000 x 2000 grid
                                                 and at 1e6 x 100: the run the job traces for the kernels' rates
  python profiles/datasets/measure.py baseline_e2e   (e) two datasets of 50 points, N = 1e6: calc_probs_datasets with and
                                                 without polynomial_baseline(t, 1) + a flat offset on the second dataset
  python profiles/datasets/measure.py ou_kernels     (f) chi2_ou_kernel (correlated noise) next to the plain weighted reduction
                                                 on the same grids, 200 000 x 2000 and 1e6 x 100: the run the job's step
                                                 `ou_rates` traces
  python profiles/datasets/measure.py ou_e2e     (g) two datasets of 50 points, N = 1e6: calc_probs_datasets with and without
                                                 red_sigma / red_timescale on the second dataset (the other half of `ou_rates`)

The job runs `kernels` twice: plainly, and under `rocprofv3 --kernel-trace --stats`, whose kernel trace gives the
per-launch times quoted (the event timings include the launch gaps of five back-to-back calls); `routes` runs under
the tracer only, in a run of its own, and so does `rates`.  --only e2e,routes: those steps of the job alone, APPENDED to
the results file.
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


def _toi465():
    import numpy as np
    import pandas as pd
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
    return tg, (t, f, s, P), kw, (("1 dataset of 100 points", one), ("2 datasets of 50 points", two))


def _timed_pass(fn):
    import torch
    torch.manual_seed(1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


E2E_ROUNDS = 7


def e2e():
    """wall clock of whole calls, each ended by a device synchronise: one warm-up of every case (caches, scratch, code
    objects), then E2E_ROUNDS rounds in which the cases take turns -- grid and fused next to each other --; the median
    and the smallest of a case's rounds"""
    import numpy as np
    import torch
    tg, (t, f, s, P), kw, cases = _toi465()
    runs = [("calc_probs", lambda: tg.calc_probs(t, f, s, P, **kw))]
    for label, ds in cases:
        for ev in ("grid", "fused"):
            runs.append(("calc_probs_datasets, %s, %s" % (label, ev),
                         lambda ds=ds, ev=ev: tg.calc_probs_datasets(ds, P, evaluation=ev, **kw)))
    times, fpp, peak = {name: [] for name, _ in runs}, {}, {}
    for name, fn in runs:
        _timed_pass(fn)
    for rnd in range(E2E_ROUNDS):
        for name, fn in runs:
            torch.cuda.reset_peak_memory_stats()
            times[name].append(_timed_pass(fn))
            fpp[name], peak[name] = tg.FPP, torch.cuda.max_memory_allocated()
    for name, _ in runs:
        v = np.sort(times[name])
        print("e2e     %-52s median %.4f s  min %.4f s  max %.4f s  (%d rounds, %d scenarios, FPP %.6g, allocator peak %.0f MiB)"
              % (name, np.median(v), v[0], v[-1], v.size, tg.lnZ.size, fpp[name], peak[name] / 2 ** 20), flush=True)
    for label, _ in cases:
        g, h = (np.median(times["calc_probs_datasets, %s, %s" % (label, ev)]) for ev in ("grid", "fused"))
        print("e2e     %-52s grid / fused = %.2f  (medians; calc_probs = 1: grid %.1f, fused %.1f)"
              % (label, g / h, g / np.median(times["calc_probs"]), h / np.median(times["calc_probs"])), flush=True)


def rates():
    """six launches of every reduction of a dataset's term on both shapes (the first is the warm-up); the job's tracer
    gives the per-launch times, the events here include the launch gaps"""
    import numpy as np
    import torch
    from triceratops_amd import _lib, synth
    from triceratops_amd.datasets import linear_system
    rng = np.random.default_rng(synth.SEED)
    for n, nt in ((N_GRID, N_TIME), (1_000_000, 100)):
        f = 1.0 + rng.normal(0.0, synth.SIGMA, nt)
        w = 1.0 / (rng.uniform(0.5, 2.0, nt) * synth.SIGMA) ** 2
        f_d, w_d = _lib.dev(f), _lib.dev(w)
        grid = torch.rand((n, nt), dtype=torch.float64, device="cuda")
        u = np.linspace(-1.0, 1.0, nt)
        cases = [("chi2_grid_weighted_kernel", lambda: _lib.chi2_grid_weighted(f_d, w_d, grid)),
                 ("chi2_grid_offset_kernel", lambda: _lib.chi2_grid_offset(f_d, w_d, grid, float(np.sum(w)), 0.0))]
        for K in (1, 4):
            system = linear_system(w, np.stack([u ** p for p in range(K)]), np.inf)
            g_d, minv = _lib.dev(system.g), system.minv
            cases.append(("chi2_grid_baseline_kernel K = %d" % K,
                          lambda g_d=g_d, minv=minv: _lib.chi2_grid_baseline(f_d, w_d, grid, g_d, minv)))
        gb = (n * nt * 8 + n * 8) / 1e9
        for name, fn in cases:
            fn()
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(5):
                fn()
            b.record()
            torch.cuda.synchronize()
            dt = a.elapsed_time(b) * 1e-3 / 5
            print("events  %-36s %d x %d  %.3f ms  %.2f TB/s  (%.2f GB)" % (name, n, nt, dt * 1e3, gb / dt / 1e3, gb), flush=True)
        del grid


def rates_summary(trace):
    """per-launch times of the `rates` step from rocprofv3's kernel trace, by kernel and launch shape, each one's first
    (warm-up) launch left out"""
    lines = []
    for f in glob.glob(os.path.join(trace, "**", "*kernel_trace.csv"), recursive=True):
        groups = {}
        for row in csv.DictReader(open(f)):
            name = row["Kernel_Name"].replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "")
            if "chi2_rows_kernel" in name:
                groups.setdefault(name, []).append(int(row["End_Timestamp"]) - int(row["Start_Timestamp"]))
        for name, ns in groups.items():
            # (per kernel: six launches on the large grid, then -- the staged instantiations only fit there -- six on 1e6 x 100)
            for part, (rows, nt) in zip((ns[i:i + 6] for i in range(0, len(ns), 6)),
                                        ((N_GRID, N_TIME), (1_000_000, 100)) if len(ns) > 6 else
                                        (((N_GRID, N_TIME),) if "<false" in name else ((1_000_000, 100),))):
                avg = sum(part[1:]) / max(len(part) - 1, 1)
                gb = (rows * nt * 8 + rows * 8) / 1e9
                lines.append("rocprofv3 %-44s %d x %d  %d launches  %.1f us  %.2f TB/s  (%.2f GB)\n"
                             % (name[:44], rows, nt, len(part) - 1, avg * 1e-3, gb / (avg * 1e-9) / 1e3, gb))
    return "".join(lines)


def baseline_e2e():
    """wall clock of calc_probs_datasets on two datasets of 50 points with and without a slope column and a flat offset on
    the second: one warm-up each, then E2E_ROUNDS rounds in which the two take turns"""
    import numpy as np
    from triceratops_amd.lightcurve import polynomial_baseline
    tg, (t, f, s, P), kw, cases = _toi465()
    two = cases[1][1]
    with_b = [two[0], dict(two[1], offset_sigma=float("inf"), baseline=polynomial_baseline(two[1]["time"], 1))]
    runs = [("2 datasets of 50 points", lambda: tg.calc_probs_datasets(two, P, **kw)),
            ("2 datasets of 50 points, slope + flat offset on the second", lambda: tg.calc_probs_datasets(with_b, P, **kw))]
    times = {name: [] for name, _ in runs}
    for name, fn in runs:
        _timed_pass(fn)
    for _ in range(E2E_ROUNDS):
        for name, fn in runs:
            times[name].append(_timed_pass(fn))
    for name, _ in runs:
        v = np.sort(times[name])
        print("e2e     %-60s median %.4f s  min %.4f s  max %.4f s  (%d rounds)" % (name, np.median(v), v[0], v[-1], v.size), flush=True)


OU_PARAMS = (3.0, 10.0)          # s_r in units of the mean error, tau in cadences


def _ou_tables(nt, rng, sigma):
    """(flux, white weights, (alpha, beta, omega)) of a light curve of nt stamps at unit cadence"""
    import numpy as np
    from triceratops_amd.datasets import ou_system, validate
    err = rng.uniform(0.5, 2.0, nt) * sigma
    d = validate([{"time": np.arange(nt, dtype=np.float64), "flux": np.ones(nt), "flux_err": err,
                   "red_sigma": OU_PARAMS[0] * sigma, "red_timescale": OU_PARAMS[1]}])[0]
    return 1.0 + rng.normal(0.0, sigma, nt), 1.0 / err ** 2, ou_system(d)


def ou_kernels():
    """six launches of the plain weighted reduction and of chi2_ou_kernel on the same grids, both shapes (the first is
    the warm-up); the job's tracer gives the per-launch times, the events here include the launch gaps"""
    import numpy as np
    import torch
    from triceratops_amd import _lib, synth
    rng = np.random.default_rng(synth.SEED)
    for n, nt in ((N_GRID, N_TIME), (1_000_000, 100)):
        f, w, abw = _ou_tables(nt, rng, synth.SIGMA)
        f_d, w_d, abw_d = _lib.dev(f), _lib.dev(w), tuple(_lib.dev(v) for v in abw)
        grid = torch.rand((n, nt), dtype=torch.float64, device="cuda")
        gb = (n * nt * 8 + n * 8) / 1e9
        for name, fn in (("chi2_grid_weighted_kernel", lambda: _lib.chi2_grid_weighted(f_d, w_d, grid)),
                         ("chi2_ou_kernel", lambda: _lib.chi2_grid_ou(f_d, grid, *abw_d))):
            fn()
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(5):
                fn()
            b.record()
            torch.cuda.synchronize()
            dt = a.elapsed_time(b) * 1e-3 / 5
            print("events  %-36s %d x %d  %.3f ms  %.2f TB/s  (%.2f GB)" % (name, n, nt, dt * 1e3, gb / dt / 1e3, gb), flush=True)
        del grid


def ou_summary(trace):
    """per-launch times of the `ou_kernels` step from rocprofv3's kernel trace, by kernel, each shape's first (warm-up)
    launch left out, and the ratio of scan_rows_kernel<ONE, OuFilter> to the plain reduction on the same grid"""
    lines, avg = [], {}
    for f in glob.glob(os.path.join(trace, "**", "*kernel_trace.csv"), recursive=True):
        groups = {}
        for row in csv.DictReader(open(f)):
            name = row["Kernel_Name"].replace("(anonymous namespace)::", "").split("(")[0].replace("void ", "")
            if "chi2_rows_kernel" in name or "OuFilter>" in name:
                groups.setdefault(name, []).append(int(row["End_Timestamp"]) - int(row["Start_Timestamp"]))
        for name, ns in groups.items():
            # (the staged plain reduction runs on both shapes, six launches each, the large grid first; the OU filter's <false>
            # on the large grid only, <true> -- one trip -- at 100 stamps only)
            shapes = ((N_GRID, N_TIME), (1_000_000, 100))
            if "OuFilter>" in name:
                shapes = shapes[1:] if "<true" in name else shapes[:1]
            for part, (rows, nt) in zip((ns[i:i + 6] for i in range(0, len(ns), 6)), shapes):
                avg[("ou" if "OuFilter>" in name else "plain", nt)] = a = sum(part[1:]) / max(len(part) - 1, 1)
                gb = (rows * nt * 8 + rows * 8) / 1e9
                lines.append("rocprofv3 %-44s %d x %d  %d launches  %.1f us  %.2f TB/s  (%.2f GB)\n"
                             % (name[:44], rows, nt, len(part) - 1, a * 1e-3, gb / (a * 1e-9) / 1e3, gb))
    for nt in (N_TIME, 100):
        if ("ou", nt) in avg and ("plain", nt) in avg:
            lines.append("rocprofv3 scan_rows_kernel<OuFilter> / chi2_rows_kernel<Chi2Plain> at %d stamps: %.2f\n"
                         % (nt, avg[("ou", nt)] / avg[("plain", nt)]))
    return "".join(lines)


def ou_e2e():
    """wall clock of calc_probs_datasets on two datasets of 50 points with and without red_sigma / red_timescale on the
    second: one warm-up each, then E2E_ROUNDS rounds in which the two take turns"""
    import numpy as np
    tg, (t, f, s, P), kw, cases = _toi465()
    two = cases[1][1]
    cadence = float(np.median(np.diff(two[1]["time"])))
    with_r = [two[0], dict(two[1], red_sigma=OU_PARAMS[0] * s, red_timescale=OU_PARAMS[1] * cadence)]
    runs = [("2 datasets of 50 points", lambda: tg.calc_probs_datasets(two, P, **kw)),
            ("2 datasets of 50 points, red noise on the second", lambda: tg.calc_probs_datasets(with_r, P, **kw))]
    times, fpp = {name: [] for name, _ in runs}, {}
    for name, fn in runs:
        _timed_pass(fn)
    for _ in range(E2E_ROUNDS):
        for name, fn in runs:
            times[name].append(_timed_pass(fn))
            fpp[name] = tg.FPP
    for name, _ in runs:
        v = np.sort(times[name])
        print("e2e     %-60s median %.4f s  min %.4f s  max %.4f s  (%d rounds, FPP %.6g)"
              % (name, np.median(v), v[0], v[-1], v.size, fpp[name]), flush=True)


ROUTE_PASSES = 3


def routes():
    """the run the job traces: every calc_probs_datasets case with both evaluations, ROUTE_PASSES passes each"""
    tg, (t, f, s, P), kw, cases = _toi465()
    for label, ds in cases:
        for ev in ("grid", "fused"):
            for _ in range(ROUTE_PASSES):
                dt = _timed_pass(lambda: tg.calc_probs_datasets(ds, P, evaluation=ev, **kw))
            print("routes  %-52s %.4f s under the tracer (last of %d passes)" % ("%s, %s" % (label, ev), dt, ROUTE_PASSES), flush=True)


def routes_summary(trace):
    """kernel time of the `routes` step by kernel, from rocprofv3's kernel trace: the likelihood kernels are told apart
    by their template arguments (cells_kernel<1, ...> writes the grid, a last argument `true` is the weighted fused
    variant), everything else is shared by the two evaluations"""
    def route(name):
        if "chi2_rows_kernel" in name or "cells_kernel<1" in name or "sec_scan_kernel<64" in name:
            return "grid"
        for k in ("cells_kernel<0", "rowc_kernel<", "sec_scan_kernel<8"):
            if k in name:
                return "fused" if name.split(">(")[0].rstrip().endswith("true") else "grid"
        return "both"
    lines = []
    for f in glob.glob(os.path.join(trace, "**", "*kernel_trace.csv"), recursive=True):
        groups = {}
        for row in csv.DictReader(open(f)):
            g = groups.setdefault(row["Kernel_Name"], [0, 0])
            g[0] += 1
            g[1] += int(row["End_Timestamp"]) - int(row["Start_Timestamp"])
        passes = 2 * ROUTE_PASSES              # passes of one evaluation: two cases
        total = {"grid": 0, "fused": 0, "both": 0}
        for name, (calls, ns) in sorted(groups.items(), key=lambda kv: -kv[1][1]):
            total[route(name)] += ns
            short = name.replace("(anonymous namespace)::", "").split("(")[0]
            if ns > 0.002 * sum(v[1] for v in groups.values()):
                lines.append("rocprofv3 %-5s %-72s %6d launches  %9.1f us in all  %7.2f us each\n"
                             % (route(name), short[:72], calls, ns * 1e-3, ns * 1e-3 / calls))
        lines.append("rocprofv3 kernel time per calc_probs_datasets pass (mean of the two cases): grid-only kernels %.2f ms, "
                     "fused-only kernels %.2f ms, kernels of both evaluations %.2f ms per pass of either\n"
                     % (total["grid"] * 1e-6 / passes, total["fused"] * 1e-6 / passes, total["both"] * 1e-6 / (2 * passes)))
    return "".join(lines)


def trace_summary(trace):
    """per-launch kernel times of the `kernels` step from rocprofv3's kernel trace, by launch shape, each shape's first
    (warm-up) launch left out -- the --stats averages would mix the shapes"""
    lines = []
    for f in glob.glob(os.path.join(trace, "**", "*kernel_trace.csv"), recursive=True):
        groups = {}
        for row in csv.DictReader(open(f)):
            if "chi2_grid_kernel" in row["Kernel_Name"] or "chi2_rows_kernel" in row["Kernel_Name"]:
                # (the weighted reduction keeps its label of earlier results: chi2_rows_kernel<STAGE, Chi2Plain>)
                name = "chi2_grid_weighted_kernel" if "chi2_rows_kernel" in row["Kernel_Name"] else "chi2_grid_kernel"
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


def job(path, only=None):
    me, base = os.path.abspath(__file__), os.path.dirname(path) or "."
    trace, trace2 = os.path.join(base, "rocprof_datasets"), os.path.join(base, "rocprof_datasets_routes")
    want = (lambda step: only is None or step in only)
    with open(path, "a" if only else "w") as out:
        if only:
            out.write("# profiles/datasets/measure.py --only %s on one MI355X: wall clock of whole calls (one warm-up, then %d "
                      "rounds, the cases taking turns); kernel times from the trace of a run of its own (rocprofv3 "
                      "--kernel-trace --stats)\n" % (",".join(only), E2E_ROUNDS))
        else:
            out.write("# profiles/datasets/measure.py on one MI355X; %.2f GB per chi2 launch\n" % GB)
        ok = True
        if want("kernels"):
            ok = _step(out, 240, [sys.executable, me, "kernels"])
            ok = ok and _step(out, 300, ["rocprofv3", "--kernel-trace", "--stats", "-d", trace, "-o", "chi2", "--output-format",
                                         "csv", "--", sys.executable, me, "kernels"])
            if ok:
                out.write(trace_summary(trace))
        if want("e2e"):
            ok = ok and _step(out, 420, [sys.executable, me, "e2e"])
        if want("routes"):
            ok = ok and _step(out, 420, ["rocprofv3", "--kernel-trace", "--stats", "-d", trace2, "-o", "routes", "--output-format",
                                         "csv", "--", sys.executable, me, "routes"])
            if ok:
                out.write(routes_summary(trace2))
        if want("rates"):
            trace3 = os.path.join(base, "rocprof_datasets_rates")
            ok = ok and _step(out, 300, ["rocprofv3", "--kernel-trace", "--stats", "-d", trace3, "-o", "rates", "--output-format",
                                         "csv", "--", sys.executable, me, "rates"])
            if ok:
                out.write(rates_summary(trace3))
        if want("baseline_e2e"):
            ok = ok and _step(out, 420, [sys.executable, me, "baseline_e2e"])
        if want("ou_rates"):
            trace4 = os.path.join(base, "rocprof_datasets_ou")
            ok = ok and _step(out, 300, ["rocprofv3", "--kernel-trace", "--stats", "-d", trace4, "-o", "ou", "--output-format",
                                         "csv", "--", sys.executable, me, "ou_kernels"])
            if ok:
                out.write(ou_summary(trace4))
            ok = ok and _step(out, 420, [sys.executable, me, "ou_e2e"])
        out.write("job %s\n" % ("complete" if ok else "ended early"))
    return 0 if ok else 1


if __name__ == "__main__":
    if sys.argv[1:2] == ["kernels"]:
        kernels()
    elif sys.argv[1:2] == ["e2e"]:
        e2e()
    elif sys.argv[1:2] == ["routes"]:
        routes()
    elif sys.argv[1:2] == ["rates"]:
        rates()
    elif sys.argv[1:2] == ["baseline_e2e"]:
        baseline_e2e()
    elif sys.argv[1:2] == ["ou_kernels"]:
        ou_kernels()
    elif sys.argv[1:2] == ["ou_e2e"]:
        ou_e2e()
    else:
        dest = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(os.path.dirname(os.path.abspath(__file__)), "results.txt")
        only = sys.argv[sys.argv.index("--only") + 1].split(",") if "--only" in sys.argv else None
        sys.exit(job(dest, only))
