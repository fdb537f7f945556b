"""Measurements for "one sweep" (DESIGN 4.1): cells_kernel's one-row instantiations evaluate a contact cell in the chunk
that planned it instead of in a second sweep.

    python profiles/one_sweep/measure.py <stage> <parent libtrx.so> <tree libtrx.so> [<parent -DTRX_CENSUS build>]

Stages (each a job of its own; every GPU step is a child process under its own time limit, and the first failure ends
the stage; nothing here uses more than the 16 threads bench.py takes by default):
  census    the parent's -DTRX_CENSUS build on config 1 (profiles/r05/census_run.py): second-sweep chunks, passes and pair
            trips per row, lanes per trip -- and the same for 2000 irregular stamps
  ab        same-job A/B of the production builds, arms alternating three times: bench.py --full --steps 10 (config 1, the
            2000 irregular stamps that run the changed code too, and the controls: 100 / 200 points, the 64-TOI step)
  counters  rocprofv3 --pmc alone, one pass of the 18 families per build (profiles/r07/cells2000_once.py)
  outputs   bench.py --dump-outputs per build: lnZ_checksum, the largest relative change of halfchi2.npy and lnZ.npy,
            and roofline.model_evaluations_per_cell of bench.py --full's census
Everything is printed; profiles/one_sweep/results.txt is the record of one such run of each stage.
"""
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

R = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PY = sys.executable


def run(cmd, limit, lib, **kw):
    env = dict(os.environ, TRX_LIB=lib)
    p = subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, cwd=R, env=env, stdout=subprocess.PIPE, text=True, **kw)
    if p.returncode != 0:
        print("FAILED (%d): %s" % (p.returncode, " ".join(cmd)))
        print(p.stdout[-2000:])
        sys.exit(1)
    return p.stdout


def last_json(text):
    return json.loads(text.strip().splitlines()[-1])


def census(parent_census):
    for n_time, grid in ((2000, "uniform"), (2000, "irregular")):
        c = last_json(run([PY, "profiles/r05/census_run.py", str(n_time), grid], 240, parent_census))
        rows = c["rows"]
        print("parent census, %d %s points, per row: first-sweep chunks %.3f, second-sweep chunks %.3f, passes %.3f, "
              "pair trips %.3f, lanes per pair trip %.2f" % (n_time, grid, c["chunk0"] / rows, c["chunk1"] / rows,
                                                             c["pass"] / rows, c["pair_trip"] / rows, c["pair_lanes"] / c["pair_trip"]))
        sys.stdout.flush()


def ab(parent, tree):
    rec = {"parent": [], "tree": []}
    for rep in (1, 2, 3):
        for arm, lib in (("parent", parent), ("tree", tree)):
            d = last_json(run([PY, "bench.py", "--gpus", "1", "--full", "--steps", "10", "--warmup", "3", "--no-cpu-baseline",
                               "--no-e2e", "--pmc", "off"], 400, lib))
            sh, b = d.get("shapes") or {}, d.get("batch") or {}
            row = {"cfg1": d["roofline"]["mean_launch_ms"], "value": d["value"], "ms_per_step": d["ms_per_step"],
                   "irregular": (sh.get("n2000_irregular") or {}).get("mean_launch_ms", float("nan")),
                   "n100": (sh.get("n100") or {}).get("mean_launch_ms", float("nan")),
                   "n200": (sh.get("n200") or {}).get("mean_launch_ms", float("nan")),
                   "toi64": b.get("ms_per_step", float("nan")),
                   "evals": d["roofline"].get("model_evaluations_per_cell"), "checksum": d["lnZ_checksum"]}
            rec[arm].append(row)
            print("%-6s rep %d  cfg1 %.4f ms  value %.4e/s  ms_per_step %.3f | irregular %.4f ms | n100 %.4f n200 %.4f | "
                  "64-TOI step %.2f ms | evaluations per cell %s | lnZ_checksum %.15g"
                  % (arm, rep, row["cfg1"], row["value"], row["ms_per_step"], row["irregular"], row["n100"], row["n200"],
                     row["toi64"], row["evals"], row["checksum"]))
            sys.stdout.flush()
    for key in ("cfg1", "ms_per_step", "irregular", "n100", "n200", "toi64"):
        p, t = (np.array([r[key] for r in rec[a]]) for a in ("parent", "tree"))
        spread = max(p.max() - p.min(), t.max() - t.min())
        print("%-11s parent %.4f (spread %.4f)  tree %.4f (spread %.4f)  tree - parent %+.4f = %+.2f %% = %.1f within-arm spreads"
              % (key, p.mean(), p.max() - p.min(), t.mean(), t.max() - t.min(), t.mean() - p.mean(),
                 100.0 * (t.mean() - p.mean()) / p.mean(), (p.mean() - t.mean()) / spread if spread > 0 else float("inf")))


def counters(parent, tree):
    out = tempfile.mkdtemp(prefix="one_sweep_pmc_")
    try:
        for arm, lib in (("parent", parent), ("tree", tree)):
            d = os.path.join(out, "pmc_" + arm)
            run(["rocprofv3", "--pmc", "SQ_INSTS_VALU", "SQ_ACTIVE_INST_VALU", "SQ_BUSY_CYCLES", "SQ_WAVE_CYCLES",
                 "--output-format", "csv", "-d", d, "--", PY, "profiles/r07/cells2000_once.py"], 240, lib, stderr=subprocess.STDOUT)
            text = run([PY, "profiles/pmc_summary.py", d], 120, lib, stderr=subprocess.STDOUT)
            print("== counters, %s" % arm)
            lines = text.splitlines()
            for i, line in enumerate(lines):
                if "cells_kernel" in line and "<0" in line.replace(" ", ""):
                    print("\n".join(lines[i:i + 5]))
            sys.stdout.flush()
    finally:
        shutil.rmtree(out, ignore_errors=True)


def outputs(parent, tree):
    out = tempfile.mkdtemp(prefix="one_sweep_dump_")
    try:
        ck = {}
        for arm, lib in (("parent", parent), ("tree", tree)):
            d = last_json(run([PY, "bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1", "--no-cpu-baseline",
                               "--dump-outputs", os.path.join(out, arm)], 300, lib))
            ck[arm] = d["lnZ_checksum"]
        print("lnZ_checksum parent %.17g tree %.17g equal: %s" % (ck["parent"], ck["tree"], ck["parent"] == ck["tree"]))
        for name in ("halfchi2", "lnZ"):
            a, b = (np.load(os.path.join(out, arm, name + ".npy")) for arm in ("parent", "tree"))
            assert a.shape == b.shape
            same = a.view(np.uint64) == b.view(np.uint64)
            fin = np.isfinite(a) & np.isfinite(b) & (a != 0)
            rel = np.abs(a[fin] - b[fin]) / np.abs(a[fin])
            print("%s.npy %s: %d of %d values bit-identical, largest relative change %.3g, NaN / inf in the same places: %s"
                  % (name, a.shape, same.sum(), a.size, rel.max() if rel.size else 0.0,
                     np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isinf(a), np.isinf(b))))
    finally:
        shutil.rmtree(out, ignore_errors=True)


if __name__ == "__main__":
    stage, parent, tree = sys.argv[1], os.path.abspath(sys.argv[2]), os.path.abspath(sys.argv[3])
    if stage == "census":
        census(os.path.abspath(sys.argv[4]))
    elif stage == "ab":
        ab(parent, tree)
    elif stage == "counters":
        counters(parent, tree)
    elif stage == "outputs":
        outputs(parent, tree)
    else:
        sys.exit("unknown stage " + stage)
