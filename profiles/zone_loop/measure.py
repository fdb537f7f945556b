"""Measurements for the zone loop and the centre deficits of cells_kernel's one-row stencil likelihood instantiations
("zone loop").

    python profiles/zone_loop/measure.py ab       <reps> <name>=<libtrx.so> <name>=<libtrx.so> [...]
    python profiles/zone_loop/measure.py counters <name>=<libtrx.so> [...]
    python profiles/zone_loop/measure.py outputs  <parent libtrx.so> <tree libtrx.so>
    python profiles/zone_loop/measure.py chunks   <tree libtrx_testing.so>

Stages (each a job of its own; every GPU step is a child process under its own time limit, and the first failure ends
the stage):
  ab        same-job A/B of production builds, the arms alternating <reps> times: bench.py --gpus 1 --steps 20 --warmup 5
            --full --no-cpu-baseline --no-e2e with TRX_LIB naming the build (config 1, and the controls: 2000 irregular
            stamps, 100 / 200 points, the 64-TOI step); the first arm is the one the others are compared with
  counters  rocprofv3 --pmc alone, one pass of the 18 families per build (profiles/r07/cells2000_once.py)
  outputs   bench.py --dump-outputs per build: halfchi2.npy, lnZ.npy and lnZ_checksum must be EQUAL
  chunks    the testing library on 18 x 512 bench rows of 2000 uniform points: first-sweep chunks are on record
            (profiles/full_chunks/results.txt); here the chunks the zone loop took, per row
Everything is printed; profiles/zone_loop/results.txt is the record.
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


def arms_of(args):
    return [(a.split("=", 1)[0], os.path.abspath(a.split("=", 1)[1])) for a in args]


KEYS = ("cfg1", "value", "ms_per_step", "irregular", "n100", "n200", "toi64")


def ab(reps, arms):
    rec = {name: [] for name, _ in arms}
    for rep in range(1, reps + 1):
        for name, lib in arms:
            d = last_json(run([PY, "bench.py", "--gpus", "1", "--full", "--steps", "20", "--warmup", "5", "--no-cpu-baseline",
                               "--no-e2e", "--pmc", "off"], 500, lib))
            sh, b = d.get("shapes") or {}, d.get("batch") or {}
            row = {"cfg1": d["roofline"]["mean_launch_ms"], "value": d["value"], "ms_per_step": d["ms_per_step"],
                   "irregular": (sh.get("n2000_irregular") or {}).get("mean_launch_ms", float("nan")),
                   "n100": (sh.get("n100") or {}).get("mean_launch_ms", float("nan")),
                   "n200": (sh.get("n200") or {}).get("mean_launch_ms", float("nan")),
                   "toi64": b.get("ms_per_step", float("nan")), "checksum": d["lnZ_checksum"]}
            rec[name].append(row)
            print("%-8s rep %d  cfg1 %.4f ms  value %.4e/s  ms_per_step %.3f | irregular %.4f ms | n100 %.4f n200 %.4f | "
                  "64-TOI step %.2f ms | lnZ_checksum %.17g"
                  % (name, rep, row["cfg1"], row["value"], row["ms_per_step"], row["irregular"], row["n100"], row["n200"],
                     row["toi64"], row["checksum"]))
            sys.stdout.flush()
    base = arms[0][0]
    for name, _ in arms[1:]:
        for key in KEYS:
            p, t = (np.array([r[key] for r in rec[a]]) for a in (base, name))
            spread = max(p.max() - p.min(), t.max() - t.min())
            every = bool((t < p).all()) if key != "value" else bool((t > p).all())
            print("%-11s %s %.5g (spread %.3g)  %s %.5g (spread %.3g)  difference %+.4g = %+.2f %% = %.1f within-arm spreads; "
                  "better in every pair: %s"
                  % (key, base, p.mean(), p.max() - p.min(), name, t.mean(), t.max() - t.min(), t.mean() - p.mean(),
                     100.0 * (t.mean() - p.mean()) / p.mean(), abs(p.mean() - t.mean()) / spread if spread > 0 else float("inf"), every))


def counters(arms):
    out = tempfile.mkdtemp(prefix="zone_loop_pmc_")
    try:
        for name, lib in arms:
            d = os.path.join(out, "pmc_" + name)
            run(["rocprofv3", "--pmc", "SQ_INSTS_VALU", "SQ_ACTIVE_INST_VALU", "SQ_BUSY_CYCLES", "SQ_WAVE_CYCLES",
                 "--output-format", "csv", "-d", d, "--", PY, "profiles/r07/cells2000_once.py"], 240, lib, stderr=subprocess.STDOUT)
            text = run([PY, "profiles/pmc_summary.py", d], 120, lib, stderr=subprocess.STDOUT)
            print("== counters, %s" % name)
            lines = text.splitlines()
            for i, line in enumerate(lines):
                if "cells_kernel" in line and "<0" in line.replace(" ", ""):
                    print("\n".join(lines[i:i + 5]))
            sys.stdout.flush()
    finally:
        shutil.rmtree(out, ignore_errors=True)


def outputs(parent, tree):
    out = tempfile.mkdtemp(prefix="zone_loop_dump_")
    try:
        ck = {}
        for arm, lib in (("parent", parent), ("tree", tree)):
            d = last_json(run([PY, "bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1", "--no-cpu-baseline",
                               "--dump-outputs", os.path.join(out, arm)], 300, lib))
            ck[arm] = d["lnZ_checksum"]
        ok = ck["parent"] == ck["tree"]
        print("lnZ_checksum parent %.17g tree %.17g equal: %s" % (ck["parent"], ck["tree"], ok))
        for name in ("halfchi2", "lnZ"):
            a, b = (np.load(os.path.join(out, arm, name + ".npy")) for arm in ("parent", "tree"))
            places = np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isinf(a), np.isinf(b))
            equal = places and np.array_equal(a[np.isfinite(a)], b[np.isfinite(b)]) and \
                np.array_equal(a[np.isinf(a)], b[np.isinf(b)])
            bits = int((a.view(np.uint64) == b.view(np.uint64)).sum())
            print("%s.npy %s: np.array_equal %s, %d of %d values bit-identical, non-finite entries in the same places: %s"
                  % (name, a.shape, equal, bits, a.size, places))
            ok = ok and equal and bits == a.size
        print("outputs equal: %s" % ok)
        if not ok:
            sys.exit(1)
    finally:
        shutil.rmtree(out, ignore_errors=True)


def chunks(testing):
    print(run([PY, "profiles/zone_loop/zone_chunks.py"], 240, testing))


if __name__ == "__main__":
    stage = sys.argv[1]
    if stage == "ab":
        ab(int(sys.argv[2]), arms_of(sys.argv[3:]))
    elif stage == "counters":
        counters(arms_of(sys.argv[2:]))
    elif stage == "outputs":
        outputs(os.path.abspath(sys.argv[2]), os.path.abspath(sys.argv[3]))
    elif stage == "chunks":
        chunks(os.path.abspath(sys.argv[2]))
    else:
        sys.exit("unknown stage " + stage)
