"""What calc_probs_datasets leaves, and how long a pass takes, per kind of dataset term -- to compare two versions of the
host plumbing (fused.py, triceratops.py, datasets.py) on the same library: bit for bit, and in wall time.

    python profiles/dataset_terms/compare.py run OUT.npz [--root DIR] [--passes 5]
    python profiles/dataset_terms/compare.py diff A.npz B.npz [...]

run:  the two-cadence TOI-465 fixture of tests/test_gpu_datasets.py (N = 4000, seed 465, six scenarios), once per kind
      of term on dataset 1 and once more with a two-node t0_grid next to a column kind.  Per configuration one warm-up pass,
      whose lnZ, probs, every dataset_* attribute and _lib.STATS go to OUT.npz, then `passes` timed passes (seconds, device
      synchronised).  --root: the directory whose triceratops_amd is imported (another version's .py files; TRX_LIB names
      the library), default this checkout.
diff: every array of every file against A's byte for byte, STATS included; and the median pass time per configuration of
      each file (series of the two versions run in turn: the spread among one version's series is the noise)."""
import argparse
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
GOLD = os.path.join(REPO, "tests", "golden")
SEED = 465
STAR_COLS = ("ID", "Tmag", "Jmag", "Hmag", "Kmag", "ra", "dec", "mass", "rad", "Teff", "plx", "fluxratio", "tdepth")
ATTRS = ("dataset_offsets", "dataset_baselines", "dataset_red_noise", "dataset_t0", "dataset_outliers",
         "dataset_red_baselines", "dataset_white_noise", "dataset_white_baselines", "dataset_red_kernel_baselines")


def configurations(sigma, n):
    cols = np.stack([np.ones(n), np.linspace(-1.0, 1.0, n)])
    ou = {"red_sigma": sigma, "red_timescale": 0.05}
    m32 = dict(ou, red_kernel="matern32")
    white = [(1.0, 0.0, 1.0), (1.5, 0.5 * sigma, 3.0)]
    kinds = {
        "none": {},
        "offset": {"offset_sigma": sigma},
        "baseline": {"baseline": cols, "baseline_sigma": 10 * sigma, "offset_sigma": sigma},
        "ou": ou,
        "ou_mix": {"red_grid": [(sigma, 0.05, 1.0), (0.5 * sigma, 0.5, 3.0)]},
        "ou_lin": dict(ou, red_baseline=cols, red_baseline_sigma=10 * sigma),
        "ss2": m32,
        "ss2_lin": dict(m32, red_kernel_baseline=cols, red_kernel_baseline_sigma=10 * sigma),
        "robust": {"outlier_frac": 0.05, "outlier_scale": 5.0},
        "white_mix": {"white_grid": white},
        "white_lin": {"white_grid": white, "white_baseline": cols, "white_baseline_sigma": 10 * sigma},
    }
    kinds["ou_lin_t0"] = dict(kinds["ou_lin"], t0_grid=[(-0.005, 1.0), (0.005, 3.0)])
    return kinds


def flatten(value, path, out):
    """arrays of a nested list / dict / None structure under their paths; a None leaves a marker"""
    if value is None:
        out[path + "/none"] = np.zeros(0)
    elif isinstance(value, dict):
        for k in sorted(value):
            flatten(value[k], "%s/%s" % (path, k), out)
    elif isinstance(value, (list, tuple)):
        out[path + "/len"] = np.array([len(value)])
        for i, v in enumerate(value):
            flatten(v, "%s/%d" % (path, i), out)
    else:
        out[path] = np.asarray(value)


def run(args):
    sys.path.insert(0, os.path.abspath(args.root))
    import pandas as pd
    import torch
    import triceratops_amd as ta
    from triceratops_amd import _lib
    from triceratops_amd.triceratops import target
    assert os.path.dirname(os.path.dirname(os.path.abspath(ta.__file__))) == os.path.abspath(args.root)
    G = np.load(os.path.join(GOLD, "toi465_calc_probs.npz"))
    st = pd.DataFrame({c: G["real_stars_%s" % c] for c in STAR_COLS})
    st["ID"] = st["ID"].astype(np.int64)
    tg = target(270380593, np.array([4]), stars=st, trilegal_fname=os.path.join(GOLD, "trilegal_synth.csv"))
    t, y, sigma, P_orb = G["time"], G["flux"], float(G["sigma"][0]), float(G["P_orb"][0])
    ia, ib = np.arange(0, 100, 2), np.arange(2, 100, 4)[:21]
    a = {"time": t[ia], "flux": y[ia], "flux_err": sigma * np.linspace(0.6, 1.8, 50), "exptime": 0.00139, "nsamples": 20}
    b = {"time": t[ib], "flux": y[ib], "flux_err": 1.4 * sigma, "exptime": 0.0208, "nsamples": 5}
    kw = dict(contrast_curve_file=os.path.join(GOLD, "toi465_cc.csv"), N=4000, parallel=True, verbose=0,
              drop_scenario=["STP", "SEB", "DTP", "DEB", "BTP", "BEB"])
    ta.set_sampling("device")
    out = {}
    for name, keys in configurations(1.4 * sigma, ib.size).items():
        seconds = []
        for k in range(1 + args.passes):
            torch.manual_seed(SEED)
            _lib.reset_stats()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tg.calc_probs_datasets([a, dict(b, **keys)], P_orb, **kw)
            torch.cuda.synchronize()
            seconds.append(time.perf_counter() - t0)
            stats = np.array([_lib.STATS[s] for s in ("rows", "cells", "launches")], dtype=np.int64)
            if k == 0:
                out[name + "/stats"] = stats
                out[name + "/lnZ"] = np.asarray(tg.lnZ)
                out[name + "/prob"] = tg.probs.prob.values.copy()
                for attr in ATTRS:
                    flatten(getattr(tg, attr), "%s/%s" % (name, attr), out)
            else:
                assert np.array_equal(stats, out[name + "/stats"]), "STATS differ between passes"
        out["seconds/" + name] = np.array(seconds[1:])
        print("%-10s median %.4f s  stats %s" % (name, np.median(seconds[1:]) if args.passes else 0.0, stats.tolist()),
              flush=True)
    np.savez(args.out, **out)


def diff(args):
    files = [dict(np.load(f)) for f in args.files]
    a = files[0]
    keys = sorted(k for k in a if not k.startswith("seconds/"))
    same, bad = True, []
    for b in files[1:]:
        same = same and keys == sorted(k for k in b if not k.startswith("seconds/"))
        bad += [k for k in keys if k not in b or a[k].dtype != b[k].dtype or a[k].shape != b[k].shape
                or a[k].tobytes() != b[k].tobytes()]
    print("%d arrays (lnZ, prob, dataset_* attributes, STATS) of %d configurations in %d files: %s"
          % (len(keys), len([k for k in a if k.startswith("seconds/")]), len(files),
             "all byte for byte the same" if same and not bad else "DIFFERENT: %s" % (bad or "the key sets")))
    print("median milliseconds of a pass: " + "  ".join(os.path.basename(f)[:-4] for f in args.files))
    for k in sorted(k for k in a if k.startswith("seconds/")):
        print("  %-10s " % k[8:] + "  ".join("%.3f" % (1e3 * np.median(f[k])) for f in files))
    return 0 if same and not bad else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="cmd", required=True)
    r = sub.add_parser("run")
    r.add_argument("out")
    r.add_argument("--root", default=REPO)
    r.add_argument("--passes", type=int, default=5)
    d = sub.add_parser("diff")
    d.add_argument("files", nargs="+")
    a = ap.parse_args()
    sys.exit(run(a) if a.cmd == "run" else diff(a))
