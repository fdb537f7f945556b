#!/usr/bin/env python3
"""Generate tests/golden/draw_seams.npz: the REFERENCE's public samplers, stellar / flux relations and companion /
background priors (priors.py, funcs.py, imported through make_golden.install_shims) on inputs that hug their seams --
the breaks of the broken power laws, the 0.45 and 0.63 M_sun switches, the spline knots, the clamps and caps, the
rounding ties of the limb-darkening lattice, the contrast curve's knots and ends, delta_mag = 0 and the log P thresholds
of the bound-companion rate.  Every seam is LOCATED by bisecting the reference function (or, for the thresholds at which
its output is continuous, the reference's own expression of log10 P in the reference's constants) down to two adjacent
doubles; no constant of this project is read.  Only DATA leaves this script.  Deterministic: a re-run writes the same
arrays.  Re-run:  python tests/golden/make_draw_seams.py   (CPU only; needs the reference checkout).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True

from make_golden import install_shims  # noqa: E402

STAR = dict(M_s=0.82, R_s=0.8, Teff=5100.0, plx=14.2)          # the star of lnz_cases.npz
REL_STAR = dict(M_s=1.0, plx=14.2)                             # q_companion * 1.0 is the companion's mass, exactly
CAPS = {"A": (0.8, 5100.0), "B": (20.0, 50000.0)}              # (max_R, max_T): caps that act, caps that never do
# (just above 0.1: 2^20 doubles.  At the adjacent double q_min = 0.1 / M_s rounds to 1 and the two segments' integrals
# cancel exactly: 1 / 0 in the reference's Python floats, as in this project's)
Q_MASSES = (1.3, 1.0, float(np.nextafter(1.0, 0.0)), 0.7, 0.3, float(np.nextafter(0.3, 0.0)), 0.25,
            float((np.array([0.1]).view(np.int64) + 2 ** 20).view(np.float64)[0]), 0.1,
            # powers of two: q M_s is exact, so the column m shows the kernel's q itself (one per branch of the law)
            0.5, 0.125)
# (2.0: bright enough in J for a 0.1 M_sun companion to lie beyond the contrast curve's last knot, 7.95 mag)
PRIOR_MASSES = (0.82, 1.25, 2.0)
THRESHOLDS = (1.0, 2.0, 3.4, 5.5, 8.0)
RUN = 16                                                       # a seam's contiguous run: the pair and 16 doubles either side


def step(x, k):
    """the double k places after (before, k < 0) the positive double x"""
    return float((np.array([x], dtype=np.float64).view(np.int64) + k).view(np.float64)[0])


def bisect(pred, lo, hi):
    """pred(lo) is False and pred(hi) True (else None): the adjacent doubles (a, b), not pred(a) and pred(b)"""
    if pred(lo) or not pred(hi):
        return None
    while True:
        mid = lo + 0.5 * (hi - lo)
        if mid <= lo or mid >= hi:
            return lo, hi
        if pred(mid):
            hi = mid
        else:
            lo = mid


def hug(pair, run=RUN, far=(6, 10, 20, 30, 40), lo=0.0, hi=np.inf, stride=1):
    """the doubles around a bisected pair: a contiguous run (every stride-th double), and a few more 2^k places away"""
    if pair is None:
        return []
    a = pair[0]
    ks = [stride * k for k in range(-run, run + 2)] + [0, 1] + [s * 2 ** k for k in far for s in (-1, 1)]
    out = []
    for k in ks:
        if a == 0.0 and k < 0:
            continue
        v = step(a, k) if a > 0.0 else k * 5e-324
        if lo <= v < hi and np.isfinite(v):
            out.append(v)
    return out


def uniq(values):
    v = np.array(sorted(set(float(x) for x in values if not np.isnan(x))), dtype=np.float64)
    return v


def write_npz(path, arrays):
    """np.savez_compressed with the members in sorted order and a fixed date: a re-run writes the same bytes"""
    import io
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            z.writestr(info, buf.getvalue())


def main():
    install_shims()
    import triceratops.funcs as rfuncs
    import triceratops.marginal_likelihoods as rml
    import triceratops.priors as rpri

    G, Msun, Rsun, au, pi = rfuncs.G, rfuncs.Msun, rfuncs.Rsun, rfuncs.au, np.pi
    out = {}
    below1 = float(np.nextafter(1.0, 0.0))

    # ---- sample_rp ------------------------------------------------------------------------------------------------
    def rp1(x, M, flat=False):
        return rpri.sample_rp(np.array([x]), np.array([M]), flat)[0]

    x0 = 0.9
    M_lo, M_hi = bisect(lambda M: rp1(x0, M) == rp1(x0, 1.0), 0.4, 0.5)
    rp_M = np.array([step(M_lo, -1), M_lo, M_hi, step(M_hi, 1)])
    xs = [0.0, 5e-324, 2.0 ** -60, 0.25, 0.5, below1, step(below1, -1)]
    for M in (M_lo, M_hi):
        for R in (3.0, 6.0):
            xs += hug(bisect(lambda x: rp1(x, M) > R, 0.0, below1), hi=1.0)
        # the end of the last segment: the largest x the law still inverts (past it the reference returns x itself)
        xs += hug(bisect(lambda x: rp1(x, M) < 10.0, 0.5, 1.0 + 1e-9), hi=1.0 + 1e-9)
    xs = uniq(xs)
    out["rp_M"], out["rp_x"] = rp_M, xs
    out["rp_out"] = np.stack([rpri.sample_rp(xs.copy(), np.full(xs.size, M), False) for M in rp_M])
    out["rp_flat"] = rpri.sample_rp(xs.copy(), np.full(xs.size, 0.82), True)

    # ---- sample_q, sample_q_companion ---------------------------------------------------------------------------
    out["q_M"] = np.array(Q_MASSES)
    for i, M in enumerate(Q_MASSES):
        xs = [0.0, 5e-324, 2.0 ** -60, 2.0 ** -30, 0.5, below1, step(below1, -1)]
        for fn in (rpri.sample_q, rpri.sample_q_companion):
            def one(x):
                return fn(np.array([x]), M)[0]
            xs += hug(bisect(lambda x: one(x) >= 0.3, 0.0, below1), hi=1.0)
            xs += hug(bisect(lambda x: one(x) >= 0.95, 0.0, below1), run=64, hi=1.0)       # the twins' seam: both masks
            xs += hug(bisect(lambda x: one(x) < 0.9999, 0.5, 1.0 + 1e-9), hi=1.0 + 1e-9)
        xs = uniq(xs)
        out["q_x%d" % i] = xs
        out["q_out%d" % i] = rpri.sample_q(xs.copy(), M)
        out["qc_out%d" % i] = rpri.sample_q_companion(xs.copy(), M)

    # ---- sample_inc, sample_w, the binaries' eccentricity law -------------------------------------------------
    xs = np.array([0.0, 5e-324, 2.0 ** -60, 2.0 ** -30, 0.25, 0.5, 0.75, 1 - 2.0 ** -30, step(below1, -1), below1])
    out["ang_x"], out["inc_out"], out["w_out"] = xs, rpri.sample_inc(xs.copy()), rpri.sample_w(xs.copy())
    P10 = np.array([10.0, np.nextafter(10.0, 11.0)])
    ecc = []
    for P in P10:
        # (the reference's sample_ecc ignores its argument and draws from scipy's powerlaw on numpy's global stream:
        # u ** (1 / a) of the next uniforms)
        np.random.seed(31)
        ecc.append(rpri.sample_ecc(np.zeros(96), False, P))
    np.random.seed(31)
    u = np.random.uniform(size=96)
    for e, a in zip(ecc, (0.2, 0.6)):
        assert np.allclose(e, u ** (1.0 / a), rtol=4e-16, atol=0), "sample_ecc is not u ** (1 / a) of the stream"
    out["ecc_P"], out["ecc_u"], out["ecc_out"] = P10, u, np.stack(ecc)

    # ---- stellar_relations, flux_relation, the lattice ---------------------------------------------------------
    def rel(M, caps):
        M = np.atleast_1d(np.asarray(M, dtype=np.float64))
        return rfuncs.stellar_relations(M.copy(), np.full(M.size, caps[0]), np.full(M.size, caps[1]))

    def R1(M, caps=CAPS["B"]):
        return rel(M, caps)[0][0]

    def T1(M, caps=CAPS["B"]):
        return rel(M, caps)[1][0]

    knots = np.concatenate([rfuncs.Mass_nodes_Torres, rfuncs.Mass_nodes_cdwrf, rfuncs.Mass_nodes, rfuncs.Mass_nodes_J,
                            rfuncs.Mass_nodes_H, rfuncs.Mass_nodes_K])
    masses = []
    for k in np.unique(knots):
        masses += [step(k, -1), float(k), step(k, 1)]
    seam063 = bisect(lambda M: R1(M) > 0.62, 0.6, 0.66)             # the cool relation ends at R = 0.6, the hot starts at 0.65
    masses += hug(seam063, run=4, far=(6, 20))
    masses += hug(bisect(lambda M: R1(M) > 0.1, 0.05, 0.12), run=4, far=(6, 20))          # clamp R < 0.1
    masses += hug(bisect(lambda M: T1(M) > 2800.0, 0.05, 0.12), run=4, far=(6, 20))       # clamp T < 2800
    masses += hug(bisect(lambda M: R1(M, CAPS["A"]) >= CAPS["A"][0], 0.64, 1.2), run=4, far=(6, 20))      # cap max_R
    masses += hug(bisect(lambda M: T1(M, CAPS["A"]) >= CAPS["A"][1], 0.64, 1.2), run=4, far=(6, 20))      # cap max_T
    masses += [0.05, 0.08, 0.3, 0.5, 0.82, 1.0, 1.7, 3.5, 20.0]

    def logg1(M):
        R = R1(M)
        return np.log10(G * (M * Msun) / (R * Rsun) ** 2)

    # rounding ties of the lattice: Teff / 250 and logg / 0.5 at half-integers, on each monotonic stretch of the relations
    ties = []
    stretches = ((0.1, seam063[0]), (seam063[1], 3.0))
    for lo, hi in stretches:
        for h in np.arange(14.5, 40.0, 1.0):                      # (inside the lattice: 3500 .. 10000 K, 3.5 .. 5.0 dex)
            ties.append((bisect(lambda M: T1(M) / 250 >= h, lo, hi), 1))
        for h in (7.5, 8.5, 9.5):
            # (logg / 0.5 moves by one double per ~30 doubles of mass: every 32nd double, so that the run crosses the tie)
            ties.append((bisect(lambda M: logg1(M) / 0.5 <= h, lo, hi), 32))
    ties = [t for t in ties if t[0] is not None]
    tie_M = {}
    for k, (t, stride) in enumerate(ties):
        for m in hug(t, run=4, far=(), stride=stride):
            tie_M[m] = k
    masses = uniq(masses + list(tie_M))
    out["rel_M"] = np.concatenate([masses, [np.nan]])
    out["rel_tie"] = np.array([tie_M.get(float(m), -1) for m in out["rel_M"]])      # which tie's run a mass belongs to, or -1
    M = out["rel_M"]
    for band in ("TESS", "J", "H", "K"):
        out["flux_" + band] = rfuncs.flux_relation(M.copy(), band)
        for Ms in (REL_STAR["M_s"], STAR["M_s"]):
            out["flux0_%s_%g" % (band, Ms)] = rfuncs.flux_relation(np.array([Ms]), band)
    seps, cons = rfuncs.file_to_contrast_curve(os.path.join(HERE, "contrast_curve_synth.csv"))
    nocc = (np.array([2.2]), np.array([1.0]))

    def share(m, Ms, band="TESS"):
        # marginal_likelihoods.py:472-475, 492-496
        return rfuncs.flux_relation(m, band) / (rfuncs.flux_relation(m, band) + rfuncs.flux_relation(np.array([Ms]), band))

    def bound_prior(fn, Ms, plx, fr, cc):
        # marginal_likelihoods.py:481-507
        with np.errstate(all="ignore"):
            dm = 2.5 * np.log10(fr / (1 - fr))
            lp = fn(Ms, plx, np.abs(dm), *(cc if cc is not None else nocc))
            lp[lp > 0.0] = 0.0
            lp[dm > 0.0] = -np.inf
        return dm, lp

    out["rel_share"] = share(M.copy(), REL_STAR["M_s"])
    for tag, caps in CAPS.items():
        with np.errstate(all="ignore"):
            R, T = rel(M, caps)
            logg = np.log10(G * (M * Msun) / (R * Rsun) ** 2)                # marginal_likelihoods.py:931
        out["rel_R_" + tag], out["rel_T_" + tag], out["rel_logg_" + tag] = R, T, logg
        # the limb-darkening cell of lnZ_STP (marginal_likelihoods.py:945-972: TESS, Z = 0, Teff cap 10000)
        Zs = rml.ldc_T_Zs
        at_Z = rml.ldc_T[(Zs == Zs[np.abs(Zs - 0.0).argmin()])]
        tZ, gZ = np.array(at_Z.Teff, dtype=int), np.array(at_Z.logg, dtype=float)
        aZ, bZ = np.array(at_Z.aLSM, dtype=float), np.array(at_Z.bLSM, dtype=float)
        with np.errstate(all="ignore"):
            rg = np.round(logg / 0.5) * 0.5
            rg[rg < 3.5] = 3.5
            rg[rg > 5.0] = 5.0
            rt = np.round(T / 250) * 250
            rt[rt < 3500] = 3500
            rt[rt > 10000] = 10000
        u1, u2 = np.full(M.size, np.nan), np.full(M.size, np.nan)
        for i, (t_, g_) in enumerate(zip(rt, rg)):
            m = (tZ == t_) & (gZ == g_)
            if m.sum() == 1:                                   # (a cell the grid lacks: the reference raises)
                u1[i], u2[i] = aZ[m].item(), bZ[m].item()
        out["rel_u1_" + tag], out["rel_u2_" + tag] = u1, u2
        out["rel_cellT_" + tag], out["rel_cellg_" + tag] = rt, rg
    for cc_tag, cc, band in (("nocc", None, "TESS"), ("ccJ", (seps, cons), "J")):
        dm, lp = bound_prior(rpri.lnprior_bound_TP, REL_STAR["M_s"], REL_STAR["plx"], share(M.copy(), REL_STAR["M_s"], band), cc)
        out["rel_dm_" + cc_tag], out["rel_lnprior_" + cc_tag] = dm, lp

    # ---- the bound priors along q_companion, and the background prior ----------------------------------------
    def log10P(Ms, plx, sep_arcsec):
        # priors.py:603-613, in the reference's constants
        M_ref = Ms if Ms >= 1.0 else 1.0
        s = (1000 / plx) * sep_arcsec
        return np.log10(((4 * pi ** 2) / (G * M_ref * Msun) * (s * au) ** 3) ** (1 / 2) / 86400)

    out["prior_M"], out["prior_thr"] = np.array(PRIOR_MASSES), np.array(THRESHOLDS)
    out["cc_seps"], out["cc_cons"] = seps, cons
    for im, Ms in enumerate(PRIOR_MASSES):
        f0 = {b: rfuncs.flux_relation(np.array([Ms]), b) for b in ("TESS", "J")}

        def dm_of(qc, band):
            fr = share(np.array([qc * Ms]), Ms, band)[0]
            return 2.5 * np.log10(fr / (1 - fr))

        for cc_tag, cc, band in (("nocc", None, "TESS"), ("ccJ", (seps, cons), "J")):
            q_lo = 0.1 / Ms                  # (a 0.1 M_sun companion: the mass ratios are staged as they are, qc_in)
            qs = [q_lo, step(q_lo, 1), 0.2, 0.35, 0.5, 0.7, 0.9, 1.2]
            qs += hug(bisect(lambda q: dm_of(q, band) > 0.0, 0.5, 1.5), run=8, far=(6, 20))          # delta_mag straddles 0
            if cc is not None:
                for c in cons:                                  # |delta_mag| at every knot of the contrast curve
                    pair = bisect(lambda q: -dm_of(q, band) <= c, q_lo, 1.0)
                    qs += hug(pair, run=1, far=())
            qs = uniq(qs)
            key = "prior_%d_%s" % (im, cc_tag)
            out[key + "_qc"] = qs
            fr = share(qs * Ms, Ms, band)
            for kind, fn in (("TP", rpri.lnprior_bound_TP), ("EB", rpri.lnprior_bound_EB)):
                dm, lp = bound_prior(fn, Ms, STAR["plx"], fr, cc)
                out[key + "_dm"], out[key + "_" + kind] = dm, lp
        # the thresholds of log10 P without a contrast curve (the separation is 2.2 arcsec): by the parallax
        qs = np.array([0.3, 0.6, 0.9])
        fr = share(qs * Ms, Ms, "TESS")
        plxs = []
        for thr in THRESHOLDS:
            pair = bisect(lambda p: log10P(Ms, p, 2.2) < thr, 1e-6, 1e6)          # (a, b): log10 P(a) >= thr > log10 P(b)
            plxs += hug(pair, run=4, far=(8,))
        # where the reference's OUTPUT jumps to -inf: lnprior_bound_TP below log10 P = 3.4 -- for M_s >= 1 exactly there
        # (just above, its rate is slightly negative and the log NaN); for M_s < 1 the negative rate is clamped to 0, so
        # -inf lasts until the rate turns positive, 1e10 doubles of parallax further -- and lnprior_bound_EB at log10 P = 1
        # itself, where its rate is exactly 0: at most one double of parallax above the threshold's
        for kind, fn, thr in (("TP", rpri.lnprior_bound_TP, 3.4), ("EB", rpri.lnprior_bound_EB, 1.0)):
            jump = bisect(lambda p: np.isneginf(bound_prior(fn, Ms, p, fr[:1], None)[1][0]), 1e-6, 1e6)
            at = bisect(lambda p: log10P(Ms, p, 2.2) < thr, 1e-6, 1e6)
            places = int(np.array([at[0]]).view(np.int64)[0] - np.array([jump[0]]).view(np.int64)[0])
            assert (places == 0) if (kind == "TP" and Ms >= 1.0) else (places >= (0 if kind == "EB" else 1)), (kind, Ms, places)
            if places <= 1:
                plxs += hug(jump, run=2, far=())
        plxs = uniq(plxs)
        out["plx_%d" % im], out["plx_%d_qc" % im] = plxs, qs
        for kind, fn in (("TP", rpri.lnprior_bound_TP), ("EB", rpri.lnprior_bound_EB)):
            out["plx_%d_%s" % (im, kind)] = np.stack([bound_prior(fn, Ms, p, fr, None)[1] for p in plxs])
        # ... and with the contrast curve: delta_mag placed so that log10 P straddles each threshold, at a parallax that
        # puts the threshold's separation in the middle of the curve (1 arcsec)
        for it, thr in enumerate(THRESHOLDS):
            pair = bisect(lambda p: log10P(Ms, p, 1.0) < thr, 1e-6, 1e6)
            plx = float("%.6g" % pair[0])

            def lp_of(qc):
                dm = dm_of(qc, "J")
                return log10P(Ms, plx, np.interp(abs(dm), cons, seps))

            q_lo = 0.1 / Ms if Ms < 1.0 else 0.1
            pair = bisect(lambda q: lp_of(q) < thr, q_lo, 1.0)
            qs = uniq(hug(pair, run=8, far=(6, 20)))
            key = "thr_%d_%d" % (im, it)
            out[key + "_plx"], out[key + "_qc"] = np.array([plx]), qs
            fr_cc = share(qs * Ms, Ms, "J")
            for kind, fn in (("TP", rpri.lnprior_bound_TP), ("EB", rpri.lnprior_bound_EB)):
                out[key + "_" + kind] = bound_prior(fn, Ms, plx, fr_cc, (seps, cons))[1]

    # ---- the field stars at the ends of the index draw (marginal_likelihoods.py:1452-1492, 1897-1955) -------------
    tri = os.path.join(HERE, "trilegal_synth.csv")
    Tmag, Jmag = 10.4, 9.5
    (Tm, masses_f, loggs_f, Teffs_f, Zs_f, Jm, Hm, Km) = rfuncs.trilegal_results(tri, Tmag)
    dT, dJ = Tmag - Tm, Jmag - Jm
    frc = 10 ** (dT / 2.5) / (1 + 10 ** (dT / 2.5))
    n = Tm.shape[0]
    out["field_n"] = np.array([n])
    out["field_mass"], out["field_frc"] = np.asarray(masses_f, dtype=float), frc
    with np.errstate(all="ignore"):
        dm = 2.5 * np.log10(frc / (1 - frc))
        lp = np.full(n, np.log((n / 0.1) * (1 / 3600) ** 2 * 2.2 ** 2))
        lp[lp > 0.0] = 0.0
        lp[dm > 0.0] = -np.inf
        out["field_lnprior_nocc"] = lp
        lp = rpri.lnprior_background(n, np.abs(dJ), seps, cons)
        lp[lp > 0.0] = 0.0
        lp[dJ > 0.0] = -np.inf
        out["field_lnprior_ccJ"] = lp
    # the background prior on the contrast curve's knots and ends
    dms = []
    for c in cons:
        dms += [step(c, -1), float(c), step(c, 1)]
    dms = uniq(dms + [0.0, 5e-324, 0.1, 9.0, 30.0])
    out["bg_dm"], out["bg_out"] = dms, rpri.lnprior_background(n, dms.copy(), seps, cons)

    write_npz(os.path.join(HERE, "draw_seams.npz"), out)
    print("wrote draw_seams.npz: %d arrays, %d values" % (len(out), sum(np.asarray(v).size for v in out.values())))


if __name__ == "__main__":
    main()
