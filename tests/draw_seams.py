"""The comparisons of tests/golden/draw_seams.npz (the reference's samplers, relations and priors on inputs that hug their
seams: tests/golden/make_draw_seams.py), written once for two backends: tests/test_draw_seams_fixture.py feeds them the
torch expression of the chain on the CPU (tests/torch_pipeline.py) and the package's host functions, which proves the
fixture and this code without a GPU; tests/test_gpu_draw_columns.py feeds them the columns, masks and prior that
trx_draw_scenario writes for the same inputs, staged.

A backend answers, for arrays of staged inputs, with the columns a draw kernel call would write:
    rp(x, M_s, flat) -> R_p                          q(x, M_s) -> (m = q M_s, mask, mask_twin)
    qc(x, M_s, parallel) -> M_host = q_c M_s         angles(x) -> (inc, w)            ecc(u, P_orb) -> ecc
    relations(M, max_R, max_T, cc) -> dict(R_host, M_host, frc, u1, u2, lnprior)      (companions of a 1 M_sun star)
    prior(kind, M_s, plx, qc, cc, plxs=None) -> lnprior [len(qc)]  (or [len(plxs)][len(qc)])
    field(kind, idx, cc) -> dict(frc, M_host, lnprior)

Deviations are measured per column against the column's scale (the largest finite reference value), the yardstick of
tests/test_gpu_golden.py's 1e-12; the prior's absolutely (it enters lnZ additively, lnZ's tolerance is 1e-9).  Every
check RETURNS its deviation so that a caller can print what it measured before it asserts.
"""
import numpy as np

from helpers import gold

S = gold("draw_seams.npz")
CAPS = {"A": (0.8, 5100.0), "B": (20.0, 50000.0)}
STAR = (0.82, 0.8, 5100.0, 14.2)
COLUMN_CEILING, PRIOR_CEILING = 1e-12, 1e-9


def same_pattern(got, want, what):
    """NaN where the reference has NaN, the same infinities: a seam crossed the wrong way shows here first"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, what
    fin = np.isfinite(want)
    bad = np.flatnonzero(~((np.isfinite(got) == fin) & ((got == want) | fin | (np.isnan(got) & np.isnan(want)))))
    assert bad.size == 0, "%s: non-finite values differ at %s: got %s, reference %s" % (what, bad[:6], got.ravel()[bad[:6]],
                                                                                       want.ravel()[bad[:6]])
    return fin


def column_dev(got, want, what):
    """largest |got - want| over the column's scale"""
    fin = same_pattern(got, want, what)
    if not fin.any():
        return 0.0
    return float(np.max(np.abs(np.asarray(got)[fin] - np.asarray(want)[fin])) / np.max(np.abs(np.asarray(want)[fin])))


def prior_dev(got, want, what):
    fin = same_pattern(got, want, what)
    return float(np.max(np.abs(np.asarray(got)[fin] - np.asarray(want)[fin]))) if fin.any() else 0.0


def runs_of_adjacent_doubles(x):
    """labels of the contiguous runs of adjacent doubles in the sorted array x (a lone value is a run of its own): the
    generator hugs a seam with such a run"""
    places = np.asarray(x, dtype=np.float64).view(np.int64)
    return np.concatenate([[0], np.cumsum(np.diff(places) != 1)])


# How far the kernel's side of a seam may lie from the reference's, in doubles of the staged number: between that number
# and the compared quantity lie about a dozen rounded operations, each good for half a place -- six.  A run of adjacent
# doubles crossed by the seam then holds at most six draws on the other side; more is a seam in another place.
SEAM_PLACES = 6
# The lattice's ties: Teff / 250 and logg / 0.5 are a cubic in Horner form (four rounded operations; a division, a
# log10 and two products more for logg) against FITPACK's B-spline recurrence.  A draw may sit in the neighbouring cell
# only where the REFERENCE's own Teff / 250 or logg / 0.5 is within four doubles of the half-integer
TIE_PLACES = 4


def places_from_tie(x):
    """how many doubles x lies from the nearest half-integer"""
    x = np.asarray(x, dtype=np.float64)
    return np.abs(x - (np.floor(x) + 0.5)) / np.spacing(x)


def seam_prior_dev(got, want, labels, what, tol, values=True):
    """A prior along inputs that straddle a seam AT WHICH THE REFERENCE ITSELF JUMPS (delta_mag = 0: -inf above; a
    threshold of log10 P: another branch of the rate, -inf below the first).  Between the staged number and the compared
    quantity lie a dozen rounded operations that the kernel and numpy do not round alike (the splines as Horner forms
    against FITPACK's B-splines, exp(ln 10 x) against 10 ** x), so within the run of ADJACENT doubles that hugs the seam
    the kernel may sit on either side: there a value must be the reference's at SOME member of the same run.  A value
    outside a run, and the far members 2^6 and more doubles away, are runs of their own and must match in place.
    values=False: lnprior_bound_EB just above log10 P = 1, where its rate is f1 (log10 P - 1) to first order and the
    prior ln of that: one place of log10 P moves it by ln 2 next to the threshold and by 1e-6 still 2^20 places away,
    so no tolerance of the prior's means anything there -- only which draws get -inf (or NaN) is compared.  The same holds
    for lnprior_bound_TP just above ITS first threshold, log10 P = 3.4: the rate starts at k4 * (-3e-6), a few 1e-8 of
    either sign (negative: NaN for M_s >= 1, clamped to ln 0 below), and a place of log10 P moves its ln by 2e-9.
    Returns (deviation, values that took the other side's)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    worst, moved, per_run = 0.0, 0, {}
    for i in range(got.size):
        per_run[labels[i]] = per_run.get(labels[i], 0) - moved          # (+ moved after this draw: see below)
        cand = want[labels == labels[i]]
        if np.isfinite(got[i]) and not values:
            assert np.isfinite(cand).any(), "%s[%d]: %r where the reference's run has %s" % (what, i, got[i], cand)
            moved += int(not np.isfinite(want[i]))
        elif np.isfinite(got[i]):
            d = np.abs(cand[np.isfinite(cand)] - got[i])
            assert d.size, "%s[%d]: %r where the reference's run has %s" % (what, i, got[i], cand)
            here = abs(want[i] - got[i]) if np.isfinite(want[i]) else np.inf
            moved += int(not here <= tol)
            worst = max(worst, float(d.min()))
        else:
            ok = np.isnan(cand) if np.isnan(got[i]) else (cand == got[i])
            assert ok.any(), "%s[%d]: %r where the reference's run has %s" % (what, i, got[i], cand)
            moved += int(not ok[np.flatnonzero(labels == labels[i]) == i][0])
        per_run[labels[i]] += moved
    most = max(per_run.values()) if per_run else 0
    assert most <= SEAM_PLACES, "%s: %d draws of one run of adjacent doubles took the other side's value" % (what, most)
    return worst, moved


# ---- the checks: each returns {name: measured deviation} ---------------------------------------------------------------
def check_rp(b):
    x, out = S["rp_x"], {}
    for i, M in enumerate(S["rp_M"]):
        out["rp[M_s %d]" % i] = column_dev(b.rp(x, float(M), False), S["rp_out"][i], "sample_rp at M_s = %r" % float(M))
    out["rp[flat]"] = column_dev(b.rp(x, 0.82, True), S["rp_flat"], "sample_rp, flat law")
    # the fixture does straddle the switch of the two laws: M_s[1] and M_s[2] are adjacent and differ in the steep segment
    assert np.nextafter(S["rp_M"][1], 1.0) == S["rp_M"][2] and np.any(S["rp_out"][1] != S["rp_out"][2])
    return out


def check_q(b):
    out = {}
    for i, M in enumerate(S["q_M"]):
        M = float(M)
        x, want = S["q_x%d" % i], S["q_out%d" % i]
        m, mask, twin = b.q(x, M)
        out["m[M_s %d]" % i] = column_dev(m, want * M, "sample_q at M_s = %r" % M)
        # both masks on either side of q = 0.95 (every staged draw transits and none collides): where the reference's q
        # is clear of 0.95 by more than the columns' tolerance, by the reference; at an M_s that is a power of two, where
        # the column m shows the kernel's own q exactly, draw by draw by that
        clear = np.abs(want - 0.95) > 1e-12
        assert np.array_equal(mask[clear] != 0, want[clear] < 0.95) and np.array_equal(twin[clear] != 0, want[clear] >= 0.95), M
        assert not np.any((mask != 0) & (twin != 0))
        if M in (1.0, 0.5, 0.25, 0.125):                # q M_s is exact
            q = m / M
            assert np.array_equal(mask != 0, q < 0.95) and np.array_equal(twin != 0, q >= 0.95), M
            out["draws with q == 0.95 exactly"] = out.get("draws with q == 0.95 exactly", 0) + int(np.sum(q == 0.95))
        for par in (True, False):
            got = b.qc(x, M, par)
            out["M_host[M_s %d, parallel %d]" % (i, par)] = column_dev(got, S["qc_out%d" % i] * M, "sample_q_companion at M_s = %r" % M)
    return out


def check_angles_and_ecc(b):
    inc, w = b.angles(S["ang_x"])
    out = {"inc": column_dev(inc, S["inc_out"], "sample_inc"), "w": column_dev(w, S["w_out"], "sample_w")}
    for P, want in zip(S["ecc_P"], S["ecc_out"]):
        out["ecc[P_orb = %r]" % float(P)] = column_dev(b.ecc(S["ecc_u"], float(P)), want, "binaries' sample_ecc")
    assert np.max(np.abs(S["ecc_out"][0] - S["ecc_out"][1])) > 1e-3          # the two exponents
    return out


def check_relations(b):
    M, tie, out = S["rel_M"], S["rel_tie"], {}
    for tag, caps in CAPS.items():
        for cc in (False, True):
            got = b.relations(M, caps[0], caps[1], cc)
            key = "[caps %s%s]" % (tag, ", cc" if cc else "")
            out["R_host" + key] = column_dev(got["R_host"], S["rel_R_" + tag], "stellar_relations' radius" + key)
            fin = ~np.isnan(M)
            out["M_host" + key] = column_dev(got["M_host"][fin], M[fin], "the companion's mass" + key)
            out["fr_comp" + key] = column_dev(got["frc"], S["rel_share"], "flux_relation (TESS) share" + key)
            want = S["rel_lnprior_ccJ" if cc else "rel_lnprior_nocc"]
            labels = runs_of_adjacent_doubles(M[fin])
            dev, moved = seam_prior_dev(got["lnprior"][fin], want[fin], labels, "lnprior" + key, PRIOR_CEILING)
            out["lnprior" + key], out["lnprior" + key + ": values on the seam's other side"] = dev, moved
            # Teff shows in the limb-darkening cell alone.  Away from a rounding tie: the reference's cell.  In the run of
            # adjacent masses that hugs a tie of Teff / 250 or logg / 0.5 (found by bisecting the reference's relations):
            # the cell round-half-even selects from the reference's numbers for SOME member of the run -- the relations'
            # last bits differ between FITPACK's B-spline evaluation and the kernel's Horner form
            u1w, u2w = S["rel_u1_" + tag], S["rel_u2_" + tag]
            other, farthest = 0, 0.0
            near = np.minimum(places_from_tie(S["rel_T_" + tag] / 250), places_from_tie(S["rel_logg_" + tag] / 0.5))
            for i in np.flatnonzero(fin):
                cand = np.flatnonzero(tie == tie[i]) if tie[i] >= 0 else np.array([i])
                pairs = {(u1w[j], u2w[j]) for j in cand if np.isfinite(u1w[j])}
                if not np.isfinite(u1w[i]):
                    continue                           # (a cell the Claret grid lacks: the reference raises there)
                assert (got["u1"][i], got["u2"][i]) in pairs, ("limb-darkening cell" + key, i, M[i], got["u1"][i], u1w[i])
                if (got["u1"][i], got["u2"][i]) != (u1w[i], u2w[i]):
                    other += 1
                    farthest = max(farthest, float(near[i]))
                    assert near[i] <= TIE_PLACES, ("the neighbouring cell %g doubles from the tie" % near[i] + key, i, M[i])
            out["farthest from its tie, in doubles, of the draws on the other side" + key] = farthest
            out["cells on a tie's other side" + key] = other
    return out


def check_priors(b):
    out = {}
    for im, Ms in enumerate(S["prior_M"]):
        Ms = float(Ms)
        for cc in (False, True):
            key = "prior_%d_%s" % (im, "ccJ" if cc else "nocc")
            qc = S[key + "_qc"]
            labels = runs_of_adjacent_doubles(qc)
            for kind in ("TP", "EB"):
                what = "lnprior_bound_%s[M_s %r%s]" % (kind, Ms, ", cc" if cc else "")
                dev, moved = seam_prior_dev(b.prior(kind, Ms, STAR[3], qc, cc), S[key + "_" + kind], labels, what, PRIOR_CEILING)
                out[what], out[what + ": other side"] = dev, moved
        # the thresholds of log10 P by the parallax: no contrast curve, so log10 P is the same few exactly rounded
        # operations on the host's constants in the kernel and in numpy -- in place, no run
        for kind in ("TP", "EB"):
            what = "lnprior_bound_%s over parallax[M_s %r]" % (kind, Ms)
            got = b.prior(kind, Ms, None, S["plx_%d_qc" % im], False, plxs=S["plx_%d" % im])
            out[what] = prior_dev(got, S["plx_%d_%s" % (im, kind)], what)
            for it, thr in enumerate(S["prior_thr"]):
                key = "thr_%d_%d" % (im, it)
                what = "lnprior_bound_%s across log10 P = %g[M_s %r, cc]" % (kind, thr, Ms)
                qc = S[key + "_qc"]
                dev, moved = seam_prior_dev(b.prior(kind, Ms, float(S[key + "_plx"][0]), qc, True), S[key + "_" + kind],
                                            runs_of_adjacent_doubles(qc), what, PRIOR_CEILING,
                                            values=not ((kind == "EB" and thr == 1.0) or (kind == "TP" and thr == 3.4)))
                out[what], out[what + ": other side"] = dev, moved
    return out


def check_field(b):
    n, out = int(S["field_n"][0]), {}
    for kind, last in (("DTP", n - 2), ("DEB", n - 2), ("BTP", n - 1), ("BEB", n - 1)):
        idx = np.array([0, last, 1, last - 1])
        for cc in (False, True):
            got = b.field(kind, idx, cc)
            key = "[%s%s]" % (kind, ", cc" if cc else "")
            assert got["n_field_draw"] == last + 1, key
            if kind[1:] == "TP" or kind[0] == "D":
                out["fr_comp" + key] = column_dev(got["frc"], S["field_frc"][idx], "field star's flux ratio" + key)
            if kind[0] == "B":
                out["M_host" + key] = column_dev(got["M_host"], S["field_mass"][idx], "field star's mass" + key)
            if kind[1:] == "TP" or kind[0] == "D":
                # (lnZ_BEB's prior counts the star's eclipsing companion too: not a function of the index alone)
                want = S["field_lnprior_ccJ" if cc else "field_lnprior_nocc"][idx]
                out["lnprior" + key] = prior_dev(got["lnprior"], want, "lnprior_background" + key)
    return out


CHECKS = {"rp": check_rp, "q": check_q, "angles_ecc": check_angles_and_ecc, "relations": check_relations,
          "priors": check_priors, "field": check_field}
