"""The draw kernel (csrc/trx_draw.hip) checked directly: every draw's columns, mask(s) and companion prior, where the rest
of the suite sees them only through lnZ and the best hundred draws.

1. Every draw of the reference's seeded runs (tests/golden/lnz_cases.npz): the operator chain's masks, columns and prior
   against the blocks the reference handed its likelihood and its log-weights, draw for draw.
2. The seams of the chain (tests/golden/draw_seams.npz, made by bisecting the reference's own functions; the comparisons
   and their CPU proof: tests/draw_seams.py, tests/test_draw_seams_fixture.py), staged into trx_draw_scenario.
3. The boundary of the geometry mask against 30-digit arithmetic on the kernel's own columns, and the fp32 pre-test of
   the library's own chain on the same staged numbers.
"""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import draw_seams as ds
from helpers import GOLD, gold, scenario, staged

pytestmark = pytest.mark.gpu

G = gold("lnz_cases.npz")
CC = os.path.join(GOLD, "contrast_curve_synth.csv")
TRI = os.path.join(GOLD, "trilegal_synth.csv")
PARALLEL_CASES = [str(c) for c in G["cases"] if not str(c).endswith("_serial")]
LC = (G["time"], G["flux"], float(G["sigma"][0]))
MAGS = (10.4, 9.5, 9.1, 9.0)


@pytest.fixture(autouse=True)
def _host_caches_as_found():
    """These tests build a few thousand argument blocks.  fused's host caches (light curves on the device, power-law and
    flux constants, populations) empty themselves when they overflow, and where that happens depends on everything that
    ran before: a later test that counts launch chains needs its calls to find ONE device copy of their light curve.
    Every test here hands the caches back as it found them."""
    from triceratops_amd import fused
    caches = {n: getattr(fused, n) for n in dir(fused) if n.endswith("_cache") and isinstance(getattr(fused, n), dict)}
    saved = {n: dict(c) for n, c in caches.items()}
    yield
    for n, c in caches.items():
        c.clear()
        c.update(saved[n])


def _bound(measured, ceiling):
    """eight times what was measured on the GPU (the docstrings carry the figures), or the project's ceiling if smaller"""
    return min(8.0 * measured, ceiling)


# ---- 1. every draw of the reference's seeded runs ----------------------------------------------------------------------
# measured on the GPU over the 28 cases: largest column deviation 1.8e-15 of the column's scale (the orbit's a: a cube root),
# largest |lnprior - (logw - lnL)| 2.3e-10 (DEB_ccJ: lnL ~ -5e5 there, so logw - lnL itself is only good to its ulps)
CASE_COLUMNS, CASE_PRIOR = 1.8e-15, 2.3e-10


def _lnz(name, P, cc, filt):
    from triceratops_amd import marginal_likelihoods as ml
    s = dict(zip(("M_s", "R_s", "Teff", "Z", "plx", "Tmag", "Jmag", "Hmag", "Kmag"), (float(v) for v in G["star"])))
    base = LC + (P, s["M_s"], s["R_s"], s["Teff"])
    fn, N = getattr(ml, "lnZ_" + name), int(G["N"][0])
    if name in ("TTP", "TEB"):
        return fn(*base, 0.0, N, True)
    if name in ("PTP", "PEB", "STP", "SEB"):
        return fn(*base, 0.0, s["plx"], cc, filt, N, True)
    mags = (s["Tmag"], s["Jmag"], s["Hmag"], s["Kmag"])
    if name in ("DTP", "DEB"):
        return fn(*base, 0.0, *mags, TRI, cc, filt, N, True)
    return fn(*base, *mags, TRI, cc, filt, N, True)


@pytest.mark.parametrize("case", PARALLEL_CASES)
def test_every_draw_of_the_reference_s_seeded_runs(case):
    """The operator chain ("numpy-device" with fused.DUMP: trx_draw_scenario, every draw in full) from the case's seed.
    Per branch: as many masked draws as the reference's block is wide; the masked draws' columns ARE the block, row for
    row in draw order (one misplaced mask bit shifts everything after it); every draw with a finite log-weight is masked;
    and there the prior column is logw - lnL, lnL rebuilt from the reference's own chi^2/2 as the reference builds it
    (marginal_likelihoods.py:130: -0.5 ln 2 pi - ln sigma - out).  The twin branch's block holds 2 P_orb and the orbit at
    2 P_orb (column a_twin), as run_operator_chain forms it for trx_lnl_batch.
    Measured (GPU, all cases): columns <= 1.8e-15 of the column's scale, prior <= 2.3e-10 (0 for TTP / TEB, which have
    none); asserted at 8x, capped by 1e-12 and 1e-9."""
    import triceratops_amd
    from triceratops_amd import _lib, fused
    _lib.require_gpu()
    name, variant = case.split("_")
    P = [2.5, 4.0] if variant == "range" else 3.3
    cc = CC if variant == "ccJ" else None
    triceratops_amd.set_sampling("numpy-device")
    fused.DUMP = []
    try:
        np.random.seed(int(G[case + "_seed"][0]))
        _lnz(name, P, cc, "J" if cc else "TESS")
        torch.cuda.synchronize()
        d = {k: (None if v is None else v.cpu().numpy()) for k, v in fused.DUMP[0].items()}
    finally:
        fused.DUMP = None
        triceratops_amd.set_sampling("numpy")
    cols, N = d["cols"], int(G["N"][0])
    masks = [d["mask"]] if d["mask_twin"] is None else [d["mask"], d["mask_twin"]]
    lnprior = np.zeros(N) if d["lnprior"] is None else d["lnprior"]
    assert (d["lnprior"] is None) == (name in ("TTP", "TEB"))
    sigma = LC[2]
    worst_col = worst_prior = 0.0
    for b, mask in enumerate(masks):
        block = G["%s_call%d_block" % (case, b)]
        idx = np.flatnonzero(mask)
        assert idx.size == block.shape[1], (case, b, idx.size, block.shape)
        rows = block.shape[0]
        got = cols[:rows][:, idx].copy()
        if b == 1:
            got[2] *= 2.0
            got[4] = cols[11][idx]
        for r in range(rows):
            if idx.size:
                dev = ds.column_dev(got[r], block[r], "%s branch %d row %d" % (case, b, r))
                worst_col = max(worst_col, dev)
        logw = G["%s_logw%d" % (case, b)]
        fin = np.isfinite(logw)
        assert mask[fin].all(), (case, b)
        lnL = np.full(N, -np.inf)
        lnL[idx] = -0.5 * np.log(2 * np.pi) - np.log(sigma) - G["%s_call%d_out" % (case, b)]
        if fin.any():
            worst_prior = max(worst_prior, float(np.max(np.abs(lnprior[fin] - (logw[fin] - lnL[fin])))))
        # (a masked draw without a finite log-weight: the likelihood excluded it, or its prior is -inf)
        gone = mask.astype(bool) & ~fin
        assert np.all(np.isinf(lnL[gone]) | (lnprior[gone] == -np.inf) | np.isnan(lnprior[gone])), (case, b)
    print("%s: columns %.3g of scale, prior %.3g" % (case, worst_col, worst_prior))
    assert worst_col <= _bound(CASE_COLUMNS, ds.COLUMN_CEILING), worst_col
    assert worst_prior <= _bound(CASE_PRIOR, ds.PRIOR_CEILING), worst_prior
    if name in ("TTP", "TEB"):
        assert worst_prior <= 2e-10       # no prior: logw - lnL is 0 but for the reference's own rounding of lnL + 0


# ---- 2. the seams ------------------------------------------------------------------------------------------------------
class KernelBackend:
    """draw_seams' questions answered by trx_draw_scenario: the inputs staged as uRp, uQ, uQc, uInc, uW, uEcc, qc_in (and
    the field-star index), the answers read off the columns, masks and prior of all draws.  The argument block is the one
    the project's own lnZ_* builds for the call (helpers.scenario): its host constants are under test too."""

    def __init__(self):
        from triceratops_amd import fused
        self.fused = fused

    def _draw(self, build, rows, qc_in=None, same_masks=False):
        """build(parallel) -> the call's _Scenario.  Staged with BOTH values of `parallel`: the columns and the prior do
        not know it (asserted: the same bytes); the masks do where P_tra > 1 (a staged inclination that rounds to 90 deg
        transits on the vector path only), so they are held equal only where the caller says that every draw transits
        (same_masks).  Returns the vector path's outputs and the scenario"""
        outs = []
        for parallel in (True, False):
            s = build(parallel)
            dump = np.zeros((9, s.N))
            # every draw transits unless a check says otherwise: inc = 90 - 6e-15 deg, e = 0.01 ** 5, w = 0
            dump[3], dump[5], dump[8] = np.nextafter(1.0, 0.0), 0.01, 1e-10
            for r, v in rows.items():
                dump[r] = v
            outs.append(staged({"scen": s, "dump": dump}, self.fused, qc_in=qc_in))
        a, b = outs
        for k in ("cols", "lnprior") + (("mask", "mask_twin") if same_masks else ()):
            assert (a[k] is None) == (b[k] is None) and (a[k] is None or a[k].tobytes() == b[k].tobytes()), k
        a["scen"] = s
        return a

    def rp(self, x, M_s, flat):
        return self._draw(lambda par: scenario("TTP", *LC, 3.3, M_s, 0.8, 5100.0, 0.0, x.size, par, "TESS", flat), {2: x})["cols"][0]

    def q(self, x, M_s):
        o = self._draw(lambda par: scenario("TEB", *LC, 3.3, M_s, max(M_s, 0.1), 5100.0, 0.0, x.size, par), {4: x},
                       same_masks=True)
        return o["cols"][12], o["mask"], o["mask_twin"]

    def qc(self, x, M_s, parallel):
        # (draw_seams asks twice: the planet layout through STP, the binary layout through SEB)
        name = "STP" if parallel else "SEB"
        build = lambda par: scenario(name, *LC, 3.3, M_s, max(M_s, 0.1), 5100.0, 0.0, 14.2, None, "TESS", x.size, par)
        return self._draw(build, {1: x, 4: 0.5})["cols"][10 if parallel else 13]

    def angles(self, x):
        c = self._draw(lambda par: scenario("TTP", *LC, 3.3, 0.82, 0.8, 5100.0, 0.0, x.size, par), {3: x, 6: x, 2: 0.5})["cols"]
        return c[2], c[8]

    def ecc(self, u, P_orb):
        return self._draw(lambda par: scenario("TEB", *LC, P_orb, 0.82, 0.8, 5100.0, 0.0, u.size, par), {5: u, 4: 0.5})["cols"][8]

    def relations(self, M, max_R, max_T, cc):
        build = lambda par: scenario("STP", *LC, 3.3, 1.0, max_R, max_T, 0.0, ds.STAR[3], CC if cc else None,
                                     "J" if cc else "TESS", M.size, par)
        o = self._draw(build, {2: 0.5}, qc_in=M)
        c = o["cols"]
        return {"R_host": c[4], "M_host": c[10], "frc": c[9], "u1": c[5], "u2": c[6], "lnprior": o["lnprior"]}

    def prior(self, kind, M_s, plx, qc, cc, plxs=None):
        name = {"TP": "PTP", "EB": "PEB"}[kind]

        def build(p):
            def one(par):
                s = scenario(name, *LC, 3.3, M_s, 0.8, 5100.0, 0.0, ds.STAR[3], CC if cc else None, "J" if cc else "TESS",
                             qc.size, par)
                self.fused._bound_constants(s.a, M_s, float(p))      # the host's constants of the rate, for this parallax
                return s
            return one

        if plxs is None:
            return self._draw(build(ds.STAR[3] if plx is None else plx), {2: 0.5, 4: 0.5}, qc_in=qc)["lnprior"]
        return np.stack([self._draw(build(p), {2: 0.5, 4: 0.5}, qc_in=qc)["lnprior"] for p in plxs])

    def field(self, kind, idx, cc):
        star = (0.82, 0.8, 5100.0)

        def build(par):
            tail = (TRI, CC if cc else None, "J" if cc else "TESS", idx.size, par)
            return scenario(kind, *(LC + (3.3,) + star + ((0.0,) if kind[0] == "D" else ()) + MAGS + tail))

        o = self._draw(build, {7: idx.astype(np.float64), 2: 0.5, 4: 0.5})
        planet = kind[1:] == "TP"
        return {"frc": o["cols"][9 if planet else 10], "M_host": o["cols"][10 if planet else 13], "lnprior": o["lnprior"],
                "n_field_draw": int(o["scen"].a.n_field_draw)}


# what trx_draw_scenario measured on the GPU against draw_seams.npz, by column (largest over the check's calls; columns
# relative to the column's scale, the prior absolute): the assertion is 8x these, capped by 1e-12 / 1e-9
SEAM_MEASURED = {
    "rp": 1.8e-16, "m": 3.4e-16, "M_host": 2.2e-15, "inc": 1.6e-16, "w": 0.0, "ecc": 1.2e-16, "R_host": 4.2e-16,
    "fr_comp": 2.2e-16, "lnprior": 1.7e-14,
    # lnprior_bound_TP just above log10 P = 3.4 at M_s = 2: its rate there is k4 (0.238095 lp^2 - 0.952381 lp + 0.485714),
    # terms of 2.75 cancelling to 3e-6, times k4 = -0.007: 2e-8, known to 1e-10 of itself whatever evaluates it
    "lnprior_TP over parallax": 7.0e-11,
}


@pytest.mark.parametrize("check", list(ds.CHECKS))
def test_seams_against_the_reference_s_own_values(check):
    """trx_draw_scenario on the fixture's seam-hugging inputs, staged; the answers read off the columns of all draws
    (tests/draw_seams.py says what is compared, tests/golden/make_draw_seams.py how each seam was located).
    Measured on the GPU, largest over each check's calls (columns against the column's scale, the prior absolutely):
      rp 1.8e-16; m = q M_s 3.4e-16; M_host = q_c M_s 2.2e-15 (q_c = exp(20 ln t): pow_pos); inc 1.6e-16; w 0; ecc 1.2e-16;
      R_host 4.2e-16; fr_comp 2.2e-16; M_host of a staged q_c and of a field star 0; lnprior 5.3e-15 (along the
      relations' masses, contrast curve in J), 1.7e-14 (the bound priors; 1.8e-15 without the 2 M_sun host), 0 (field stars; EB over the parallax; TP over
      the parallax at M_s = 0.82, 1.25), 6.9e-11 (TP over the parallax at M_s = 2, just above log10 P = 3.4: see SEAM_MEASURED).
    Every call is staged with `parallel` True and False: the same columns and prior, bit for bit.
    Asserted at 8x these (SEAM_MEASURED), far below the ceilings 1e-12 / 1e-9.
    Nothing differs ACROSS a seam in place: the planet-radius laws at 0.45 M_sun, the mass-radius / temperature branches at
    0.63 M_sun, every knot, clamp and cap, the breaks of the power laws (the uniform that IS a segment's upper edge is in
    each run), delta_mag at 0 without a contrast curve, the five log10 P thresholds by the parallax -- the same values as
    the reference, on the same side.  Where the REFERENCE jumps and the staged number is a dozen rounded operations away
    from the comparison (delta_mag = 0 and the log10 P thresholds along q_companion WITH a contrast curve: -inf | finite
    at log10 P = 1 for EB and 3.4 for TP, branch values 1e-6 apart at 3.4 and 5.5; the lattice's rounding ties), draws of
    the run of adjacent doubles that hugs the seam may take the reference's value of the other side: on the GPU 1-3 draws
    of a run of 18 do at log10 P = 1, 3.4 and 5.5 (at most 6 may: draw_seams.SEAM_PLACES) (as many as for the torch expression on the CPU), one draw of the
    knot and delta_mag = 0 runs (EB, M_s = 1.25 and 2), 10 / 41 of the lattice's tie draws, each within draw_seams.TIE_PLACES
    doubles of its tie by the reference's own Teff / 250 or logg / 0.5 (caps A / B: the reference's B-spline
    evaluation and the kernel's Horner form differ in the last bit of Teff).  No draw with q == 0.95 exactly exists in the runs of 129 adjacent uniforms
    around that seam at M_s = 1, 0.5, 0.25, 0.125 (where m shows q exactly): q = exp(2 ln t) steps by two doubles."""
    from triceratops_amd import _lib
    _lib.require_gpu()
    dev = ds.CHECKS[check](KernelBackend())
    worst = {}
    for k, v in dev.items():
        print("%-72s %.3g" % (k, v))
        if "other side" in k or "exactly" in k or "farthest" in k:
            continue
        col = "lnprior" if k.startswith("lnprior") else k.split("[")[0]
        if "over parallax" in k and "TP" in k:
            col = "lnprior_TP over parallax"
        worst[col] = max(worst.get(col, 0.0), v)
    print("worst by column:", {k: float("%.3g" % v) for k, v in worst.items()})
    for col, v in worst.items():
        assert v <= _bound(SEAM_MEASURED[col], ds.PRIOR_CEILING if col.startswith("lnprior") else ds.COLUMN_CEILING), (col, v)


# ---- 3. the mask boundary, and the fp32 pre-test on it -----------------------------------------------------------------
import draw_boundary as db  # noqa: E402
from test_gpu_fused import _Replay  # noqa: E402


def _kernel_draw(name, star, P, parallel, dump):
    """trx_draw_scenario on staged numbers: every draw's columns and mask(s)"""
    from triceratops_amd import fused
    s = scenario(name, *LC, P, star[0], star[1], star[2], 0.0, dump.shape[1], parallel)
    return staged({"scen": s, "dump": dump}, fused)


def _chain(name, star, P, parallel, dump, pretest):
    """the library's own chain (trx_star_enqueue: fp32 pre-test, mask pass, ordered compaction, fill pass, likelihood,
    evidence, best draw) on the same staged numbers: "numpy-device", fused.TABLE_ROWS = 1, the staged arrays handed out by
    a replay object in the order the scenario asks for them.  Returns the branches' records: [columns of the best draw,
    lnZ, masked count]."""
    import triceratops_amd
    from triceratops_amd import _lib, fused
    from triceratops_amd import device_pipeline as dp
    t = _lib.dev(np.ascontiguousarray(dump), _lib.compute_device())
    order = ([0] if isinstance(P, list) else []) + db.ORDER[name]
    saved = (fused.TABLE_ROWS, fused.PRETEST)
    triceratops_amd.set_sampling("numpy-device")
    saved_rng = dp.RNG
    try:
        dp.RNG, fused.TABLE_ROWS, fused.PRETEST = _Replay(t, order), 1, pretest
        fused.begin_deferred(1)
        p = getattr(fused, "lnZ_" + name)(*LC, P, star[0], star[1], star[2], 0.0, dump.shape[1], parallel)
        assert isinstance(p, fused.Pending) and not p.scen.philox
        fused.flush()
        torch.cuda.synchronize()
        rec = p.out.numpy().copy()
    finally:
        fused.end_deferred()
        dp.RNG = saved_rng
        fused.TABLE_ROWS, fused.PRETEST = saved
        triceratops_amd.set_sampling("numpy")
    W, ncol = p.stride, p.ncol
    assert rec[2 * W] == 0.0
    return [rec[b * W:b * W + ncol + 2] for b in range(1 if name == "TTP" else 2)]


@pytest.mark.parametrize("name,star,parallel,family", db.CONFIGS,
                         ids=["%s-%s-%s-%s" % (c[0], c[1], "vector" if c[2] else "loop", c[3]) for c in db.CONFIGS])
def test_mask_boundary_and_the_fp32_pretest_on_it(name, star, parallel, family):
    """Pass A: seeded numbers through trx_draw_scenario, P_tra / the twin's / the collision margins in 30 digits from its
    columns.  Pass B, one class of offsets per call (tests/draw_boundary.py): the same numbers with one input moved so that
    a comparison of the mask sits at relative offset delta from its boundary -- families: cos i at P_tra (inc, inc_twin);
    P_tra at 1 and size at a (1 - e) by the period (ptra, coll, and the twin's); q around 0.95 (q95); host / companion
    masses inside and just outside the pre-test's `unsure` bands around 0.45 / 0.63 M_sun (mass); e up to the collision at
    25-50 d (high_e).  N = 2000 per call (mass: 600): a partial last pre-test chunk and a partial last share (c).
    (a) the masks equal the 30-digit verdict wherever its relative margin is >= 1e-13; (b) the library's own chain on the
    same staged numbers gives those masked counts with fused.PRETEST on and off, and between the two the same record
    (best draw, lnZ bits, count), the best draw being one of trx_draw_scenario's masked draws bit for bit.
    Measured on the GPU, share of draws left out per class: nearest staged double and its +-1, +-4 neighbours 98.0-100 %
    (their margins are 1e-16 .. 4e-15: only (b) speaks there); every class with |delta| >= 2^-40: 0 %; the q classes: the
    five within 4 doubles of the seam 100 %, the sixteen from 2^14 doubles on 0 %; per family 21.3-23.8 % in all (mass 0 %)."""
    from triceratops_amd import _lib
    _lib.require_gpu()
    planet = name == "TTP"
    total = left = calls = 0
    shares = {}
    for label, spec, star_, P, dump in db.family_calls(family, _kernel_draw, name, star, parallel):
        out = _kernel_draw(name, star_, P, parallel, dump)
        # (a) the masks of trx_draw_scenario against the 30-digit verdict on its own columns
        n, l = db.check_masks(out, planet, parallel, spec, label)
        total, left, calls = total + n, left + l, calls + 1
        shares.setdefault(spec[0], []).append(l / n)
        # (b) the library's own chain on the same numbers, with and without the fp32 pre-test: the masked counts of
        # trx_draw_scenario, and between the two the same lnZ bits and the same best draw
        masks = [out["mask"]] if planet else [out["mask"], out["mask_twin"]]
        recs = {pre: _chain(name, star_, P, parallel, dump, pre) for pre in (True, False)}
        for b, m in enumerate(masks):
            for pre in (True, False):
                assert recs[pre][b][-1] == m.sum(), (label, spec, "branch %d, pre-test %s" % (b, pre), recs[pre][b][-1], int(m.sum()))
            assert recs[True][b].tobytes() == recs[False][b].tobytes(), (label, spec, b)
            if m.sum() and np.isfinite(recs[True][b][-2]):
                # the best draw is one of trx_draw_scenario's masked draws, bit for bit
                ncol = out["cols"].shape[0]
                same = np.all(out["cols"][:, m != 0] == recs[True][b][:ncol, None], axis=0)
                assert same.any(), (label, spec, b)
    print("%s %s %s %s: %d calls of %d draws, left out %.1f %% in all; by class: %s"
          % (name, star, "vector" if parallel else "loop", family, calls, total // calls, 100.0 * left / total,
             {k: "%.1f %%" % (100.0 * np.mean(v)) for k, v in shares.items()}))
    assert left <= 0.25 * total
    assert (total // calls) % 1024 and (total // calls) % 1536          # (c) partial last chunk, partial last share
