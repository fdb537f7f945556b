"""tests/golden/draw_seams.npz and the comparison code of tests/draw_seams.py, proven on the CPU before any GPU time is
spent on them: the torch expression of the draw chain (tests/torch_pipeline.py) stands in for the kernel's columns, and
the package's host priors / funcs are held to the same fixture, seam by seam.  The GPU half is
tests/test_gpu_draw_columns.py."""
import os

import numpy as np
import pytest
import torch

import draw_seams as ds
import torch_pipeline as dp
from helpers import GOLD
from triceratops_amd import funcs, priors
from triceratops_amd.constants import G, Msun, Rsun

S = ds.S
CC = os.path.join(GOLD, "contrast_curve_synth.csv")
TRI = os.path.join(GOLD, "trilegal_synth.csv")


def T(a):
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64))


class TorchBackend:
    """tests/torch_pipeline.py's primitives on CPU tensors, combined the way csrc/trx_draw.hip combines them"""

    def rp(self, x, M_s, flat):
        return dp.sample_rp(T(x), T(np.full(x.size, M_s)), flat).numpy()

    def q(self, x, M_s):
        q = dp.sample_q(T(x), M_s).numpy()
        return q * M_s, (q < 0.95).astype(np.uint8), (q >= 0.95).astype(np.uint8)

    def qc(self, x, M_s, parallel):
        return dp.sample_q_companion(T(x), M_s).numpy() * M_s

    def angles(self, x):
        return dp.sample_inc(T(x)).numpy(), x * 360.0

    def ecc(self, u, P_orb):
        return u ** (1.0 / (0.2 if P_orb <= 10 else 0.6))

    def relations(self, M, max_R, max_T, cc):
        m = T(M)
        R, Te = dp.stellar_relations(m, T(np.full(M.size, max_R)), T(np.full(M.size, max_T)))
        logg = torch.log10(G * (m * Msun) / (R * Rsun) ** 2)
        ig = torch.clamp(torch.round(logg / 0.5) * 0.5, 3.5, 5.0).numpy()
        it = torch.clamp(torch.round(Te / 250) * 250, 3500, 10000).numpy()
        u1, u2 = np.full(M.size, np.nan), np.full(M.size, np.nan)
        for tag in ds.CAPS:          # the lattice's cells by their (Teff, logg): the fixture's own table of them
            for t_, g_, a_, b_ in zip(S["rel_cellT_" + tag], S["rel_cellg_" + tag], S["rel_u1_" + tag], S["rel_u2_" + tag]):
                sel = (it == t_) & (ig == g_)
                u1[sel], u2[sel] = a_, b_
        return {"R_host": R.numpy(), "M_host": M * 1.0, "frc": dp._flux_share(m, 1.0).numpy(), "u1": u1, "u2": u2,
                "lnprior": self.prior("TP", 1.0, ds.STAR[3], M, cc)}

    def prior(self, kind, M_s, plx, qc, cc, plxs=None):
        if plxs is not None:
            return np.stack([self.prior(kind, M_s, float(p), qc, cc) for p in plxs])
        fr = dp._flux_share(T(qc * M_s), M_s, "J" if cc else "TESS")
        dm = 2.5 * torch.log10(fr / (1 - fr))
        seps, cons = (S["cc_seps"], S["cc_cons"]) if cc else (np.array([2.2]), np.array([1.0]))
        return dp._clip_prior(dp._bound_rate(M_s, plx, dm.abs(), seps, cons, kind == "EB"), dm).numpy()

    def field(self, kind, idx, cc):
        from triceratops_amd import marginal_likelihoods as ml
        f = ml._Field(TRI, 10.4, 9.5, 9.1, 9.0)
        n = f.N_comp
        delta = f.dJ if cc else f.dT
        if cc:
            lp = priors.lnprior_background(n, np.abs(delta[idx]), S["cc_seps"], S["cc_cons"])
        else:
            lp = np.full(idx.size, np.log((n / 0.1) * (1 / 3600) ** 2 * 2.2 ** 2))
            fr = f.fluxratios[idx]
            delta = np.empty(n)
            delta[idx] = 2.5 * np.log10(fr / (1 - fr))
        lp = np.where(delta[idx] > 0.0, -np.inf, np.minimum(lp, 0.0))
        return {"frc": f.fluxratios[idx], "M_host": f.masses[idx], "lnprior": lp,
                "n_field_draw": n - 1 if kind[0] == "D" else n}


@pytest.mark.parametrize("check", list(ds.CHECKS))
def test_torch_expression_of_the_chain_on_the_seams(check):
    dev = ds.CHECKS[check](TorchBackend())
    for k, v in dev.items():
        print("%-70s %.3g" % (k, v))
        if "other side" in k or "exactly" in k or "farthest" in k:
            continue
        assert v <= (ds.PRIOR_CEILING if "lnprior" in k else ds.COLUMN_CEILING), (k, v)


def test_fixture_hugs_its_seams():
    """what the generator promises: adjacent doubles on both sides of every seam, and outputs that differ across it"""
    # the switch of the planet-radius laws and of the mass-radius relation
    assert S["rp_M"][1] <= 0.45 < S["rp_M"][2]
    M, R = S["rel_M"], S["rel_R_B"]
    i = int(np.searchsorted(M[:-1], 0.63))
    assert M[i] == 0.63 and np.nextafter(M[i], 1.0) == M[i + 1] and R[i + 1] - R[i] > 0.04 and abs(R[i] - 0.6) < 1e-12
    assert np.isnan(M[-1]) and S["rel_R_B"][-1] == 0.1 and S["rel_T_B"][-1] == 2800.0
    # clamps and caps act on some masses and not on their neighbours
    for tag, (cap_R, cap_T) in ds.CAPS.items():
        assert (S["rel_R_" + tag] == 0.1).any() and (S["rel_T_" + tag] == 2800.0).any()
    assert (S["rel_R_A"] == 0.8).any() and (S["rel_R_A"] < 0.8).any() and (S["rel_T_A"] == 5100.0).any()
    assert not (S["rel_R_B"] == 20.0).any()
    # every tie's run holds both cells
    for k in range(int(S["rel_tie"].max()) + 1):
        sel = S["rel_tie"] == k
        assert sel.sum() >= 8
        cells = {(t, g) for t, g in zip(S["rel_cellT_B"][sel], S["rel_cellg_B"][sel])}
        assert len(cells) == 2, (k, cells)
    # the samplers' breaks: outputs on both sides of 3 and 6 R_earth, of q = 0.3 and 0.95
    for i in range(4):
        r = S["rp_out"][i]
        assert (r <= 3.0).any() and (r > 3.0).any() and (r <= 6.0).any() and (r > 6.0).any()
    for i, M_s in enumerate(S["q_M"]):
        if 0.1 / M_s < 0.95:              # (below that the law has no room under 0.95: q_min = 0.1 / M_s)
            for out in (S["q_out%d" % i], S["qc_out%d" % i]):
                assert (out < 0.95).any() and (out >= 0.95).any()
    # delta_mag on both sides of 0, the contrast curve's knots and ends, the thresholds of log10 P
    for im in range(S["prior_M"].size):
        for tag in ("nocc", "ccJ"):
            dm = S["prior_%d_%s_dm" % (im, tag)]
            assert (dm > 0).any() and (dm < 0).any()
        dm = np.abs(S["prior_%d_ccJ_dm" % im])
        cons = S["cc_cons"]
        assert (dm < cons[0]).any()
        hugged = [bool((dm <= c).any() and (dm > c).any() and np.min(np.abs(dm - c)) < 1e-13) for c in cons]
        # a 0.1 M_sun companion is 6.1 mag fainter than the 0.82 M_sun host in J and 7.8 mag than the 1.25 M_sun one: they
        # reach 11 and 34 of the curve's 40 knots (the last is at 7.95 mag).  The 2 M_sun host reaches all, and both ends
        assert sum(hugged) == (11, 34, 40)[im] and all(hugged[:sum(hugged)]), (im, hugged)
        if im == 2:
            assert (dm > cons[-1]).any() and (dm < cons[0]).any()
        for kind in ("TP", "EB"):
            v = S["plx_%d_%s" % (im, kind)]
            assert np.isneginf(v).any() and np.isfinite(v).any()


def test_host_functions_on_the_seams():
    """the package's numpy priors / funcs (bit-identical to the reference on random inputs: tests/test_host.py) on the
    fixture's seam-hugging inputs: the same bits there too"""
    x = S["rp_x"]
    for i, M in enumerate(S["rp_M"]):
        assert np.array_equal(priors.sample_rp(x.copy(), np.full(x.size, M), False), S["rp_out"][i])
    assert np.array_equal(priors.sample_rp(x.copy(), np.full(x.size, 0.82), True), S["rp_flat"])
    for i, M in enumerate(S["q_M"]):
        x = S["q_x%d" % i]
        assert np.array_equal(priors.sample_q(x.copy(), float(M)), S["q_out%d" % i])
        assert np.array_equal(priors.sample_q_companion(x.copy(), float(M)), S["qc_out%d" % i])
    assert np.array_equal(priors.sample_inc(S["ang_x"].copy()), S["inc_out"])
    assert np.array_equal(priors.sample_w(S["ang_x"].copy()), S["w_out"])
    for P, want in zip(S["ecc_P"], S["ecc_out"]):
        np.random.seed(31)
        assert np.array_equal(priors.sample_ecc(np.zeros(96), False, float(P)), want)
    M = S["rel_M"]
    for tag, (cap_R, cap_T) in ds.CAPS.items():
        R, Te = funcs.stellar_relations(M.copy(), np.full(M.size, cap_R), np.full(M.size, cap_T))
        assert np.array_equal(R, S["rel_R_" + tag]) and np.array_equal(Te, S["rel_T_" + tag])
    for band in ("TESS", "J", "H", "K"):
        with np.errstate(all="ignore"):
            assert np.array_equal(funcs.flux_relation(M.copy(), band), S["flux_" + band], equal_nan=True)
    seps, cons = funcs.file_to_contrast_curve(CC)
    assert np.array_equal(seps, S["cc_seps"]) and np.array_equal(cons, S["cc_cons"])
    n = int(S["field_n"][0])
    assert np.array_equal(priors.lnprior_background(n, S["bg_dm"].copy(), seps, cons), S["bg_out"])
    for im, Ms in enumerate(S["prior_M"]):
        for tag, cc in (("nocc", (np.array([2.2]), np.array([1.0]))), ("ccJ", (seps, cons))):
            key = "prior_%d_%s" % (im, tag)
            dm = S[key + "_dm"]
            for kind, fn in (("TP", priors.lnprior_bound_TP), ("EB", priors.lnprior_bound_EB)):
                with np.errstate(all="ignore"):
                    lp = fn(float(Ms), ds.STAR[3], np.abs(dm), *cc)
                lp = np.where(dm > 0.0, -np.inf, np.where(lp > 0.0, 0.0, lp))
                assert np.array_equal(lp, S[key + "_" + kind], equal_nan=True), (key, kind)


import draw_boundary as db  # noqa: E402


@pytest.mark.parametrize("name,star,family", [c[:2] + c[3:] for c in db.CONFIGS if c[2] and c[:2] in (("TTP", "M"), ("TEB", "K"))])
def test_boundary_construction_stays_inside_its_conditions(name, star, family):
    """tests/draw_boundary.py with the torch expression of the chain standing in for the kernel's columns: every class of
    offsets lands where it is meant to -- no draw of a class with |delta| >= 2^-40 is left without a 30-digit verdict, at
    most a quarter of a family's draws are left out in all -- and the 30-digit verdict agrees with torch_pipeline's own
    fp64 masks wherever it claims to be sure.  (N = 200 here: the construction does not depend on N.)"""
    planet, total, left, moved = name == "TTP", 0, 0, 0
    base = db.base_dump(20260117, 200)
    for parallel in ((True, False) if family in ("inc", "inc_twin", "ptra_twin") else (True,)):
        for label, spec, star_, P, dump in db.family_calls(family, db.torch_columns, name, star, parallel, N=200):
            out = db.torch_columns(name, star_, P, parallel, dump)
            n, l = db.check_masks(out, planet, parallel, spec, label)
            total, left = total + n, left + l
            moved += int((dump != base).any(axis=0).sum())
    print("%s %s %s: %d draws, %d left out (%.1f %%), %d moved" % (name, star, family, total, left, 100.0 * left / total, moved))
    assert left <= 0.25 * total and moved >= 0.5 * total
