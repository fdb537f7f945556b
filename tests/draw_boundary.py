"""The boundary of the draw kernel's geometry mask, constructed on purpose (tests/test_gpu_draw_columns.py, section 3; the
construction itself is proven on the CPU in tests/test_draw_seams_fixture.py).

Pass A: a call's random inputs ([9][N] staged numbers, the layout of fused.DUMP) go through a backend that returns every
draw's columns.  From those columns -- the kernel's own fp64 numbers -- the transit probability P_tra = size / a (1 + e
sin w) / (1 - e^2), the twin's at 2 P_orb and the collision margins are formed in 30-digit arithmetic (mpmath).
Pass B: the same numbers again with ONE input changed so that a comparison of the mask sits at a chosen relative offset
delta from its boundary: cos i = P_tra (1 + delta) through the inclination's uniform; P_tra = 1 + delta or size = a (1 -
e)(1 + delta) through the period's; the mass ratio's uniform a few doubles around q = 0.95.  One class of offsets per
call: the nearest staged double and its +-1 and +-4 neighbours, then +-2^-40 ... +-1e-2.
verdict(): the masks a draw's columns imply, in 30-digit arithmetic wherever fp64 cannot tell (margins below 1e-11), with the smallest
relative margin of the comparisons made -- a mask is asserted where that margin is at least 1e-13 (the columns
themselves are rounded: cos of the rounded inclination returns the staged cosine to 2.5e-15 of P_tra)."""
import mpmath as mp
import numpy as np

from triceratops_amd.constants import Rearth, Rsun

mp.mp.dps = 30
N_DRAWS = 2000                 # neither a multiple of the pre-test's chunk (1024) nor of a workgroup's share (1536)
MARGIN = 1e-13
DELTAS = (2.0 ** -40, 2.0 ** -30, 1e-7, 1e-5, 5e-4, 9e-4, 1.1e-3, 2e-3, 1e-2)
CLASSES = [("place", k) for k in (0, 1, -1, 4, -4)] + [("delta", s * d) for d in DELTAS for s in (1, -1)]
STARS = {"K": (0.82, 0.8, 5100.0), "M": (0.44, 0.43, 3600.0)}
ORDER = {"TTP": [2, 3, 6], "TEB": [3, 4, 5, 6]}          # the slots a scenario's staged arrays are asked for, in order


def step(x, k):
    """the double k places from the positive double x"""
    return float((np.array([x], dtype=np.float64).view(np.int64) + k).view(np.float64)[0])


def base_dump(seed, N=N_DRAWS):
    rng = np.random.default_rng(seed)
    d = rng.random((9, N))
    d[7] = 0.0
    d[8] = rng.beta(0.867, 3.030, N)
    return d


# ---- the geometry of a draw from its columns ---------------------------------------------------------------------------
def _geometry(c, planet, i, f):
    """f: the number type (float or mp.mpf) and its sin / cos"""
    num, sin, cos, pi = f
    if planet:
        rp, inc, a, Rh, e, w = (num(c[k][i]) for k in (0, 2, 3, 4, 7, 8))
        S, S2, a2, q = rp * num(Rearth) + Rh * num(Rsun), None, None, None
    else:
        r, inc, a, Rh, e, w, a2, m, Mh = (num(c[k][i]) for k in (0, 3, 4, 5, 8, 9, 11, 12, 13))
        S, S2, q = (r + Rh) * num(Rsun), 2 * Rh * num(Rsun), m / Mh
    E = (1 + e * sin(w * pi / 180)) / (1 - e * e)
    g = {"S": S, "a": a, "e": e, "E": E, "P1": S / a * E, "ci": cos(inc * pi / 180), "S2": S2, "a2": a2, "q": q}
    g["P2"] = None if planet else S / a2 * E
    return g


_MP = (mp.mpf, mp.sin, mp.cos, mp.pi)


def geometry_mp(cols, planet, i):
    return _geometry(cols, planet, i, _MP)


def _decide(g, planet, parallel):
    """(mask, mask_twin, smallest relative margin) of one draw from its geometry, csrc/trx_draw.hip's rules: a draw transits
    where P_tra <= 1 and cos i <= P_tra (inc >= acos P_tra; no staged inclination is 90 deg), collides where size > a (1 -
    e); the twin branch at 2 P_orb takes q >= 0.95 and, in the per-draw loop's semantics, P_tra <= 1 as well"""
    one = 1
    t1, o1 = abs(g["ci"] - g["P1"]) / g["P1"], abs(g["P1"] - one)
    c1 = abs(g["S"] - g["a"] * (1 - g["e"])) / g["S"]
    hit1 = g["P1"] <= 1 and g["ci"] <= g["P1"]
    coll1 = g["S"] > g["a"] * (1 - g["e"])
    if planet:
        return bool(hit1 and not coll1), False, float(min(t1, o1, c1))
    t2, o2 = abs(g["ci"] - g["P2"]) / g["P2"], abs(g["P2"] - one)
    c2 = abs(g["S2"] - g["a2"] * (1 - g["e"])) / g["S2"]
    qq = abs(g["q"] - 0.95) / 0.95                      # (0.95: the double the kernel compares with, in both arithmetics)
    hit2 = g["P2"] <= 1 and g["ci"] <= g["P2"]
    coll2 = g["S2"] > g["a2"] * (1 - g["e"])
    small = g["q"] < 0.95
    m1 = hit1 and not coll1 and small
    m2 = hit2 and not coll2 and not small and (parallel or g["P1"] <= 1)
    return bool(m1), bool(m2), float(min(t1, o1, c1, t2, o2, c2, qq))


def _decide_np(c, planet, parallel):
    """_decide for all draws at once in fp64 (numpy)"""
    if planet:
        rp, inc, a, Rh, e, w = (c[k] for k in (0, 2, 3, 4, 7, 8))
        S = rp * Rearth + Rh * Rsun
    else:
        r, inc, a, Rh, e, w, a2, m, Mh = (c[k] for k in (0, 3, 4, 5, 8, 9, 11, 12, 13))
        S, S2, q = (r + Rh) * Rsun, 2 * Rh * Rsun, m / Mh
    E = (1 + e * np.sin(w * np.pi / 180)) / (1 - e * e)
    ci, P1 = np.cos(inc * np.pi / 180), S / a * E
    margin = np.minimum(np.minimum(np.abs(ci - P1) / P1, np.abs(P1 - 1)), np.abs(S - a * (1 - e)) / S)
    m1 = (P1 <= 1) & (ci <= P1) & ~(S > a * (1 - e))
    if planet:
        return m1, np.zeros_like(m1), margin
    P2 = S / a2 * E
    for t in (np.abs(ci - P2) / P2, np.abs(P2 - 1), np.abs(S2 - a2 * (1 - e)) / S2, np.abs(q - 0.95) / 0.95):
        margin = np.minimum(margin, t)
    m2 = (P2 <= 1) & (ci <= P2) & ~(S2 > a2 * (1 - e)) & ~(q < 0.95)
    if not parallel:
        m2 = m2 & (P1 <= 1)
    return m1 & (q < 0.95), m2, margin


FP64_SURE, FP64_OUT = 1e-11, 5e-14


def verdict(cols, planet, parallel):
    """(mask, mask_twin, margin) [N].  fp64 evaluates a margin to a few 1e-15 (a dozen roundings of numbers of order one),
    so fp64 decides where it sees at least 1e-11, and a draw whose fp64 margin is below 5e-14 has a 30-digit margin below
    1e-13 whatever its digits: it is left out either way.  Everything between goes through 30 digits."""
    with np.errstate(all="ignore"):
        m1, m2, margin = _decide_np(cols, planet, parallel)
    margin = np.where(np.isnan(margin), 0.0, margin)
    for i in np.flatnonzero((margin < FP64_SURE) & (margin >= FP64_OUT)):
        m1[i], m2[i], margin[i] = _decide(geometry_mp(cols, planet, i), planet, parallel)
    return m1, m2, margin


# ---- pass B: one input moved to the boundary -------------------------------------------------------------------------------
def _delta(spec):
    """the class's relative offset as a 30-digit number (a "place" class aims at the boundary itself and steps from there)"""
    return mp.mpf(spec[1]) if spec[0] == "delta" else mp.mpf(0)


def _placed(x, spec):
    """the staged double for the 30-digit aim x: the nearest double, or for a "place" class the double spec[1] places on"""
    x = float(x)
    return step(x, spec[1]) if (spec[0] == "place" and x > 0) else x


def _set(row, i, x, lo=0.0, hi=np.nextafter(1.0, 0.0)):
    if lo <= x <= hi:
        row[i] = x
        return True
    return False


def inclination_at(dump, geo, spec, branch):
    """cos i = P_tra (1 + delta) of branch 0 (at P_orb) or 1 (the twin, at 2 P_orb): inc = acos(1 - u), so u = 1 - cos i"""
    out = dump.copy()
    grow = 1 + _delta(spec)
    for i, g in enumerate(geo):
        P = g["P2"] if branch else g["P1"]
        if P < 1:
            _set(out[3], i, _placed(1 - P * grow, spec))
    return out


def period_at(dump, geo, spec, branch, P_lo, P_hi, what):
    """the period (staged uniform of a period range) that makes P_tra = 1 + delta (what = "ptra") or size = a (1 - e)
    (1 + delta) (what = "coll") in branch 0 or 1; a ~ P^(2/3), P_tra ~ P^(-2/3).  The inclination: in the "ptra" classes
    the draw's own; in the "coll" classes cos i = P_tra / 2, so that the collision decides"""
    out = dump.copy()
    shrink = (1 + _delta(spec)) ** mp.mpf(-1.5)
    for i, g in enumerate(geo):
        P_A = P_lo + (P_hi - P_lo) * mp.mpf(dump[0][i])
        a_A = g["a2"] if branch else g["a"]
        key = (what, branch)
        if key not in g:                # (P_B(delta) = P_B(0) (1 + delta)^-1.5: the draw's power once, the class's once)
            if what == "ptra":
                g[key] = P_A * (g["P2"] if branch else g["P1"]) ** mp.mpf(1.5)
            else:
                g[key] = P_A * ((g["S2"] if branch else g["S"]) / (1 - g["e"]) / a_A) ** mp.mpf(1.5)
        if _set(out[0], i, _placed((g[key] * shrink - P_lo) / (P_hi - P_lo), spec)) and what == "coll":
            # at the collision boundary P_tra = (1 - e) E of the branch whose sizes collide; the twin's sizes are 2 R_host
            Pt = (1 - g["e"]) * g["E"] * (1 if not branch else g["S"] / g["S2"])
            _set(out[3], i, float(1 - Pt / 2))
    return out


def eccentricity_near_collision(dump, geo, planet, seed):
    """e = 1 - size / a (1 + g), g log-uniform in [1e-3, 0.3]: the largest eccentricities at which the draw does not
    collide -- where 1 - e^2 cancels in fp32.  Planets: the staged eccentricity itself; binaries: u = e^0.6 (P_orb > 10 d)"""
    rng = np.random.default_rng(seed)
    out = dump.copy()
    gap = 10.0 ** rng.uniform(-3.0, np.log10(0.3), len(geo))
    for i, g in enumerate(geo):
        e = float(1 - g["S"] / g["a"] * (1 + gap[i]))
        if 0.0 < e < 1.0:
            out[8 if planet else 5][i] = e if planet else e ** 0.6
    return out


def uniform_where(fn, level, lo=0.0, hi=np.nextafter(1.0, 0.0)):
    """the smallest double x in [lo, hi] with fn(x) >= level (fn monotonic), by bisection"""
    assert fn(lo) < level <= fn(hi)
    while True:
        mid = lo + 0.5 * (hi - lo)
        if mid <= lo or mid >= hi:
            return hi
        if fn(mid) >= level:
            hi = mid
        else:
            lo = mid


# ---- the torch expression of the chain as a stand-in for the columns (CPU) ---------------------------------------------
def torch_columns(name, star, P, parallel, dump):
    """the columns and masks of lnZ_TTP / lnZ_TEB from staged numbers: tests/torch_pipeline.py's primitives on CPU tensors"""
    import torch
    import torch_pipeline as tp
    M_s, R_s, Teff = star
    N = dump.shape[1]
    T = lambda v: torch.as_tensor(np.ascontiguousarray(v, dtype=np.float64))
    Pd = T(np.full(N, P)) if np.isscalar(P) else P[0] + (P[1] - P[0]) * T(dump[0])
    inc, w = tp.sample_inc(T(dump[3])), T(dump[6]) * 360.0
    if name == "TTP":
        rp = tp.sample_rp(T(dump[2]), T(np.full(N, M_s)), False)
        a = tp._sma(M_s, Pd)
        z = torch.zeros(N, dtype=torch.float64)
        cols = [rp, Pd, inc, a, z + R_s, z, z, T(dump[8]), w, z, z + M_s]
    else:
        P_mean = P if np.isscalar(P) else float(Pd.mean())
        q = tp.sample_q(T(dump[4]), M_s)
        m = q * M_s
        r, _ = tp.stellar_relations(m, T(np.full(N, R_s)), T(np.full(N, Teff)))
        ecc = T(dump[5]) ** (1.0 / (0.2 if P_mean <= 10 else 0.6))
        z = torch.zeros(N, dtype=torch.float64)
        cols = [r, z, Pd, inc, tp._sma(M_s + m, Pd), z + R_s, z, z, ecc, w, z, tp._sma(M_s + m, 2 * Pd), m, z + M_s]
    cols = torch.stack(cols)
    # the masks of marginal_likelihoods.py:111-123 in fp64, independent of verdict() above
    e, sinw = cols[7 if name == "TTP" else 8], torch.sin(w * np.pi / 180)
    E = (1 + e * sinw) / (1 - e ** 2)
    if name == "TTP":
        S = cols[0] * Rearth + R_s * Rsun
        mask = tp._transits(S / cols[3] * E, inc, parallel) & ~(S > cols[3] * (1 - e))
        return {"cols": cols.numpy(), "mask": mask.numpy().astype(np.uint8), "mask_twin": None}
    S = (cols[0] + R_s) * Rsun
    P1, P2 = S / cols[4] * E, S / cols[11] * E
    m1 = tp._transits(P1, inc, parallel) & ~(S > cols[4] * (1 - e)) & (q < 0.95)
    m2 = tp._transits(P2, inc, parallel) & ~(2 * R_s * Rsun > cols[11] * (1 - e)) & (q >= 0.95)
    if not parallel:
        m2 = m2 & (P1 <= 1.0)
    return {"cols": cols.numpy(), "mask": m1.numpy().astype(np.uint8), "mask_twin": m2.numpy().astype(np.uint8)}


# ---- the families of classes ------------------------------------------------------------------------------------------
FAMILIES = ("inc", "inc_twin", "ptra", "ptra_twin", "coll", "coll_twin", "q95", "mass", "high_e", "high_e_twin")
Q_PLACES = (0, 1, -1, 4, -4) + tuple(s * 2 ** k for k in (14, 16, 20, 24, 28, 32, 36, 40) for s in (1, -1))
MASS_OFFSETS = (("place", 0), ("place", 1), ("place", -1)) + tuple(("offset", s * d) for d in (0.5e-4, 0.99e-4, 1.01e-4, 2e-4)
                                                                  for s in (1, -1))
MASS_CLASSES = [("delta", s * d) for d in (1e-7, 9e-4, 1.1e-3) for s in (1, -1)]
P_SHORT, P_LONG = (0.01, 5.0), (25.0, 50.0)


def applies(family, name, star_key):
    """the twin's classes and q = 0.95 need a binary; the planet-radius switch a host next to 0.45 M_sun (the M dwarf's
    mass is moved there); the mass-radius switch a companion that reaches 0.63 M_sun (the K dwarf's)"""
    planet = name == "TTP"
    if family.endswith("_twin") or family == "q95":
        return not planet
    if family == "mass":
        return (planet and star_key == "M") or (not planet and star_key == "K")
    return True


# (name, star, parallel, family): planets and binaries, a K and an M dwarf, the vector path's semantics and the per-draw
# loop's
CONFIGS = [(name, star, parallel, family) for name in ("TTP", "TEB") for star in ("K", "M") for parallel in (True, False)
           for family in FAMILIES if applies(family, name, star)]


def must_decide(spec):
    """classes none of whose draws may be left out: every offset of at least 2^-40 (for the q classes: 2^14 doubles of
    the uniform, 3e-13 of q)"""
    return spec[0] == "delta" or (spec[0] == "q" and abs(spec[1]) >= 2 ** 14)


def family_draws(family):
    """draws per call: 2000, neither a multiple of the pre-test's chunk (1024) nor of a workgroup's share (1536); the
    "mass" family, eleven first passes, 600: one partial chunk"""
    return 600 if family == "mass" else N_DRAWS


def family_calls(family, draw, name, star_key, parallel, N=None, seed=20260117):
    """yields (label, spec, star, P, dump) for every class of a family: what pass B stages.  draw(name, star, P, parallel,
    dump) -> {"cols", "mask", "mask_twin"} is the backend (pass A goes through it too)."""
    from triceratops_amd import priors
    planet = name == "TTP"
    star = STARS[star_key]
    assert applies(family, name, star_key)
    twin = family.endswith("_twin")
    family, b = family.replace("_twin", ""), int(twin)

    def geometry(star_, P, dump):
        cols = draw(name, star_, P, parallel, dump)["cols"]
        return [geometry_mp(cols, planet, i) for i in range(cols.shape[1])]

    base = base_dump(seed, family_draws(family) if N is None else N)
    if family == "inc":
        geo = geometry(star, 3.3, base)
        for spec in CLASSES:
            yield "cos i at P_tra of branch %d" % b, spec, star, 3.3, inclination_at(base, geo, spec, b)
    elif family in ("ptra", "coll"):
        geo = geometry(star, list(P_SHORT), base)
        for spec in CLASSES:
            yield ("%s of branch %d by the period" % ("P_tra at 1" if family == "ptra" else "the collision", b), spec, star,
                   list(P_SHORT), period_at(base, geo, spec, b, P_SHORT[0], P_SHORT[1], family))
    elif family == "q95":
        x = uniform_where(lambda u: priors.sample_q(np.array([u]), star[0])[0], 0.95)
        base[4] = x
        geo = geometry(star, 3.3, base)
        for i, g in enumerate(geo):                     # every draw transits at P_orb and at 2 P_orb: q decides
            _set(base[3], i, float(1 - g["P2"] / 2))
        for k in Q_PLACES:
            d = base.copy()
            d[4] = step(x, k)
            yield "q at 0.95", ("q", k), star, 3.3, d
    elif family == "mass":
        for kind, v in MASS_OFFSETS:
            at = 0.45 if planet else 0.63
            target = step(at, v) if kind == "place" else at + v
            d0, star_ = base.copy(), star
            if planet:
                star_ = (target,) + star[1:]
            else:
                d0[4] = uniform_where(lambda u: priors.sample_q(np.array([u]), star[0])[0] * star[0], target)
            geo = geometry(star_, 3.3, d0)
            for spec in MASS_CLASSES:
                yield ("%s mass %s %g from %g" % ("host" if planet else "companion", kind, v, at), spec, star_, 3.3,
                       inclination_at(d0, geo, spec, 0))
    elif family == "high_e":
        geo = geometry(star, list(P_LONG), base)
        d1 = eccentricity_near_collision(base, geo, planet, seed + 1)
        geo = geometry(star, list(P_LONG), d1)
        for spec in CLASSES:
            yield "cos i at P_tra of branch %d, e next to the collision" % b, spec, star, list(P_LONG), inclination_at(d1, geo, spec, b)


def check_masks(out, planet, parallel, spec, label):
    """(a): the masks equal the 30-digit verdict wherever its margin is at least 1e-13.  Returns (draws, draws left out)."""
    m1, m2, margin = verdict(out["cols"], planet, parallel)
    sure = margin >= MARGIN
    bad = np.flatnonzero(sure & ((out["mask"] != 0) != m1))
    assert bad.size == 0, (label, spec, "mask", bad[:5], margin[bad[:5]])
    if not planet:
        bad = np.flatnonzero(sure & ((out["mask_twin"] != 0) != m2))
        assert bad.size == 0, (label, spec, "mask_twin", bad[:5], margin[bad[:5]])
    left = int((~sure).sum())
    if must_decide(spec):
        assert left == 0, (label, spec, "draws left out", left)
    return sure.size, left
