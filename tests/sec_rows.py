"""EB rows whose secondary-eclipse verdict (lnL_EB_p, likelihoods.py:535-538: chi^2 = +inf when the secondary eclipse is
deeper than 1.5 sigma) rests on the 25-point scan BY CONSTRUCTION, for tests/test_sec_rows.py (the design, on the oracle
alone) and tests/test_gpu_sec_scan.py (every route of the device against the oracle).  Host only, seeded, no GPU.

On the device the verdict comes from the centre point of the 25 (rowc_kernel<SEC>: deep enough already -> settled) and,
for the rows that leaves open, from sec_scan_kernel<8> over a cross-workgroup list.  Of synth.eb_rows' draws 0.05 % are
excluded by the scan alone, so the suite's 96 .. 300-row likelihood tests hold none of them.

The construction.  The 25-point secondary curve m_j depends on the geometry (R_s / R_EB, P, a, inc, ecc, argp, u1, u2) and
not on EB_fr, and for fixed geometry and comp_fr the depth grows monotonically with EB_fr -- (1 - m) EB_fr without a
companion.  So a geometry whose minimum lies AWAY from the centre point takes its verdict from where EB_fr puts the limit
L = 1.5 synth.SIGMA between the centre depth and the scan depth:

    candidates   synth.eb_rows-like draws with ecc ~ U[0, 0.9], argp ~ U[0, 360), and inc spread around the grazing limit
                 of the SECONDARY conjunction (e_corr with 1 - e sin w; cos i = Ptra U(0.5, 1.05), clipped to 1); rows
                 within 1e-3 of R_EB = R_s are left out (the two k-rules differ there: not this module's subject)
    replay       m_j = O.evaluate_pv at k = R_s / R_EB, t0 = 0, w = (90 - argp + 180) deg, t_j = -0.05 + (0.1 / 24) j with
                 t_24 = 0.05 exactly, no supersampling; depth_of() turns a minimum into the oracle's secdepth by the
                 oracle's own steps, and tests/test_sec_rows.py holds the pair to O.flux_grid's secdepth
    keep         (1 - m_min) >= KEEP_RATIO (1 - m_centre) and (1 - m_min) >= 4 L
    EB_fr        from the oracle's own secdepth: closed form without a companion, bisection on O.flux_grid with one
      scan-excluded   D_min = L f, f = min(sqrt(ratio), 2): the centre depth is L f / ratio <= L / MARGIN, the scan depth
                      >= MARGIN L
      scan-kept       D_min = g L / MARGIN, g in [0.5, 0.999]: open after the quick test, and the scan must leave it finite
    and two plain populations
      centre-excluded EB_fr ~ U(0.3, 0.5) on deep central eclipses (1 - m_centre >= 0.05): settled by the quick test
      faint           EB_fr = 1e-5: open, and kept

KEEP_RATIO is MARGIN^2 = 1.010025 rounded UP, not 1.01: sqrt(1.01) = 1.004988 would leave a row at the threshold 1.2e-5
short of the 0.5 % margin on either side.  The margin is 3.7e-6 in depth against the 5e-13 to which device and oracle
flux agree: no designed verdict hinges on rounding.

Variants: "plain" (no companion), "companion" (comp_fr ~ U(0.01, 0.5), the target is the host), "host" (the same with
companion_is_host, flag 1).  A geometry whose target depth EB_fr < EB_FR_MAX cannot reach is left out of that variant.
"""
import numpy as np

from oracle import oracle as O
from triceratops_amd import synth
from triceratops_amd.constants import G, Msun, Rsun

KINDS = ("scan-excluded", "scan-kept", "centre-excluded", "faint")
OPEN_KINDS = ("scan-excluded", "scan-kept", "faint")
EXCLUDED_KINDS = ("scan-excluded", "centre-excluded")
VARIANTS = {"plain": (False, False), "companion": (True, False), "host": (True, True)}      # (has companion, flag 1)
L = 1.5 * synth.SIGMA
MARGIN = 1.005
KEEP_RATIO = 1.0101
EB_FR_MAX = 0.6
N_POINTS, CENTRE = 25, 12
SEED = synth.SEED + 535
N_CANDIDATES = 40000
PER_KIND = 384                 # geometries per scan-decided kind (the two kinds share them), rows per plain kind


def scan_times():
    """np.linspace(-0.05, 0.05, 25) as the oracle walks it: start + j * step, the end point exact"""
    t = -0.05 + (0.1 / 24.0) * np.arange(N_POINTS, dtype=np.float64)
    t[-1] = 0.05
    return t


def candidates(rng, n):
    """geometry block [11][n] (EB_fr and comp_fr left at 0) in the layout of synth.eb_rows"""
    R_s = rng.uniform(0.3, 2.0, n)
    M_s = rng.uniform(0.3, 2.0, n)
    R_EB = rng.uniform(0.1, 1.0, n) * R_s
    q = rng.uniform(0.1, 0.95, n)
    ecc = rng.uniform(0.0, 0.9, n)
    argp = rng.uniform(0.0, 360.0, n)
    P = rng.uniform(1.0, 30.0, n)
    a = ((G * M_s * (1 + q) * Msun) / (4 * np.pi ** 2) * (P * 86400) ** 2) ** (1 / 3)
    e_corr = (1 - ecc * np.sin(argp * np.pi / 180)) / (1 - ecc ** 2)          # the SECONDARY conjunction
    Ptra = np.clip((R_EB + R_s) * Rsun / a * e_corr, 0.0, 1.0)
    inc = np.degrees(np.arccos(np.minimum(Ptra * rng.uniform(0.5, 1.05, n), 1.0)))
    u1 = rng.uniform(0.1, 0.6, n)
    u2 = rng.uniform(0.05, 0.4, n)
    z = np.zeros(n)
    rows = np.stack([R_EB, z, P, inc, a, R_s, u1, u2, ecc, argp, z])
    return np.ascontiguousarray(rows[:, np.abs(R_EB / R_s - 1.0) >= 1e-3])


def replay(rows):
    """the secondary curve m [n][25] of EB rows [11][n]: likelihoods.py:417-422 on the oracle's evaluate_pv"""
    R_EB, P, inc, a, R_s, u1, u2, ecc, argp = (rows[i] for i in (0, 2, 3, 4, 5, 6, 7, 8, 9))
    pvp = np.stack([R_s / R_EB, np.zeros_like(P), P, a / (R_s * Rsun), inc * (np.pi / 180.0), ecc,
                    (90.0 - argp + 180.0) * (np.pi / 180.0)], axis=1)
    return O.evaluate_pv(scan_times(), pvp, np.stack([u1, u2], axis=1), 0.0, 1)


def depth_of(m, EB_fr, comp_fr, host):
    """the oracle's secdepth from a point (or the minimum) of the secondary curve, step by step as likelihoods.py:399-438
    dilutes it (no closed form is assumed: tests/test_sec_rows.py compares this with O.flux_grid's secdepth)"""
    feb = EB_fr / (1.0 - EB_fr)
    fcomp = comp_fr / (1.0 - comp_fr)
    with np.errstate(divide="ignore", invalid="ignore"):
        y = fcomp / feb if host else 1.0 / feb
        fdil = 1.0 / (fcomp + feb) if host else fcomp / (1.0 + feb)
        sec = (m + y) / (1.0 + y)
        return 1.0 - (sec + fdil) / (1.0 + fdil)


def oracle_depth(rows, host):
    """O.flux_grid's secdepth of rows [11][n] (one stamp: the depth does not depend on the light curve)"""
    return O.flux_grid(O.MODEL_EB, np.zeros(1), rows, companion_is_host=host, exptime=0.0, nsamples=1)[1]


def solve_EB_fr(rows, target, host, above):
    """EB_fr in (0, EB_FR_MAX) at which the oracle's secdepth of each row meets target: the closed form target / (1 - m_min)
    where no row has a companion, else 60 bisections on O.flux_grid, returning the end of the bracket whose depth is >=
    target (above) or <= target (not above).  Second value: the rows whose target lies inside the bracket at all."""
    rows = rows.copy()
    if not rows[10].any():
        fr = target / (1.0 - replay(rows).min(axis=1))
        return fr, (fr > 0.0) & (fr < EB_FR_MAX)
    lo, hi = np.full(rows.shape[1], 1e-9), np.full(rows.shape[1], np.nextafter(EB_FR_MAX, 0.0))

    def depth(fr):
        rows[1] = fr
        return oracle_depth(rows, host)

    ok = (depth(lo) < target) & (depth(hi) > target)
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        up = depth(mid) >= target
        hi, lo = np.where(up, mid, hi), np.where(up, lo, mid)
    return (hi if above else lo), ok


def _pick(argmin, centre_out, n):
    """n of the kept geometries: the rows with the centre point out of eclipse and the rare positions of the minimum first,
    so that every position the candidates reach and both ends of the scan are there at any n"""
    order, taken = [], np.zeros(argmin.size, dtype=bool)
    for i in np.flatnonzero(centre_out)[:32]:
        order.append(i)
        taken[i] = True
    queues = [list(np.flatnonzero((argmin == j) & ~taken)) for j in range(N_POINTS)]
    while len(order) < min(n, argmin.size):
        for qj in queues:
            if qj and len(order) < n:
                order.append(qj.pop(0))
    return np.array(sorted(order[:n]))


_pool = {}


def pool():
    """the geometries, made once per process: `kept` [11][m] with curves `m` [m][25] (minimum away from the centre, at
    least 4 L deep), `deep` [11][PER_KIND] (central eclipses) and `any` [11][PER_KIND] (the first candidates)"""
    if not _pool:
        rng = np.random.default_rng(SEED)
        cand = candidates(rng, N_CANDIDATES)
        m = replay(cand)
        dmin, dcen = 1.0 - m.min(axis=1), 1.0 - m[:, CENTRE]
        keep = np.flatnonzero((dmin >= KEEP_RATIO * dcen) & (dmin >= 4.0 * L))
        deep = np.flatnonzero(dcen >= 0.05)[:PER_KIND]
        _pool.update(kept=np.ascontiguousarray(cand[:, keep]), m=m[keep], n_candidates=cand.shape[1],
                     deep=np.ascontiguousarray(cand[:, deep]), any=np.ascontiguousarray(cand[:, :PER_KIND]),
                     comp_fr=rng.uniform(0.01, 0.5, cand.shape[1]), keep=keep, deep_at=deep,
                     u_kept=rng.uniform(0.5, 0.999, cand.shape[1]), u_deep=rng.uniform(0.3, 0.5, cand.shape[1]))
    return _pool


_blocks = {}


def blocks(variant):
    """the designed rows of a variant, made once per process: {kind: dict(rows [11][n], m [n][25] or None)} and, under
    "host", the variant's companion_is_host"""
    if variant in _blocks:
        return _blocks[variant]
    has_comp, host = VARIANTS[variant]
    p = pool()
    out = {"host": host}

    def with_comp(rows, at):
        rows = rows.copy()
        if has_comp:
            rows[10] = p["comp_fr"][at]
        return rows

    geo, m = with_comp(p["kept"], p["keep"]), p["m"]
    dmin, dcen = 1.0 - m.min(axis=1), 1.0 - m[:, CENTRE]
    with np.errstate(divide="ignore"):
        f = np.minimum(np.sqrt(dmin / dcen), 2.0)
    targets = {"scan-excluded": (L * f, True), "scan-kept": (p["u_kept"][p["keep"]] * L / MARGIN, False)}
    frs, ok = {}, np.ones(geo.shape[1], dtype=bool)
    for kind, (target, above) in targets.items():
        frs[kind], reach = solve_EB_fr(geo, target, host, above)
        ok &= reach
    sel = np.flatnonzero(ok)
    sel = sel[_pick(m[sel].argmin(axis=1), dcen[sel] == 0.0, PER_KIND)]
    for kind in targets:
        rows = geo[:, sel].copy()
        rows[1] = frs[kind][sel]
        out[kind] = dict(rows=np.ascontiguousarray(rows), m=m[sel])
    rows = with_comp(p["deep"], p["deep_at"])
    rows[1] = p["u_deep"][p["deep_at"]]
    out["centre-excluded"] = dict(rows=rows, m=None)
    rows = with_comp(p["any"], np.arange(PER_KIND))
    rows[1] = 1e-5
    out["faint"] = dict(rows=rows, m=None)
    _blocks[variant] = out
    return out


def all_rows(variant):
    """every designed row of the variant as one block [11][n] with its kinds [n] (indices into KINDS)"""
    b = blocks(variant)
    return (np.ascontiguousarray(np.concatenate([b[k]["rows"] for k in KINDS], axis=1)),
            np.concatenate([np.full(b[k]["rows"].shape[1], i) for i, k in enumerate(KINDS)]))


def scan_argmin(variant):
    """per row of all_rows(variant): the position 0 .. 24 of the secondary curve's minimum where the row is scan-decided,
    -1 where it is of a plain kind"""
    b = blocks(variant)
    return np.concatenate([np.full(b[k]["rows"].shape[1], -1) if b[k]["m"] is None else b[k]["m"].argmin(axis=1)
                           for k in KINDS])


def arrange(kinds, n, seed, variant="plain"):
    """n rows of the variant's `kinds`, dealt in turn (every kind is there from n = len(kinds) on, the first alone at n = 1)
    and then shuffled by the seed; a kind's rows are taken in a seeded order and, beyond its block's size, again.
    Returns (rows [11][n], kind [n] as indices into KINDS, at [n]: the row's place in all_rows(variant))."""
    b = blocks(variant)
    rng = np.random.default_rng([SEED, seed, n])
    start = np.cumsum([0] + [b[k]["rows"].shape[1] for k in KINDS])
    kind = np.array([KINDS.index(kinds[i % len(kinds)]) for i in range(n)])
    at = np.empty(n, dtype=np.int64)
    for k in np.unique(kind):
        size = b[KINDS[k]]["rows"].shape[1]
        mine = np.flatnonzero(kind == k)
        at[mine] = start[k] + rng.permutation(size)[np.arange(mine.size) % size]
    order = rng.permutation(n)
    kind, at = kind[order], at[order]
    return np.ascontiguousarray(all_rows(variant)[0][:, at]), kind, at
