"""Shared test helpers: golden loaders and an oracle-backed stand-in for the device calls, so the
host logic (sampling order, masks, priors, tables) can be checked on a CPU-only box.  The
stand-in is test infrastructure: the product has no CPU path."""
import ctypes
import os

import numpy as np
import torch

from oracle import oracle as O

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def gold(name):
    return np.load(os.path.join(GOLD, name), allow_pickle=False)


def install_cpu_device_fakes(monkeypatch):
    """route triceratops_amd._lib's device entry points to the CPU oracle (tests only)"""
    from triceratops_amd import _lib

    def dev(x, device=None):
        if isinstance(x, torch.Tensor):
            return x.to(dtype=torch.float64).contiguous()
        return torch.as_tensor(np.ascontiguousarray(x, dtype=np.float64))

    def lnl_batch(model, flags, t, f, sigma, params, exptime, nsamples, out=None):
        h = O.lnl_batch(model, t.numpy(), f.numpy(), sigma, params.numpy().reshape(params.shape),
                        companion_is_host=bool(flags & 1), exptime=exptime, nsamples=nsamples,
                        scalar_k=bool(flags & 2)) if params.shape[1] else np.empty(0)
        return torch.as_tensor(h)

    def lnz_scenario(model, flags, t, f, sigma, params, exptime, nsamples, lnprior, n_total, lnsigma):
        h = lnl_batch(model, flags, t, f, sigma, params, exptime, nsamples).numpy()
        logw = np.full(n_total, -np.inf)
        lw = -0.5 * np.log(2 * np.pi) - lnsigma - h
        if lnprior is not None:
            lw = lw + lnprior.numpy()
        logw[:h.size] = lw
        return torch.as_tensor(h), torch.tensor([O.log_mean_exp(logw, n_total)], dtype=torch.float64)

    def flux_grid(model, flags, t, params, exptime, nsamples, want_secdepth=True):
        if model == _lib.MODEL_RAW:
            p = params.numpy()
            g = O.evaluate_pv(t.numpy(), p[:7].T, p[7:].T, exptime, nsamples)
            return torch.as_tensor(g), None
        g, s = O.flux_grid(model, t.numpy(), params.numpy(), companion_is_host=bool(flags & 1),
                           exptime=exptime, nsamples=nsamples, scalar_k=bool(flags & 2))
        return torch.as_tensor(g), torch.as_tensor(s)

    def log_mean_exp(x, n_total):
        return torch.tensor([O.log_mean_exp(x.numpy(), n_total)], dtype=torch.float64)

    monkeypatch.setattr(_lib, "dev", dev)
    monkeypatch.setattr(_lib, "lnl_batch", lnl_batch)
    monkeypatch.setattr(_lib, "lnz_scenario", lnz_scenario)
    monkeypatch.setattr(_lib, "flux_grid", flux_grid)
    monkeypatch.setattr(_lib, "log_mean_exp", log_mean_exp)
    monkeypatch.setattr(_lib, "require_gpu", lambda: None)


def call_extra(ml, case, g):
    """invoke one of the four lnZ_* that calc_probs never calls, as make_golden.py did"""
    tri = os.path.join(GOLD, "trilegal_synth.csv")
    b = (g["time"], g["flux"], float(g["sigma"][0]))
    name, variant = case.split("_")
    par = variant != "serial"
    N = 2000 if par else 300
    if name == "NTPu":
        return ml.lnZ_NTP_unknown(*b, 3.3, 30.0 if variant == "empty" else 14.0, tri, N, par)
    if name == "NEBu":
        return ml.lnZ_NEB_unknown(*b, 3.3, 30.0 if variant == "empty" else 14.0, tri, N, par)
    if name == "NTPe":
        return ml.lnZ_NTP_evolved(*b, 3.3, 3.2, 4900.0, 0.0, N, par)
    return ml.lnZ_NEB_evolved(*b, [3.0, 3.6] if par else 3.3, 3.2, 4900.0, 0.0, N, par)


def check_extra(res, case, g, lnz_tol):
    dicts = res if isinstance(res, tuple) else (res,)
    assert len(dicts) == int(g[case + "_nres"][0])
    for i, d in enumerate(dicts):
        assert sorted(d.keys()) == [str(k) for k in g["%s_keys%d" % (case, i)]], (case, i)
        want = g["%s_lnZ%d" % (case, i)][0]
        assert (d["lnZ"] == want) if not np.isfinite(want) else abs(d["lnZ"] - want) < lnz_tol
        key = "%s_logw%d" % (case, i)
        n_fin = min(100, int(np.isfinite(g[key]).sum())) if key in g.files else 1
        for k in d:
            if k == "lnZ":
                continue
            w = g["%s_res%d_%s" % (case, i, k)]
            v = np.atleast_1d(np.asarray(d[k], dtype=float))
            assert v.shape == w.shape
            top = n_fin if v.size > 1 else 1
            assert np.allclose(v[:top], w[:top], rtol=1e-12, atol=0), (case, i, k)


class ZeroRng:
    """stands in for device_pipeline.RNG while a scenario's argument block is built for staged(): every array it hands
    out is replaced there, so it hands out zeros"""

    def uniform(self, n, device):
        return torch.zeros(n, dtype=torch.float64, device=device)

    def beta(self, n, a, b, device):
        return torch.zeros(n, dtype=torch.float64, device=device)

    def randint(self, hi, n, device):
        return torch.zeros(n, dtype=torch.int64, device=device)

    def discard(self, n):
        pass


def scenario(name, *args, **kw):
    """the _Scenario that fused.lnZ_<name>(*args, **kw) builds -- the project's own host constants in its argument
    block -- without running it: what staged() takes as run["scen"]"""
    from triceratops_amd import device_pipeline as dp
    from triceratops_amd import fused
    real, saved = fused._Scenario.run, dp.RNG
    fused._Scenario.run = lambda self, is_host: self
    dp.RNG = ZeroRng()
    try:
        return getattr(fused, "lnZ_" + name)(*args, **kw)
    finally:
        fused._Scenario.run, dp.RNG = real, saved


def staged(run, fused, qc_in=None):
    """trx_draw_scenario on the run's argument block with use_philox = 0 and no map: every random input staged from the
    run's dump ([9][N]: P, q_companion, R_p, inc, q, ecc, argp uniforms, the field-star index, the planets' eccentricity);
    qc_in: the companions' mass ratios themselves ([N], trx_draw_args.qc_in) in place of their uniforms"""
    from triceratops_amd import _lib
    s = run["scen"]
    a, N, dev = s.a, s.N, s.dev
    dump = _lib.dev(np.ascontiguousarray(run["dump"]), dev)
    ncol = 11 if a.planet else 14
    cols = torch.empty((ncol, N), dtype=torch.float64, device=dev)
    mask = torch.empty(N, dtype=torch.uint8, device=dev)
    mask2 = None if a.planet else torch.empty(N, dtype=torch.uint8, device=dev)
    lnprior = torch.empty(N, dtype=torch.float64, device=dev) if a.prior != fused.PRIOR_NONE else None
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    idx = dump[7].to(torch.int64).contiguous()
    a.use_philox, a.warp, a.dump = 0, None, None
    a.uInc, a.uW = dump[3].data_ptr(), dump[6].data_ptr()
    if a.range_P:
        a.uP = dump[0].data_ptr()
    if a.planet:
        a.uRp, a.ecc_in = dump[2].data_ptr(), dump[8].data_ptr()
    else:
        a.uQ, a.uEcc = dump[4].data_ptr(), dump[5].data_ptr()
    qc = None
    if a.comp == fused.COMP_BOUND:
        if qc_in is None:
            a.uQc, a.qc_in = dump[1].data_ptr(), None
        else:
            qc = _lib.dev(np.ascontiguousarray(qc_in, dtype=np.float64), dev)
            a.uQc, a.qc_in = None, qc.data_ptr()
    if a.comp == fused.COMP_FIELD or a.host == fused.HOST_FIELD:
        a.idx = idx.data_ptr()
    a.cols, a.mask, a.mask_twin, a.flag = cols.data_ptr(), mask.data_ptr(), fused._ptr(mask2), flag.data_ptr()
    a.lnprior = fused._ptr(lnprior)
    a.splines = fused._spline_table(dev, s.band).data_ptr()
    with torch.cuda.device(dev):
        torch.cuda.synchronize()
        rc = fused._fn()(ctypes.byref(a), torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize()
    assert rc == 0
    # the map and staged numbers do not go together
    a.warp = dump.data_ptr()
    assert fused._fn()(ctypes.byref(a), torch.cuda.current_stream(dev).cuda_stream) == 1      # TRX_ERR_ARG
    a.warp = None
    return {"cols": cols.cpu().numpy(), "mask": mask.cpu().numpy(), "mask_twin": None if mask2 is None else mask2.cpu().numpy(),
            "lnprior": None if lnprior is None else lnprior.cpu().numpy()}
