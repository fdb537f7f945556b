"""trxw_hist_from_halfchi2 (include/trx_warp.h) and target.calc_probs_datasets_refined on the host (DESIGN.md sections 12 and 14): the
export's argument checks and the method's refusals.  No GPU: every check here ends before the first device call."""
import ctypes

import numpy as np
import pandas as pd
import pytest

from triceratops_amd import _lib, fused


def _target():
    from triceratops_amd.triceratops import target
    stars = pd.DataFrame({"ID": [1], "Tmag": [10.0], "Jmag": [9.5], "Hmag": [9.3], "Kmag": [9.2], "ra": [0.0],
                          "dec": [0.0], "mass": [1.0], "rad": [1.0], "Teff": [5777.0], "plx": [10.0],
                          "fluxratio": [1.0], "tdepth": [0.01]})
    return target(1, np.array([1]), stars=stars)


def _ds(n=5):
    return {"time": np.linspace(-0.1, 0.1, n), "flux": np.ones(n), "flux_err": 1e-3}


def _declared():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "trx_warp.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(trxw_[a-z0-9_]+)\s*\(", text)))


def _exports(path):
    import subprocess
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(ln.split()[-1] for ln in out.splitlines() if " T " in ln)


def test_header_library_and_binding_list_the_same_symbols():
    """include/trx_warp.h against both libraries and _lib.WARP_SYMBOLS, as tests/test_abi.py does for include/trx.h:
    the libraries export under trxw_ exactly what the header declares"""
    import __graft_entry__ as g
    g.build()
    assert _declared() == sorted(_lib.WARP_SYMBOLS) == ["trxw_hist_from_halfchi2"]
    for path in (g.LIB, g.LIB_TESTING):
        assert [s for s in _exports(path) if s.startswith("trxw_")] == _declared()
    assert not set(_lib.WARP_SYMBOLS) & set(_lib.ABI_SYMBOLS)


def test_the_export_is_bound_and_the_switch_exists():
    assert hasattr(_lib.lib(), "trxw_hist_from_halfchi2") and callable(_lib.warp_hist_from_halfchi2)
    assert fused.DATASET_WARP_HIST is None
    with fused.switches(DATASET_WARP_HIST={}):
        assert fused.DATASET_WARP_HIST == {}
    assert fused.DATASET_WARP_HIST is None


def test_argument_checks_need_no_gpu():
    """every refusal comes before anything touches a device: the pointers below are not device memory"""
    L = _lib.lib()
    a = fused.DrawArgs()
    a.N, a.use_philox, a.planet, a.seed = 100, 1, 1, 7
    draw = ctypes.addressof(a)
    h = np.zeros(4)
    idx = np.zeros(4, dtype=np.int64)
    out = np.zeros(_lib.WARP_BRANCH, dtype=np.uint64)
    ws = np.zeros(16)
    hp, ip, op, wp = h.ctypes.data, idx.ctypes.data, out.ctypes.data, ws.ctypes.data
    big = L.trx_workspace_bytes()
    ERR_ARG, ERR_WORKSPACE = 1, 3
    f = L.trxw_hist_from_halfchi2
    assert f(None, hp, None, ip, 4, 0.0, op, wp, big, None) == ERR_ARG                 # NULL draw
    assert f(draw, hp, None, ip, 4, 0.0, None, wp, big, None) == ERR_ARG               # NULL out
    assert f(draw, None, None, ip, 4, 0.0, op, wp, big, None) == ERR_ARG               # NULL halfchi2 with n > 0
    assert f(draw, hp, None, None, 4, 0.0, op, wp, big, None) == ERR_ARG               # NULL idx with n > 0
    assert f(draw, hp, None, ip, -1, 0.0, op, wp, big, None) == ERR_ARG                # n < 0
    assert f(draw, hp, None, ip, 2 ** 31, 0.0, op, wp, big, None) == ERR_ARG           # n > 2^31 - 1
    a.use_philox = 0
    assert f(draw, hp, None, ip, 4, 0.0, op, wp, big, None) == ERR_ARG                 # staged uniforms: nothing to recompute
    a.use_philox = 1
    assert f(draw, hp, None, ip, 4, 0.0, op, None, big, None) == ERR_WORKSPACE         # no workspace
    assert f(draw, hp, None, ip, 4, 0.0, op, wp, big - 1, None) == ERR_WORKSPACE       # too small
    assert not out.any()


def test_error_codes_are_the_headers():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "trx.h")).read()
    assert re.search(r"TRX_ERR_ARG\s*=?\s*1\b", text) and re.search(r"TRX_ERR_WORKSPACE\s*=?\s*3\b", text)


def test_refined_datasets_refusals():
    import triceratops_amd as ta
    from triceratops_amd.triceratops import target
    assert hasattr(target, "calc_probs_datasets_refined")
    tg = _target()
    mode = ta.get_sampling()
    try:
        for m in ("numpy", "numpy-device", "device"):
            ta.set_sampling(m)
            with pytest.raises(ValueError):
                tg.calc_probs_datasets_refined([_ds()], 3.0, n_adapt=-1, N=100)
        for m in ("numpy", "numpy-device"):
            ta.set_sampling(m)
            with pytest.raises(NotImplementedError):
                tg.calc_probs_datasets_refined([_ds()], 3.0, N=100)
            with pytest.raises(NotImplementedError):
                tg.calc_probs_datasets_refined([_ds()], 3.0, n_adapt=1, N=100, evaluation="fused")
        # the checks of calc_probs_datasets come first, whatever n_adapt
        ta.set_sampling("device")
        with pytest.raises(ValueError):
            tg.calc_probs_datasets_refined([_ds()], 3.0, evaluation="nope")
        with pytest.raises(TypeError):
            tg.calc_probs_datasets_refined([_ds()], 3.0, exptime=0.02)
        with pytest.raises(ValueError):
            tg.calc_probs_datasets_refined([], 3.0)
    finally:
        ta.set_sampling(mode)
    assert fused.WARP_GRIDS is None and fused.DATASET_WARP_HIST is None and fused.POSTERIOR_ROWS == 0
