"""fused._Dataset's one `term` per kind ("device record"), on T = 12 sorted stamps and a random
[3][12] model grid, with J = 2 candidates and K = 2 columns -- the smallest sizes at which every kind still has
something to pick wrongly.  For each of the eleven key sets of tests/test_dataset_terms_api.py (none, and the ten kinds),
through datasets.validate, the per-key functions and _Dataset.upload:
  the term's type is the tabled one (None for none), and with a one-node t0_grid next to the keys `shift` is set and the
        type is the same;
  with every _lib.chi2_grid_* wrapped by a counter, rec.halfchi2(grid) calls the tabled entry once and no other;
  its result has the bytes of that entry called directly on the system that the datasets.*_system function forms from
        the same dict (the offset's two numbers are formed as its record's docstring says: there is no such function);
  under DATASET_EVALUATION = "fused" _Scenario._datasets_halfchi2 refuses each kind, and a t0_grid, with its full sentence
        before any device work (a stub `self` that carries only `datasets`), and a list of two kinds with the sentence of
        the one that stands first in the order offset, baseline, red_baseline, red_kernel_baseline, red_sigma, red_kernel,
        red_grid, white_grid, t0_grid, outlier_frac."""
import math
import types

import numpy as np
import pytest

from test_dataset_terms_api import KINDS, T, T0, dataset, sequences
from triceratops_amd import _lib, datasets as D, fused

pytestmark = pytest.mark.gpu

ENTRIES = [name for name in dir(_lib) if name.startswith("chi2_grid_")]
NO_RECURRENCE = "the fused kernel carries no recurrence along the row"
# kind: (the term's type, the _lib entry of its reduction, what the fused evaluation says)
TABLE = {
    "none": (None, "chi2_grid_weighted", None),
    "offset": ("_Offset", "chi2_grid_offset", ("an offset_sigma", "the fused kernel carries no sum of w * residual")),
    "baseline": ("_Baseline", "chi2_grid_baseline", ("a baseline", "the fused kernel carries no sums of basis * residual")),
    "ou": ("_Ou", "chi2_grid_ou", ("a red_sigma", NO_RECURRENCE)),
    "ou_mix": ("_OuMix", "chi2_grid_ou_mix", ("a red_grid", NO_RECURRENCE)),
    "ou_lin": ("_OuLin", "chi2_grid_ou_baseline", ("a red_baseline", NO_RECURRENCE)),
    "ss2": ("_Ss2", "chi2_grid_ss2", ("a red_kernel", NO_RECURRENCE)),
    "ss2_lin": ("_Ss2Lin", "chi2_grid_ss2_baseline", ("a red_kernel_baseline", NO_RECURRENCE)),
    "robust": ("_Robust", "chi2_grid_robust", ("an outlier_frac", "the fused kernel carries no exp and log1p per point")),
    "white_mix": ("_WhiteMix", "chi2_grid_white_mix",
                  ("a white_grid", "the fused kernel carries one sum per row, not one per candidate")),
    "white_lin": ("_WhiteLin", "chi2_grid_white_baseline",
                  ("a white_grid", "the fused kernel carries one sum per row, not one per candidate")),
}
T0_SENTENCE = ("a t0_grid", "the nodes' terms are folded from the grid reductions")


def _sentence(what, why):
    return "evaluation='fused' with %s dataset is not built: %s; use evaluation='grid'" % (what, why)


def _upload(keys):
    """(the validated Dataset, its per-key values by Datasets' keywords, its device record)"""
    dicts = [dataset(**keys)]
    sets = D.validate(dicts)
    seq = {k: v[0] for k, v in sequences(dicts, sets).items()}
    rec = fused._Dataset.upload(sets[0], _lib.compute_device(), seq["t0_grids"], seq["outliers"], seq["red_baselines"],
                                seq["white_grids"], seq["white_baselines"], seq["red_kernel_baselines"])
    return sets[0], seq, rec


@pytest.fixture(scope="module")
def grid():
    return _lib.dev(1.0 - 2e-3 * np.random.default_rng(12).random((3, T)))


@pytest.fixture(scope="module")
def uploaded():
    return {kind: _upload(keys) for kind, keys in KINDS.items()}


def _direct(kind, s, seq, grid):
    """the kind's _lib entry on the system formed here from the validated dataset"""
    up = lambda v: _lib.dev(np.ascontiguousarray(v))                                      # noqa: E731
    inv_var = 1.0 / (s.flux_err * s.flux_err)
    y, w = up(s.flux), up(inv_var)
    if kind == "none":
        return _lib.chi2_grid_weighted(y, w, grid)
    if kind == "offset":
        return _lib.chi2_grid_offset(y, w, grid, math.fsum(inv_var.tolist()), 1.0 / (s.offset_sigma * s.offset_sigma))
    if kind == "baseline":
        system = D.baseline_system(s)
        return _lib.chi2_grid_baseline(y, w, grid, up(system.g), system.minv)
    if kind == "ou":
        return _lib.chi2_grid_ou(y, grid, *(up(v) for v in D.ou_system(s)))
    if kind == "ou_mix":
        alpha, beta, omega, lnc = D.ou_mix_system(s)
        return _lib.chi2_grid_ou_mix(y, grid, up(alpha), up(beta), up(omega), lnc)
    if kind == "ou_lin":
        system = D.ou_baseline_system(s, *seq["red_baselines"])
        return _lib.chi2_grid_ou_baseline(y, grid, up(system.alpha), up(system.beta), up(system.omega), up(system.c),
                                          system.minv)
    if kind == "ss2":
        return _lib.chi2_grid_ss2(y, grid, *(up(v) for v in D.ss2_system(s)))
    if kind == "ss2_lin":
        system = D.ss2_baseline_system(s, *seq["red_kernel_baselines"])
        return _lib.chi2_grid_ss2_baseline(y, grid, up(system.A), up(system.g), up(system.omega), up(system.c), system.minv)
    if kind == "robust":
        return _lib.chi2_grid_robust(y, w, grid, *D.robust_constants(*seq["outliers"]))
    if kind == "white_mix":
        wj, lnc = D.white_mix_system(s, seq["white_grids"])
        return _lib.chi2_grid_white_mix(y, grid, up(wj), lnc)
    system = D.white_baseline_system(s, seq["white_grids"], *seq["white_baselines"])
    return _lib.chi2_grid_white_baseline(y, grid, up(system.w), up(system.B), system.minv, system.lnc)


def test_the_table_names_every_kind_and_every_entry():
    assert set(TABLE) == set(KINDS) and len(TABLE) == 11
    assert sorted(ENTRIES) == sorted(entry for _, entry, _ in TABLE.values())


@pytest.mark.parametrize("kind", list(KINDS))
def test_the_term_is_of_the_tabled_type_with_and_without_a_shift(uploaded, kind):
    name = TABLE[kind][0]
    rec = uploaded[kind][2]
    assert rec.shift is None
    assert rec.term is None if name is None else type(rec.term) is getattr(fused, name)
    if kind == "ou_mix":
        return                                  # (validate takes nothing next to a red_grid)
    _, seq, shifted = _upload(dict(KINDS[kind], t0_grid=T0))
    assert type(shifted.shift) is fused._Shift and len(shifted.shift.stamps) == 1
    assert type(shifted.term) is type(rec.term)


@pytest.mark.parametrize("kind", list(KINDS))
def test_halfchi2_makes_the_one_call_of_the_kind_with_the_bytes_of_the_direct_call(monkeypatch, uploaded, grid, kind):
    s, seq, rec = uploaded[kind]
    want = _direct(kind, s, seq, grid).cpu().numpy()
    assert want.shape == (3,) and np.isfinite(want).all()
    calls = []
    for entry in ENTRIES:
        def counted(*a, _name=entry, _real=getattr(_lib, entry), **k):
            calls.append(_name)
            return _real(*a, **k)
        monkeypatch.setattr(_lib, entry, counted)
    got = rec.halfchi2(grid).cpu().numpy()
    assert calls == [TABLE[kind][1]]
    assert got.tobytes() == want.tobytes()


def _refused(records):
    stub = types.SimpleNamespace(datasets=records)
    with fused.switches(DATASET_EVALUATION="fused"):
        with pytest.raises(NotImplementedError) as err:
            fused._Scenario._datasets_halfchi2(stub, None, 0, None)
    return str(err.value)


@pytest.mark.parametrize("kind", [k for k in KINDS if k != "none"] + ["t0_grid"])
def test_the_fused_evaluation_refuses_the_kind_with_its_full_sentence(uploaded, kind):
    plain = uploaded["none"][2]
    if kind == "t0_grid":
        assert _refused([plain, _upload({"t0_grid": T0})[2]]) == _sentence(*T0_SENTENCE)
    else:
        assert _refused([plain, uploaded[kind][2]]) == _sentence(*TABLE[kind][2])


def test_of_two_kinds_the_fused_evaluation_names_the_earlier_of_the_order(uploaded):
    rec = {kind: u[2] for kind, u in uploaded.items()}
    assert _refused([rec["ou"], rec["ou_lin"]]) == _sentence(*TABLE["ou_lin"][2])
    assert _refused([rec["robust"], rec["ss2"], rec["ou_mix"]]) == _sentence(*TABLE["ss2"][2])
    shifted = _upload(dict(KINDS["white_mix"], t0_grid=T0))[2]
    assert _refused([rec["robust"], shifted]) == _sentence(*TABLE["white_mix"][2])
    assert _refused([rec["robust"], _upload({"t0_grid": T0})[2]]) == _sentence(*T0_SENTENCE)
