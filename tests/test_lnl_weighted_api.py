"""The `evaluation` keyword of target.calc_probs_datasets and the fused.DATASET_EVALUATION switch behind it (host
side only: no device is touched)."""
import inspect

import numpy as np
import pytest

from triceratops_amd import _lib, fused, sharding
from triceratops_amd import marginal_likelihoods as ml
from triceratops_amd.triceratops import target

ONE = [{"time": np.linspace(-0.1, 0.1, 7), "flux": np.ones(7), "flux_err": 1e-3}]


def _no_device(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("device work")
    for name in ("require_gpu", "dev", "lnl_batch_weighted", "flux_grid", "chi2_grid_weighted"):
        monkeypatch.setattr(_lib, name, refuse)
    monkeypatch.setattr(sharding, "run_units", refuse)


def test_the_keyword_defaults_to_the_grid_route():
    assert inspect.signature(target.calc_probs_datasets).parameters["evaluation"].default == "grid"
    assert fused.DATASET_EVALUATION == "grid" and fused.DATASET_EVALUATIONS == ("grid", "fused")
    assert "trx_lnl_batch_weighted" in _lib.ABI_SYMBOLS


@pytest.mark.parametrize("bad", ["nope", "", "Fused", None, 1])
def test_an_unknown_evaluation_is_refused_before_any_device_work(monkeypatch, bad):
    _no_device(monkeypatch)
    tg = target.__new__(target)                     # (nothing of the target is looked at before the keyword)
    monkeypatch.setattr(target, "_prepare", lambda *a, **k: pytest.fail("the scenarios were prepared"))
    with pytest.raises(ValueError, match="evaluation"):
        tg.calc_probs_datasets(ONE, 1.0, evaluation=bad)
    assert fused.DATASET_EVALUATION == "grid"


@pytest.mark.parametrize("evaluation", ["grid", "fused"])
def test_the_switch_is_set_for_the_call_and_restored_after_an_exception(monkeypatch, evaluation):
    seen = []

    def run_units(units, **kw):
        seen.append((fused.DATASET_EVALUATION, fused.POSTERIOR_ROWS))
        raise RuntimeError("stop here")

    monkeypatch.setitem(ml._sampling, "mode", "device")
    monkeypatch.setattr(target, "_prepare", lambda self, *a, **k: ([], 0))
    monkeypatch.setattr(sharding, "run_units", run_units)
    tg = target.__new__(target)
    with pytest.raises(RuntimeError, match="stop here"):
        tg.calc_probs_datasets(ONE, 1.0, n_samples=3, evaluation=evaluation)
    assert seen == [(evaluation, 3)]
    assert fused.DATASET_EVALUATION == "grid" and fused.POSTERIOR_ROWS == 0


def test_a_user_setting_of_the_switch_is_refused_where_it_is_read(monkeypatch):
    sc = fused._Scenario.__new__(fused._Scenario)
    with fused.switches(DATASET_EVALUATION="nope"):
        with pytest.raises(ValueError, match="DATASET_EVALUATION"):
            sc._datasets_halfchi2(_lib.MODEL_TP, 0, None)
    assert fused.DATASET_EVALUATION == "grid"
