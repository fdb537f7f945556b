"""The plumbing between a dataset's keys and what calc_probs_datasets reports ("device record"),
without a GPU: every sentence with which target._datasets_pass refuses evaluation='fused', in full and in its order, and
target._scatter_best -- the one loop that turns what a DATASET_* switch collected into an attribute's rows -- on designed
input.  KINDS (one key set per kind of term, T = 12 points, J = 2 candidates, K = 2 columns) also serves
tests/test_gpu_dataset_terms.py."""
import numpy as np
import pytest

from test_datasets_api import _target
from triceratops_amd import datasets as D
from triceratops_amd.sharding import Unit

T = 12
TIME = np.linspace(-0.1, 0.1, T)
COLS = np.stack([np.ones(T), np.linspace(-1.0, 1.0, T)])
OU = {"red_sigma": 2e-3, "red_timescale": 0.05}
M32 = dict(OU, red_kernel="matern32")
WHITE = [(1.0, 0.0, 1.0), (1.5, 5e-4, 3.0)]
T0 = [(0.0, 1.0)]
KINDS = {
    "none": {},
    "offset": {"offset_sigma": 1e-3},
    "baseline": {"baseline": COLS, "baseline_sigma": 1e-2},
    "ou": OU,
    "ou_mix": {"red_grid": [(2e-3, 0.05, 1.0), (1e-3, 0.5, 3.0)]},
    "ou_lin": dict(OU, red_baseline=COLS, red_baseline_sigma=1e-2),
    "ss2": M32,
    "ss2_lin": dict(M32, red_kernel_baseline=COLS, red_kernel_baseline_sigma=1e-2),
    "robust": {"outlier_frac": 0.05, "outlier_scale": 5.0},
    "white_mix": {"white_grid": WHITE},
    "white_lin": {"white_grid": WHITE, "white_baseline": COLS, "white_baseline_sigma": 1e-2},
}


def dataset(**keys):
    flux = 1.0 - 1e-3 * np.exp(-0.5 * (TIME / 0.03) ** 2)
    return dict({"time": TIME.copy(), "flux": flux, "flux_err": np.linspace(8e-4, 1.2e-3, T)}, **keys)


def sequences(dicts, sets):
    """Datasets' per-dataset sequences, by its keywords, as target._datasets_args forms them"""
    return {"t0_grids": D.t0_grids(dicts, sets), "outliers": D.outliers(dicts, sets),
            "red_baselines": D.red_baselines(dicts, sets), "white_grids": D.white_grids(dicts, sets),
            "white_baselines": D.white_baselines(dicts, sets),
            "red_kernel_baselines": D.red_kernel_baselines(dicts, sets)}


def _datasets(dicts, only=None):
    sets = D.validate(dicts)
    seqs = sequences(dicts, sets)
    return D.Datasets(sets, **{k: v for k, v in seqs.items() if only is None or k in only})


def _sentence(what):
    return "evaluation='fused' with %s dataset is not built: use evaluation='grid'" % what


# (the keys of dataset 1, the Datasets sequences kept -- None: all --, the wording).  A validated white_baseline stands next
# to a white_grid, whose sentence comes first: its own is reached by a Datasets that carries the columns alone.
REFUSALS = [
    (KINDS["offset"], None, "an offset_sigma"),
    (KINDS["baseline"], None, "a baseline"),
    (KINDS["ou_lin"], None, "a red_baseline"),
    (KINDS["ss2_lin"], None, "a red_kernel_baseline"),
    (KINDS["ou"], None, "a red_sigma or red_grid"),
    (KINDS["ou_mix"], None, "a red_sigma or red_grid"),
    ({"t0_grid": T0}, None, "a t0_grid"),
    (KINDS["white_mix"], None, "a white_grid"),
    (KINDS["white_lin"], ("white_baselines",), "a white_baseline"),
    (KINDS["robust"], None, "an outlier_frac"),
]


@pytest.fixture
def tg(monkeypatch):
    """a target whose preparation (priors, TRILEGAL) -- not what is under test -- is stubbed: no unit, no device call"""
    from triceratops_amd.triceratops import target
    monkeypatch.setattr(target, "_prepare", lambda self, *a, **k: ([], 0))
    return _target()


@pytest.mark.parametrize("keys, only, what", REFUSALS, ids=[r[2].split()[-1] + str(i) for i, r in enumerate(REFUSALS)])
def test_datasets_pass_refuses_the_fused_evaluation_with_the_full_sentence(tg, keys, only, what):
    ds = _datasets([dataset(), dataset(**keys)], only)
    with pytest.raises(NotImplementedError) as err:
        tg._datasets_pass(ds, 3.0, {}, 0, "fused")
    assert str(err.value) == _sentence(what)
    assert tg._datasets_pass(ds, 3.0, {}, 0, "grid") == ([], [], 0)        # (the grid evaluation takes every one of them)


def test_of_two_kinds_in_a_list_the_earlier_of_the_order_is_named(tg):
    ds = _datasets([dataset(**KINDS["robust"]), dataset(**KINDS["white_mix"]), dataset(**KINDS["ou_lin"])])
    with pytest.raises(NotImplementedError) as err:
        tg._datasets_pass(ds, 3.0, {}, 0, "fused")
    assert str(err.value) == _sentence("a red_baseline")
    ds = _datasets([dataset(**KINDS["robust"]), dataset(t0_grid=T0, **KINDS["white_mix"])])
    with pytest.raises(NotImplementedError) as err:
        tg._datasets_pass(ds, 3.0, {}, 0, "fused")
    assert str(err.value) == _sentence("a t0_grid")


# ---------------------------------------------------------------------------------------
# target._scatter_best: three scenario rows in two work units.  Unit 0 (row 0) left nothing in the switch's dict; unit 1
# (rows 1 and 2, star 1 of the job: share 0.25) left both branches, and row 1 has lnZ = -inf.
UNITS = [Unit(0, ("TP",), 1, 1, None, "TP", group=(0, 0)), Unit(1, ("EB", "EBx2P"), 1, 1, None, "EB", group=(0, 1))]
SHARE = np.array([1.0, 0.25])


def _scatter(best, blank, fill):
    tg = _target()
    tg.lnZ = np.array([-3.0, -np.inf, -5.0])
    return tg._scatter_best(UNITS, best, blank, fill)


def test_scatter_best_with_a_coefficient_style_fill():
    best = {1: [[None, np.array([2.0, 4.0])], [None, np.array([8.0, -16.0])]]}
    rows = _scatter(best, lambda: [None, np.full(2, np.nan)],
                    lambda u, per: [None if c is None else c * SHARE[u.group[1]] for c in per])
    assert len(rows) == 3
    for r in rows[:2]:                                                      # no entry; no finite lnZ
        assert r[0] is None and r[1].shape == (2,) and np.isnan(r[1]).all()
    assert rows[0][1] is not rows[1][1]                                     # (a blank row of its own per scenario)
    assert rows[2][0] is None and rows[2][1].tobytes() == np.array([2.0, -4.0]).tobytes()
    # an [L] array per branch, as DATASET_OFFSETS holds
    rows = _scatter({1: [np.array([1.0, np.nan]), np.array([4.0, np.nan])]}, lambda: np.full(2, np.nan),
                    lambda u, c: c * SHARE[u.group[1]])
    assert np.array(rows).tobytes() == np.array([[np.nan, np.nan], [np.nan, np.nan], [1.0, np.nan]]).tobytes()


def test_scatter_best_with_a_dict_style_fill():
    grid = np.array([[1.0, 0.0, 1.0], [1.5, 5e-4, 3.0]])

    def cand(w=None):
        return {"grid": grid.copy(), "weight": np.full(2, np.nan) if w is None else w}
    w1, w2 = np.array([0.5, 0.5]), np.array([0.125, 0.875])
    rows = _scatter({1: [[None, w1], [None, w2]]}, lambda: [None, cand()], lambda u, per: [None, cand(per[1])])
    for r in rows[:2]:
        assert r[0] is None and np.isnan(r[1]["weight"]).all() and r[1]["grid"].tobytes() == grid.tobytes()
    assert rows[2][0] is None and rows[2][1]["weight"] is w2                # (a pure number: no share enters)


def test_scatter_best_of_a_switch_that_was_not_opened_is_none():
    assert _scatter(None, lambda: [], lambda u, per: per) is None
