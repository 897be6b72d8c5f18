"""The host side of ls_spa_interactions_bootstrap, without a GPU: the interaction planners through their debug entry
points (lsspa_debug_boot_inter_plan, lsspa_debug_boot_groups_inter_plan), the summary logic of
InteractionBootstrapResults on synthetic replicates, the refusals of the public call that need no engine, and -- on the
recording double of tests/test_driver_lifecycle.py -- that the call frees the bootstrap rows on success and on failure."""
import numpy as np
import pytest

import ls_spa as package
from ls_spa import InteractionBootstrapResults, ls_spa_bootstrap, ls_spa_interactions, ls_spa_interactions_bootstrap
from ls_spa._engine import debug_boot_groups_plan, debug_boot_plan
from test_driver_lifecycle import Boom, RecordingEngine
from test_groups_host import labels_of
from test_interactions_host import shap_matrix
from test_subsets_host import data

BLOCK_BYTES, PER_LAUNCH, UNITS, GROUPS_WORK = 256 << 20, 1 << 20, 8192, 1 << 26


def inter_cols(d):
    return d + 2 + d + d * (d - 1) // 2


def test_it_is_exported():
    assert "ls_spa_interactions_bootstrap" in package.__all__ and "InteractionBootstrapResults" in package.__all__
    assert callable(package.ls_spa_interactions_bootstrap)


# ---- planner ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [12, 20, 27, 32])
def test_steps_are_the_one_problem_cut_whatever_the_run(p):
    n_high = 1 << (p - 6)
    units = min(n_high, UNITS)
    per = n_high // units
    want = min(per, max(1, PER_LAUNCH // units))            # subsets_enumerate's own cut (csrc/lsspa_api.hip)
    for R in (1, 7, 1000):
        for block in (0, 1, 3):
            a = debug_boot_plan(R, 10 ** 4, 10 ** 4, p, block, inter=True)
            assert (a["units"], a["per"], a["steps"]) == (units, per, want)
            assert a["units"] * a["enum_reps"] * a["steps"] <= PER_LAUNCH and 1 <= a["enum_reps"] <= a["block"]
            table = a["enum_reps"] * a["units"] * inter_cols(p) * 8
            assert a["block"] == 1 or a["block"] * a["rep_bytes"] + table <= BLOCK_BYTES
            assert 1 <= a["block"] <= min(R, 1024) and (block == 0 or a["block"] <= block)
            assert a["n_blocks"] == -(-R // a["block"])
            b = debug_boot_plan(R, 10 ** 4, 10 ** 4, p, block)
            for key in ("cb", "ldz", "pairs", "rpw", "rps_train", "rps_test", "slices_train", "slices_test"):
                assert a[key] == b[key]
    # the table stands beside the block: it does not cut a block to the handful that 256 MB / 37 MB would leave
    assert debug_boot_plan(1000, 10 ** 4, 10 ** 4, 32, inter=True)["block"] >= 100
    assert debug_boot_plan(1000, 10 ** 4, 10 ** 4, 12, inter=True)["enum_reps"] > 64     # the grid is filled at small p


def test_small_p_and_refusals_of_the_planner():
    for p in (1, 2, 5, 6, 7):
        a = debug_boot_plan(9, 50, 40, p, inter=True)
        assert a["units"] == (1 if p <= 6 else 2) and a["per"] == a["steps"] == 1 and a["enum_reps"] == 9
    for bad in ((0, 5, 5, 3, 0), (1, 0, 5, 3, 0), (1, 5, 2 ** 31, 3, 0), (1, 5, 5, 33, 0), (1, 5, 5, 0, 0), (1, 5, 5, 3, -1)):
        with pytest.raises(ValueError):
            debug_boot_plan(*bad, inter=True)


GROUP_SHAPES = {
    "g8_p40": labels_of([5] * 8, 0, seed=8),
    "g12_p64": labels_of([1] * 6 + [10] * 5 + [8], 0, seed=12),
    "g20_p20_two_steps": labels_of([1] * 20),
    "g20_p64_six_launches": labels_of([4] * 4 + [3] * 16, 0, seed=20),
    "g26_p64_baseline": labels_of([1] * 6 + [2] * 20, 18, seed=26),
    "g32_p64": labels_of([1] * 6 + [2] * 19 + [3] * 6 + [2], 0, seed=32),
}


@pytest.mark.parametrize("name", list(GROUP_SHAPES))
def test_the_grouped_planner_keeps_the_phi_planners_cut(name):
    labels = GROUP_SHAPES[name]
    g = int(labels.max()) + 1
    seen = set()
    for R in (1, 7, 1000):
        for block in (0, 1, 3):
            a = debug_boot_groups_plan(R, 10 ** 4, 10 ** 4, labels, block, inter=True)
            b = debug_boot_groups_plan(R, 10 ** 4, 10 ** 4, labels, block)
            for key in ("cb", "ldz", "pairs", "rpw", "rps_train", "rps_test", "slices_train", "slices_test", "units", "per",
                        "steps"):
                assert a[key] == b[key]
            seen.add((a["units"], a["per"], a["steps"]))
            assert a["units"] * a["enum_reps"] * a["steps"] <= PER_LAUNCH and 1 <= a["enum_reps"] <= a["block"]
            table = a["enum_reps"] * a["units"] * inter_cols(g) * 8
            assert a["block"] == 1 or a["block"] * a["rep_bytes"] + table <= BLOCK_BYTES
            assert 1 <= a["block"] <= min(R, 1024) and (block == 0 or a["block"] <= block)
    assert len(seen) == 1


def test_the_old_planners_are_unchanged():
    """The fifteen numbers of the phi planners as the parent commit returns them, at a few shapes."""
    fields = ("cb", "ldz", "pairs", "rpw", "rps_train", "rps_test", "slices_train", "slices_test", "rep_bytes", "block",
              "n_blocks", "enum_reps", "units", "per", "steps")
    want = {
        (1000, 10 ** 4, 10 ** 4, 12): (1, 16, 1, 4, 256, 256, 40, 40, 341312, 786, 2, 786, 64, 1, 1),
        (1000, 10 ** 5, 10 ** 5, 24): (2, 32, 3, 4, 784, 784, 128, 128, 4851264, 55, 19, 55, 8192, 32, 2),
        (7, 513, 77, 16): (2, 32, 3, 4, 256, 256, 3, 1, 187056, 7, 1, 7, 1024, 1, 1),
        (5, 300, 270, 32): (3, 48, 6, 2, 256, 256, 2, 2, 2286096, 5, 1, 5, 8192, 8192, 25),
    }
    for args, numbers in want.items():
        got = debug_boot_plan(*args)
        assert tuple(got[k] for k in fields) == numbers, (args, got)
    gwant = {
        "g8_p40": (3, 48, 6, 2, 256, 256, 40, 40, 1259840, 213, 5, 213, 128, 1, 1),
        "g20_p64_six_launches": (5, 80, 15, 1, 256, 256, 40, 40, 4264256, 62, 17, 1, 8192, 32, 6),
    }
    for name, numbers in gwant.items():
        got = debug_boot_groups_plan(1000, 10 ** 4, 10 ** 4, GROUP_SHAPES[name])
        assert tuple(got[k] for k in fields) == numbers, (name, got)


# ---- InteractionBootstrapResults -----------------------------------------------------------------------------------------
def synthetic(n_boot=9, d=4, seed=0):
    rng = np.random.default_rng(seed)
    raw = rng.standard_normal((n_boot, d, d))
    raw = raw + np.swapaxes(raw, 1, 2)
    att = rng.standard_normal((n_boot, d))
    rep = np.stack([shap_matrix(r, a) for r, a in zip(raw, att)])
    return rep, att, rep.sum(axis=(1, 2))


def test_results_summaries_on_synthetic_replicates():
    rep, att, r2 = synthetic()
    failed = np.zeros(9, dtype=bool)
    failed[[2, 5]] = True
    point = shap_matrix(np.ones((4, 4)), np.arange(4.0))
    res = InteractionBootstrapResults.from_replicates(point, np.arange(4.0), np.ones(6), 0.5, rep, att, r2, failed,
                                                      confidence=0.5)
    ok = rep[~failed]
    assert res.n_failed == 2 and res.confidence == 0.5 and res.baseline_r_squared_replicates is None
    assert res.replicates.shape == (9, 4, 4) and res.attribution_replicates.shape == (9, 4)
    assert res.std_error.shape == res.lower.shape == res.upper.shape == res.prob_positive.shape == (4, 4)
    assert np.isnan(res.replicates[failed]).all() and np.isnan(res.attribution_replicates[failed]).all()
    assert np.isnan(res.r_squared_replicates[failed]).all()
    np.testing.assert_array_equal(res.replicates[~failed], ok)
    np.testing.assert_array_equal(res.attribution_replicates[~failed], att[~failed])
    np.testing.assert_array_equal(res.lower, np.quantile(ok, 0.25, axis=0))
    np.testing.assert_array_equal(res.upper, np.quantile(ok, 0.75, axis=0))
    np.testing.assert_array_equal(res.std_error, ok.std(axis=0, ddof=1))
    count = np.zeros((4, 4))
    for r in range(9):
        if not failed[r]:
            count += rep[r] > 0
    np.testing.assert_array_equal(res.prob_positive, count / 7)
    for field in (res.interactions, res.lower, res.upper, res.std_error, res.prob_positive):
        np.testing.assert_array_equal(field, field.T)
    np.testing.assert_array_equal(res.interactions, point)
    assert np.all(res.lower <= res.upper) and res.theta.shape == (6,) and res.r_squared == 0.5
    assert np.isfinite(rep[2]).all()                             # the caller's array is not written
    assert "9 bootstrap replicates (2 failed)" in repr(res)
    with pytest.raises(RuntimeError, match="5 of 9"):
        InteractionBootstrapResults.from_replicates(point, np.arange(4.0), np.ones(6), 0.5, rep, att, r2,
                                                    [True] * 5 + [False] * 4)
    base = np.linspace(0.1, 0.2, 9)
    grouped = InteractionBootstrapResults.from_replicates(point, np.arange(4.0), np.ones(6), 0.5, rep, att, r2, failed,
                                                          0.95, base)
    assert np.isnan(grouped.baseline_r_squared_replicates[failed]).all() and grouped.confidence == 0.95
    np.testing.assert_array_equal(grouped.baseline_r_squared_replicates[~failed], base[~failed])
    np.testing.assert_array_equal(grouped.upper, np.quantile(ok, 1.0 - (1.0 - 0.95) / 2.0, axis=0))
    assert base[2] == np.linspace(0.1, 0.2, 9)[2]


# ---- refusals that need no engine ----------------------------------------------------------------------------------------
def test_argument_checks_need_no_engine():
    d = data(4, n=30, m=20, seed=1)

    class NoEngine:
        def __getattr__(self, name):
            raise AssertionError(f"the engine was asked for {name} before the arguments were checked")

    def call(*a, **k):
        return ls_spa_interactions_bootstrap(*a, _engine=NoEngine(), **k)

    with pytest.raises(ValueError, match="at most p = 32"):
        call(*data(33, n=40, m=40, seed=1))
    with pytest.raises(ValueError, match="at most p = 64 columns"):
        call(*data(65, n=80, m=80, seed=1), groups=np.arange(65) % 4)
    with pytest.raises(ValueError, match="at most g = 32"):
        call(*data(40, n=50, m=50, seed=1), groups=np.arange(40))
    with pytest.raises(ValueError, match="two players"):
        call(*data(1, n=30, m=20, seed=1))
    with pytest.raises(ValueError, match="two players"):
        call(*d, groups=[0, 0, -1, 0])
    with pytest.raises(ValueError, match="gap in its numbering"):
        call(*d, groups=[0, 0, 2, 2])
    for kw, what in ((dict(n_boot=1), "n_boot"), (dict(confidence=1.0), "confidence"), (dict(confidence=0.0), "confidence"),
                     (dict(resample=()), "resample"), (dict(resample=("train", "valid")), "resample"),
                     (dict(weights=(None,)), "pair"), (dict(n_boot=3, weights=(np.ones((3, 29)), None)), "w_train"),
                     (dict(n_boot=3, weights=(None, -np.ones((3, 20)))), "w_test must be finite and >= 0"),
                     (dict(n_boot=3, weights=(np.zeros((3, 30)), None)), "replicate 0 sum to zero")):
        with pytest.raises(ValueError, match=what):
            call(*d, **kw)
        with pytest.raises(ValueError, match=what):
            call(*d, groups=[0, 1, 1, -1], **kw)


# ---- lifecycle on the recording double -----------------------------------------------------------------------------------
class BootRecordingEngine(RecordingEngine):
    """The recording double with the bootstrap's methods: replicate r is the point estimate scaled by 1 + r / 10 (what the
    replicates hold is the GPU tests' business; here the order of calls is)."""
    RECORDED = RecordingEngine.RECORDED + ("boot_load", "boot_free", "boot_run", "boot_interactions_run",
                                           "boot_groups_interactions_run")

    def boot_load(self, X_train, X_test, y_train, y_test, reg, grouped=False):
        self.boot_rows = (len(X_train), len(X_test))

    def boot_free(self):
        self.boot_rows = None

    def _scaled(self, point, R, first):
        s = 1.0 + (first + np.arange(R)) / 10.0
        return [s.reshape((R,) + (1,) * np.ndim(x)) * x for x in point]

    def boot_run(self, R, seed, w_train=None, w_test=None, block=0, first=0):
        phi, _ = RecordingEngine.subsets_shapley(self)
        return (*self._scaled((phi,), R, first), np.full(R, 0.5), np.zeros(R, dtype=np.int32))

    def boot_interactions_run(self, R, seed, w_train=None, w_test=None, block=0, first=0):
        phi, raw, _ = RecordingEngine.subsets_interactions(self)
        return (*self._scaled((phi, raw), R, first), np.full(R, 0.5), np.zeros(R, dtype=np.int32))

    def boot_groups_interactions_run(self, labels, R, seed, w_train=None, w_test=None, block=0, first=0):
        phi, raw, _ = RecordingEngine.groups_interactions(self, labels)
        return (*self._scaled((phi, raw), R, first), np.full(R, 0.5), np.full(R, 0.1), np.zeros(R, dtype=np.int32))


def names(log):
    return [entry[0] for entry in log]


@pytest.mark.parametrize("groups", [None, labels_of([3, 3, 3], 1, seed=4)])
def test_the_call_frees_the_bootstrap_rows_on_success(groups):
    d, log = data(10, seed=90), []
    eng = BootRecordingEngine(log)
    res = ls_spa_interactions_bootstrap(*d, n_boot=6, seed=3, groups=groups, _engine=eng)
    run = "boot_interactions_run" if groups is None else "boot_groups_interactions_run"
    point = "subsets_interactions" if groups is None else "groups_interactions"
    order = [n for n in names(log) if n in ("load_data", "full_fit", point, "boot_load", run, "boot_free", "close")]
    assert order == ["load_data", "full_fit", point, "boot_load", run, "boot_free"]      # the caller's engine stays open
    assert eng.boot_rows is None
    want = ls_spa_interactions(*d, groups=groups, _engine=BootRecordingEngine([]))
    np.testing.assert_array_equal(res.interactions, want.interactions)
    np.testing.assert_array_equal(res.attribution, want.attribution)
    dd = len(want.attribution)
    assert res.replicates.shape == (6, dd, dd) and res.n_failed == 0
    assert (res.baseline_r_squared_replicates is None) == (groups is None)
    np.testing.assert_allclose(res.replicates[5], 1.5 * want.interactions, rtol=1e-14)
    load = next(e for e in log if e[0] == "boot_load")
    assert bool(load[2].get("grouped", False)) == (groups is not None)


@pytest.mark.parametrize("fail", ["boot_interactions_run", "boot_load", "subsets_interactions"])
def test_the_call_frees_the_bootstrap_rows_on_failure(fail):
    d, log = data(10, seed=90), []
    eng = BootRecordingEngine(log, fail=fail)
    with pytest.raises(Boom):
        ls_spa_interactions_bootstrap(*d, n_boot=6, seed=3, _engine=eng)
    got = names(log)
    if fail == "boot_interactions_run":
        assert got.index("boot_load") < got.index(fail) < got.index("boot_free") and got.count("boot_free") == 1
        assert eng.boot_rows is None
    else:
        assert "boot_free" not in got and "boot_interactions_run" not in got      # nothing was loaded: nothing to free


def test_a_side_that_is_not_resampled_is_cut_like_ls_spa_bootstraps(monkeypatch):
    from ls_spa import _driver
    d, log = data(10, n=60, m=40, seed=90), []
    monkeypatch.setattr(_driver, "BOOT_ONES_BYTES", 8 * 60 * 4)                       # four replicates of ones a call
    ls_spa_interactions_bootstrap(*d, n_boot=10, seed=3, resample="test", _engine=BootRecordingEngine(log))
    runs = [e for e in log if e[0] == "boot_interactions_run"]
    assert [(e[1][0], e[2]["first"]) for e in runs] == [(4, 0), (4, 4), (2, 8)]
    assert all(e[1][2].shape == (e[1][0], 60) and (e[1][2] == 1.0).all() and e[1][3] is None for e in runs)
    log2 = []
    ls_spa_bootstrap(*d, n_boot=10, seed=3, resample="test", _engine=BootRecordingEngine(log2))
    runs2 = [e for e in log2 if e[0] == "boot_run"]
    assert [(e[1][0], e[2]["first"]) for e in runs2] == [(4, 0), (4, 4), (2, 8)]
