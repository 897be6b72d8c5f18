"""ls_spa_best_subsets_bootstrap: the bootstrap of the best-subset selection -- CPU side.

The truth of a replicate (tests/best_boot_ref.py) and the gap between best and runner-up of every (replicate, size) of
every case the GPU tests compare with it; the planner of the run through its host-only hook, with the properties the GPU
cases were chosen for; and the driver's plumbing through a NumPy double of the engine whose replicates are that truth."""
import threading
import warnings

import numpy as np
import pytest

import best_boot_ref as BB
import best_ref as B
import ls_spa as package
from ls_spa import (BestSubsetsBootstrapResults, SizeIncompatible, _driver, ls_spa_best_subsets,
                    ls_spa_best_subsets_bootstrap)
from ls_spa._engine import debug_boot_best_plan, debug_boot_plan
from ls_spa._results import best_sizes
from test_best_subsets_host import BestOracleEngine
from test_subsets_host import data

BITS_BIG = (27, 2)      # (p, R) of the GPU bits case whose plan has per > steps: several launches per replicate


def test_it_is_exported():
    assert "ls_spa_best_subsets_bootstrap" in package.__all__ and "BestSubsetsBootstrapResults" in package.__all__


# ---- the truth and the GPU cases ---------------------------------------------------------------------------------------
def test_truth_of_a_replicate_is_the_selection_on_the_repeated_rows():
    d = data(3, n=12, m=9, seed=1)
    wa, we = np.array([2, 0, 1] * 4), np.array([1, 3, 0] * 3)
    rows = BB.repeated(d, wa, we)
    assert rows[0].shape == (12, 3) and rows[1].shape == (12, 3) and len(rows[2]) == 12 and len(rows[3]) == 12
    np.testing.assert_array_equal(rows[0][:2], d[0][[0, 0]])
    np.testing.assert_array_equal(rows[3][:4], d[3][[0, 1, 1, 1]])
    # weight 1 everywhere: the selection on the rows themselves
    ones = BB.repeated(d, np.ones(12, dtype=int), np.ones(9, dtype=int))
    np.testing.assert_array_equal(B.all_values(ones), B.all_values(d))


@pytest.mark.parametrize("p, reg", BB.CASES)
def test_every_gpu_case_has_a_clear_winner_in_every_replicate(p, reg):
    d, wa, we, v = BB.boot_case(p, reg)
    assert wa.shape == (BB.R, d[0].shape[0]) and we.shape == (BB.R, d[1].shape[0])
    assert wa.min() == 0 and wa.max() == 3 and we.min() == 0 and we.max() == 3
    for inc in BB.includes(p, reg):
        k0 = bin(inc).count("1")
        for r in range(BB.R):
            best, _, found, runner = B.best_truth(v[r], p, inc)
            assert found[k0:].all() and not found[:k0].any()
            assert ((best - runner)[found] > B.MIN_GAP).all(), (p, reg, inc, r, (best - runner)[found].min())


# ---- the planner ---------------------------------------------------------------------------------------------------------
def test_the_plan_of_the_truth_cases():
    """q = p below 6, q = 6 with no high feature (p = 6), one high feature (p = 7), 64 units (p = 12); one launch takes
    all replicates and all steps."""
    want_units = {1: 1, 2: 1, 5: 1, 6: 1, 7: 2, 9: 8, 12: 64}
    for p in B.BRUTE_P:
        d = B.case_data(p)
        plan = debug_boot_best_plan(BB.R, d[0].shape[0], d[1].shape[0], p)
        assert (plan["units"], plan["per"], plan["steps"]) == (want_units[p], 1, 1)
        assert plan["block"] == plan["enum_reps"] == BB.R and plan["n_blocks"] == 1


def test_the_plan_of_the_bits_case_has_several_launches_a_replicate():
    p, R = BITS_BIG
    plan = debug_boot_best_plan(R, 50, 40, p)
    assert plan["per"] > plan["steps"] and plan["per"] // plan["steps"] == 2          # two launches a replicate ...
    assert plan["block"] == R and plan["enum_reps"] == 1                            # ... and one replicate a launch
    assert plan["units"] == 8192 and plan["per"] <= 2 ** 13


def test_the_plan_of_the_independence_case_follows_the_block():
    for block, want in ((0, 7), (1, 1), (3, 3)):
        plan = debug_boot_best_plan(7, 300, 270, 9, block)
        assert plan["block"] == want and plan["enum_reps"] == want and plan["n_blocks"] == -(-7 // want)


@pytest.mark.parametrize("p", [1, 6, 7, 12, 16, 19, 20, 24, 27, 32])
def test_a_table_entry_counts_sixteen_bytes_and_the_bounds_hold(p):
    for R, n, m, block in ((1, 1, 1, 0), (1000, 10 ** 4, 10 ** 4, 0), (200, 10 ** 5, 10 ** 5, 0), (5000, 300, 200, 64),
                           (10 ** 6, 2 ** 31 - 1, 5, 0)):
        best, phi = debug_boot_best_plan(R, n, m, p, block), debug_boot_plan(R, n, m, p, block)
        for k in ("cb", "ldz", "pairs", "rpw", "rps_train", "rps_test", "slices_train", "slices_test", "units", "per"):
            assert best[k] == phi[k]
        assert best["rep_bytes"] == phi["rep_bytes"] + best["units"] * (p + 1) * 8        # 16 bytes against 8
        assert 1 <= best["block"] <= min(R, 1024) and (block == 0 or best["block"] <= block)
        assert best["block"] == 1 or best["block"] * best["rep_bytes"] <= 256 << 20
        assert best["n_blocks"] == -(-R // best["block"])
        assert 1 <= best["enum_reps"] <= best["block"] and 1 <= best["steps"] <= best["per"] <= 2 ** 13
        assert best["units"] * best["enum_reps"] * best["steps"] <= 2 ** 20
        assert best["units"] * best["per"] == 1 << max(p - 6, 0)


def test_the_planner_refuses_what_the_run_refuses():
    for bad in ((0, 5, 5, 4, 0), (3, 0, 5, 4, 0), (3, 5, 2 ** 31, 4, 0), (3, 5, 5, 0, 0), (3, 5, 5, 33, 0), (3, 5, 5, 4, -1)):
        with pytest.raises(ValueError, match="lsspa_debug_boot_best_plan"):
            debug_boot_best_plan(*bad)


# ---- the summaries on hand-made masks ------------------------------------------------------------------------------------
def test_best_sizes_with_ties_and_nan_rows():
    sizes = np.array([2, 3, 4, 5])
    r2 = np.array([[0.1, 0.7, 0.7, 0.2],              # a tie: the smaller size
                   [np.nan, 0.3, np.nan, 0.3],        # NaN skipped, then the tie rule
                   [np.nan] * 4,                      # nothing found
                   [0.5, 0.4, 0.3, 0.2],
                   [-0.5, np.nan, -0.1, -0.1]])       # negative values are values
    assert best_sizes(sizes, r2).tolist() == [3, 3, -1, 2, 4]
    assert best_sizes(sizes, r2[0]).tolist() == 3


class Point:
    sizes = np.array([0, 1, 2, 3])
    subsets = np.array([[0, 0, 0], [1, 0, 0], [1, 0, 1], [1, 1, 1]], dtype=bool)
    r_squared = np.array([0.0, 0.5, 0.6, 0.55])
    best_size = 2
    best_subset = np.array([1, 0, 1], dtype=bool)
    full_r_squared = 0.55


def test_tallies_on_hand_made_masks_leave_a_failed_replicate_out():
    # five replicates at p = 3; replicate 3 failed (its rows would otherwise count), replicate 4 lacks size 3
    masks = np.array([[0, 0b001, 0b101, 0b111],
                      [0, 0b100, 0b101, 0b111],
                      [0, 0b001, 0b011, 0b111],
                      [0, 0b010, 0b110, 0b111],
                      [0, 0b001, 0b101, 0]], dtype=np.uint32)
    found = np.ones((5, 4), dtype=bool)
    found[4, 3] = False
    values = np.array([[0.0, 0.5, 0.6, 0.55],
                       [0.0, 0.4, 0.4, 0.3],         # a tie between sizes 1 and 2: size 1
                       [0.0, 0.2, 0.3, 0.7],
                       [0.0, 0.9, 0.9, 0.9],
                       [0.0, 0.1, 0.2, 123.0]])      # the value beside found = False means nothing
    failed = np.array([False, False, False, True, False])
    res = BestSubsetsBootstrapResults.from_replicates(Point, values, masks, found, np.arange(5.0), failed)
    assert res.n_failed == 1 and res.subset_replicates.shape == (5, 4, 3) and res.subset_replicates.dtype == bool
    assert not res.subset_replicates[3].any() and np.isnan(res.r_squared_replicates[3]).all()
    assert np.isnan(res.r_squared_replicates[4, 3]) and not res.subset_replicates[4, 3].any()
    assert res.subset_replicates[1, 1].tolist() == [False, False, True]
    assert res.best_size_replicates.tolist() == [2, 1, 3, -1, 2]
    assert np.isnan(res.full_r_squared_replicates[3]) and res.full_r_squared_replicates[[0, 1, 2, 4]].tolist() == [0, 1, 2, 4]
    np.testing.assert_array_equal(res.inclusion_frequency, np.array([[0, 0, 0], [3, 0, 1], [4, 1, 3], [3, 3, 3]]) / 4)
    # the overall best models: 101, 100, 111, (failed), 101
    np.testing.assert_array_equal(res.best_inclusion_frequency, np.array([3, 1, 4]) / 4)
    np.testing.assert_array_equal(res.best_size_frequency, np.array([0, 1, 2, 1]) / 4)
    np.testing.assert_array_equal(res.reselected, np.array([4, 3, 3, 3]) / 4)
    assert res.best_size == 2 and res.sizes is not None and "Best model" in repr(res)
    with pytest.raises(RuntimeError, match="3 of 5 bootstrap replicates"):
        BestSubsetsBootstrapResults.from_replicates(Point, values, masks, found, np.arange(5.0),
                                                    np.array([True, True, False, True, False]))


# ---- driver plumbing on a test double --------------------------------------------------------------------------------------
class BootBestOracleEngine(BestOracleEngine):
    """BestOracleEngine with the bootstrap of the selection: a replicate's weights are integers 0 .. 3 drawn from
    (seed, replicate, side) -- or the caller's --, its result the brute-force truth on the repeated rows.  fail: the
    replicates whose info word it sets."""

    def __init__(self, fail=(), **kw):
        super().__init__(**kw)
        self.log, self._fail, self._rows = [], set(fail), None

    def boot_load(self, X_train, X_test, y_train, y_test, reg, grouped=False):
        self.log.append(("boot_load", grouped))
        self._rows, self._reg = (X_train, X_test, y_train, y_test), reg

    def boot_free(self):
        self.log.append(("boot_free",))
        self._rows = None

    def drawn(self, seed, r, side):
        n = self._rows[side].shape[0]
        w = np.random.default_rng([seed, r, side]).integers(0, 4, size=n)
        w[0] = max(w[0], 1)
        return w

    def boot_best_run(self, R, seed, w_train=None, w_test=None, *, include=0, first=0, block=0):
        self.log.append(("boot_best_run", R, first, include, w_train is not None, w_test is not None))
        p = self._rows[0].shape[1]
        v, masks = np.empty((R, p + 1)), np.zeros((R, p + 1), dtype=np.uint32)
        found, r2, info = np.zeros((R, p + 1), dtype=bool), np.empty(R), np.zeros(R, dtype=np.int32)
        for r in range(R):
            wa = self.drawn(seed, first + r, 0) if w_train is None else w_train[r].astype(int)
            we = self.drawn(seed, first + r, 1) if w_test is None else w_test[r].astype(int)
            assert w_train is None or np.array_equal(wa, w_train[r])
            assert w_test is None or np.array_equal(we, w_test[r])
            vals = B.all_values(BB.repeated(self._rows, wa, we), self._reg)
            v[r], masks[r], found[r], _ = B.best_truth(vals, p, include)
            r2[r] = vals[-1]
            if first + r in self._fail:
                info[r] = 1
        return v, masks, found, r2, info


def test_result_shapes_fields_and_frequencies():
    p, n_boot = 5, 6
    d = data(p, n=40, m=30, seed=3)
    eng = BootBestOracleEngine()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        res = ls_spa_best_subsets_bootstrap(*d, n_boot=n_boot, seed=7, _engine=eng)
    assert isinstance(res, BestSubsetsBootstrapResults)
    point = ls_spa_best_subsets(*d, _engine=BestOracleEngine())
    for name in ("sizes", "subsets", "r_squared", "best_subset"):
        np.testing.assert_array_equal(getattr(res, name), getattr(point, name))
    assert res.best_size == point.best_size and res.full_r_squared == point.full_r_squared
    assert res.subset_replicates.shape == (n_boot, p + 1, p) and res.subset_replicates.dtype == bool
    assert res.r_squared_replicates.shape == (n_boot, p + 1) and res.best_size_replicates.shape == (n_boot,)
    assert res.full_r_squared_replicates.shape == (n_boot,) and res.n_failed == 0
    assert res.inclusion_frequency.shape == (p + 1, p) and res.best_inclusion_frequency.shape == (p,)
    assert res.best_size_frequency.shape == (p + 1,) and res.reselected.shape == (p + 1,)
    np.testing.assert_array_equal(res.subset_replicates.sum(axis=2), np.tile(np.arange(p + 1), (n_boot, 1)))
    np.testing.assert_array_equal(res.r_squared_replicates[:, p], res.full_r_squared_replicates)
    # a replicate is the truth on its repeated rows
    eng.boot_load(*d, 0.0)
    for r in (0, n_boot - 1):
        vals = B.all_values(BB.repeated(d, eng.drawn(7, r, 0), eng.drawn(7, r, 1)))
        best, masks, _, _ = B.best_truth(vals, p)
        np.testing.assert_array_equal(res.r_squared_replicates[r], best)
        assert [B.mask_of(np.nonzero(s)[0]) for s in res.subset_replicates[r]] == masks.tolist()
    # the frequencies, recomputed
    np.testing.assert_array_equal(res.inclusion_frequency, res.subset_replicates.mean(axis=0))
    np.testing.assert_array_equal(res.best_size_replicates, np.argmax(res.r_squared_replicates, axis=1))
    chosen = res.subset_replicates[np.arange(n_boot), res.best_size_replicates]
    np.testing.assert_array_equal(res.best_inclusion_frequency, chosen.mean(axis=0))
    np.testing.assert_array_equal(res.best_size_frequency, np.bincount(res.best_size_replicates, minlength=p + 1) / n_boot)
    np.testing.assert_array_equal(res.reselected, (res.subset_replicates == point.subsets[None]).all(axis=2).mean(axis=0))
    assert res.reselected[0] == res.reselected[p] == 1.0 and res.best_size_frequency.sum() == 1.0


def test_include_starts_the_sizes_and_reaches_the_engine():
    p = 5
    d = data(p, n=40, m=30, seed=4)
    eng = BootBestOracleEngine()
    res = ls_spa_best_subsets_bootstrap(*d, n_boot=3, include=[4, 1], _engine=eng)
    assert eng.best_calls == [0b10010] and ("boot_best_run", 3, 0, 0b10010, False, False) in eng.log
    assert res.sizes.tolist() == [2, 3, 4, 5] and res.subset_replicates.shape == (3, 4, p)
    assert res.subset_replicates[:, :, [1, 4]].all() and res.inclusion_frequency[:, [1, 4]].min() == 1.0
    np.testing.assert_array_equal(res.subset_replicates.sum(axis=2), np.tile([2, 3, 4, 5], (3, 1)))
    assert res.best_size_replicates.min() >= 2


def test_a_failed_replicate_is_nan_false_left_out_and_warned_about():
    p, n_boot = 4, 5
    d = data(p, n=30, m=20, seed=5)
    good = ls_spa_best_subsets_bootstrap(*d, n_boot=n_boot, _engine=BootBestOracleEngine())
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        res = ls_spa_best_subsets_bootstrap(*d, n_boot=n_boot, _engine=BootBestOracleEngine(fail=(2,)))
    assert len(seen) == 1 and issubclass(seen[0].category, RuntimeWarning) and seen[0].filename == __file__
    assert "1 of 5 bootstrap replicates had a Gram matrix that was not numerically positive definite" in str(seen[0].message)
    keep = [0, 1, 3, 4]
    assert res.n_failed == 1 and np.isnan(res.r_squared_replicates[2]).all() and not res.subset_replicates[2].any()
    assert res.best_size_replicates[2] == -1 and np.isnan(res.full_r_squared_replicates[2])
    np.testing.assert_array_equal(res.subset_replicates[keep], good.subset_replicates[keep])
    np.testing.assert_array_equal(res.inclusion_frequency, good.subset_replicates[keep].mean(axis=0))
    np.testing.assert_array_equal(res.best_size_frequency,
                                  np.bincount(good.best_size_replicates[keep], minlength=p + 1) / 4)
    with pytest.raises(RuntimeError, match="3 of 5 bootstrap replicates"):
        ls_spa_best_subsets_bootstrap(*d, n_boot=n_boot, _engine=BootBestOracleEngine(fail=(0, 2, 4)))


def test_the_point_estimates_warning_is_this_calls():
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        ls_spa_best_subsets_bootstrap(*data(4, n=30, m=20, seed=2), n_boot=2, _engine=BootBestOracleEngine(info=1))
    assert len(seen) == 1 and "not numerically positive definite" in str(seen[0].message)
    assert seen[0].filename == __file__


def test_weights_and_a_side_that_is_not_resampled(monkeypatch):
    p, n, m = 3, 20, 15
    d = data(p, n=n, m=m, seed=6)
    rng = np.random.default_rng(0)
    wa, we = rng.integers(1, 4, size=(4, n)).astype(float), rng.integers(1, 4, size=(4, m)).astype(float)
    eng = BootBestOracleEngine()
    both = ls_spa_best_subsets_bootstrap(*d, n_boot=4, weights=(wa, we), _engine=eng)
    assert ("boot_best_run", 4, 0, 0, True, True) in eng.log
    eng = BootBestOracleEngine()
    ones = ls_spa_best_subsets_bootstrap(*d, n_boot=4, weights=(wa, np.ones((4, m))), _engine=eng)
    monkeypatch.setattr(_driver, "BOOT_ONES_BYTES", 8 * m * 3)        # three replicates of ones a call
    eng = BootBestOracleEngine()
    train = ls_spa_best_subsets_bootstrap(*d, n_boot=4, weights=(wa, None), resample="train", _engine=eng)
    runs = [e for e in eng.log if e[0] == "boot_best_run"]
    assert runs == [("boot_best_run", 3, 0, 0, True, True), ("boot_best_run", 1, 3, 0, True, True)]
    np.testing.assert_array_equal(train.subset_replicates, ones.subset_replicates)
    np.testing.assert_array_equal(train.r_squared_replicates, ones.r_squared_replicates)
    assert both.subset_replicates.shape == train.subset_replicates.shape


def _zero_y(d):
    return d[0], d[1], d[2], np.zeros_like(d[3])


@pytest.mark.parametrize("make, kw, error, text", [
    (lambda: data(33, n=80, m=50, seed=1), {}, ValueError, "at most p = 32"),
    (lambda: data(6), dict(groups=[0, 0, 1, 1, 2, -1]), ValueError, "does not take groups= yet"),
    (lambda: data(6), dict(include=[6]), ValueError, "outside 0 .. 5"),
    (lambda: data(6), dict(include=[1, 4, 1]), ValueError, "twice"),
    (lambda: data(6), dict(include=[1.5]), ValueError, "integer column indices"),
    (lambda: data(6), dict(include=3), ValueError, "iterable of column indices"),
    (lambda: _zero_y(data(6)), {}, ValueError, "identically zero"),
    (lambda: data(6), dict(n_boot=1), ValueError, "n_boot must be an integer >= 2"),
    (lambda: data(6), dict(n_boot=2.5), ValueError, "n_boot must be an integer >= 2"),
    (lambda: data(6), dict(resample="rows"), ValueError, "resample must name"),
    (lambda: data(6), dict(resample=()), ValueError, "resample must name"),
    (lambda: data(6), dict(n_boot=3, weights=(np.ones((3, 7)), None)), ValueError, "w_train must have shape"),
    (lambda: data(6), dict(n_boot=3, weights=(None, -np.ones((3, data(6)[1].shape[0])))), ValueError,
     "w_test must be finite and >= 0"),
    (lambda: data(6), dict(n_boot=3, weights=(np.zeros((3, data(6)[0].shape[0])), None)), ValueError, "sum to zero"),
    (lambda: data(6), dict(weights=(None,)), ValueError, "weights must be a pair"),
    (lambda: (data(6)[0], data(5)[1]) + data(6)[2:], {}, SizeIncompatible, None),
    (lambda: (data(6)[0][:-1],) + data(6)[1:], {}, SizeIncompatible, None),
])
def test_refusals_come_before_any_engine_work(monkeypatch, make, kw, error, text):
    def no_engine(*a, **k):
        raise AssertionError("an engine was acquired")
    monkeypatch.setattr(_driver, "_acquire_engine", no_engine)
    eng = BootBestOracleEngine()
    with pytest.raises(error, match=text):
        ls_spa_best_subsets_bootstrap(*make(), _engine=eng, **kw)
    assert eng.touched == 0 and eng.best_calls == [] and eng.log == []
    with pytest.raises(error, match=text):
        ls_spa_best_subsets_bootstrap(*make(), **kw)          # no engine of the caller's: none is acquired either


def test_the_call_frees_the_bootstrap_rows_on_success_and_on_failure():
    d = data(4, n=30, m=20, seed=4)
    eng = BootBestOracleEngine()
    ls_spa_best_subsets_bootstrap(*d, n_boot=2, _engine=eng)
    assert [e[0] for e in eng.log] == ["boot_load", "boot_best_run", "boot_free"] and eng.log[0] == ("boot_load", False)

    class Broken(BootBestOracleEngine):
        def boot_best_run(self, *a, **k):
            self.log.append(("boot_best_run",))
            raise RuntimeError("boom")

    eng = Broken()
    with pytest.raises(RuntimeError, match="boom"):
        ls_spa_best_subsets_bootstrap(*d, n_boot=2, _engine=eng)
    assert [e[0] for e in eng.log] == ["boot_load", "boot_best_run", "boot_free"]


def test_the_callers_engine_is_left_open_and_a_kept_one_is_reset(monkeypatch):
    log = []

    class Kept(BootBestOracleEngine):
        def set_flags(self, flags):
            log.append(("set_flags", flags))

        def history_enable(self, n):
            log.append(("history_enable", n))

        def close(self):
            log.append(("close",))

    kept = Kept()
    lock = threading.Lock()
    lock.acquire()
    monkeypatch.setattr(_driver, "_acquire_engine", lambda device: (kept, lock))
    res = ls_spa_best_subsets_bootstrap(*data(4, n=30, m=20, seed=4), n_boot=2)
    assert res.n_failed == 0 and log == [("set_flags", 0), ("history_enable", 0)] and not lock.locked()
    assert [e[0] for e in kept.log] == ["boot_load", "boot_best_run", "boot_free"]
    own = Kept()
    ls_spa_best_subsets_bootstrap(*data(4, n=30, m=20, seed=4), n_boot=2, _engine=own)
    assert log == [("set_flags", 0), ("history_enable", 0)]          # the caller's engine: nothing reset, nothing closed


def test_kept_engine_back_to_float64():
    class Float32Engine(BootBestOracleEngine):
        precision = "float32"

        def set_precision(self, dtype):
            self.precision = np.dtype(dtype).name

    eng = Float32Engine()
    ls_spa_best_subsets_bootstrap(*data(4, n=30, m=20, seed=3), n_boot=2, _engine=eng)
    assert eng.precision == "float64"
