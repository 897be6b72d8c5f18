"""ls_spa_best_group_subsets_bootstrap: the bootstrap of the best-subset selection over groups of columns -- CPU side.

The truth of a replicate (tests/group_best_boot_ref.py) and the gap between best and runner-up of every (replicate, size)
of every case the GPU tests compare with it; the planner of the run through its host-only hook, with the edges the GPU
cases were chosen for; and the driver's plumbing through a NumPy double of the engine whose replicates are that truth."""
import warnings

import numpy as np
import pytest

import best_ref as B
import group_best_boot_ref as GB
import group_best_ref as GR
import ls_spa as package
from ls_spa import (BestGroupSubsetsBootstrapResults, BestSubsetsBootstrapResults, SizeIncompatible, _driver,
                    ls_spa_best_group_subsets_bootstrap, ls_spa_best_subsets, ls_spa_best_subsets_bootstrap)
from ls_spa._engine import debug_boot_groups_best_plan, debug_boot_groups_plan
from test_group_best_host import GroupBestOracleEngine
from test_groups_host import group_values, labels_of, value
from test_subsets_host import data, gram_problem

BITS_PLANTED = ("g20x3", 2, 128)        # (PLANTED name, R, rows a side) of the GPU bits case with several launches a replicate
BITS_SPLIT = ("g12p64", 256, 192)       # (case, n, m) of the GPU bits case whose replicates are split over launches
INDEPENDENCE = ("nine", 7)              # (case, R) of the GPU independence case


def split_R():
    """R of the BITS_SPLIT run: two more replicates than one enumeration launch takes at most."""
    name, n, m = BITS_SPLIT
    return debug_boot_groups_best_plan(1000, n, m, GR.case_labels(name))["enum_reps"] + 2


def test_it_is_exported():
    assert "ls_spa_best_group_subsets_bootstrap" in package.__all__
    assert "BestGroupSubsetsBootstrapResults" in package.__all__


def test_the_column_call_still_refuses_groups_with_its_old_message():
    with pytest.raises(ValueError, match="does not take groups= yet"):
        ls_spa_best_subsets_bootstrap(*data(6), groups=[0, 0, 1, 1, 2, -1])


# ---- the truth and the GPU cases ---------------------------------------------------------------------------------------
def test_truth_of_a_replicate_is_the_one_problem_truth_on_the_repeated_rows():
    labels = labels_of([2, 1, 2], 1, seed=2)
    d = data(6, n=14, m=10, seed=1)
    wa, we = np.array([2, 0, 1, 3, 1, 0, 2] * 2), np.array([1, 3, 0, 2, 1] * 2)
    rows = GB.repeated(d, wa, we)
    assert rows[0].shape == (18, 6) and rows[1].shape == (14, 6) and len(rows[2]) == 18 and len(rows[3]) == 14
    u = GB.replicate_values(d, labels, wa, we, 0.1)
    np.testing.assert_array_equal(u, GR.all_group_values(rows, labels, 0.1))
    # the same numbers from the weighted Grams of the rows themselves, to rounding: a replicate IS a weighting
    G = (d[0].T * wa) @ d[0] / wa.sum() + 0.1 * np.eye(6)
    gv = (d[0].T * wa) @ d[2] / wa.sum()
    H, h, yy = (d[1].T * we) @ d[1], (d[1].T * we) @ d[3], float(we @ (d[3] * d[3]))
    np.testing.assert_allclose(u, group_values(G, gv, H, h, yy, labels, np.arange(8)), rtol=0, atol=1e-12)
    # weight 1 everywhere: the selection on the rows themselves
    ones = GB.replicate_values(d, labels, np.ones(14, dtype=int), np.ones(10, dtype=int))
    np.testing.assert_array_equal(ones, GR.all_group_values(d, labels))
    best, masks, found, _ = GB.truth(u, 3)
    assert found.all() and masks[0] == 0 and masks[3] == 7
    assert abs(best[0] - value(*gram_problem(*rows, reg=0.1), np.nonzero(labels < 0)[0])) < 1e-13      # the baseline alone


@pytest.mark.parametrize("name, reg", GB.CASES)
def test_every_gpu_case_has_a_clear_winner_in_every_replicate(name, reg):
    d, labels, wa, we, u = GB.boot_case(name, reg)
    g = int(labels.max()) + 1
    assert wa.shape == (GB.R, d[0].shape[0]) and we.shape == (GB.R, d[1].shape[0]) and u.shape == (GB.R, 1 << g)
    assert wa.min() == 0 and wa.max() == 3 and we.min() == 0 and we.max() == 3
    assert (we.sum(axis=1) > 0).all() and (wa.sum(axis=1) > 0).all()          # "rect": M = 9 test rows
    for r in range(GB.R):
        best, masks, found, runner = GB.truth(u[r], g)
        assert found.all() and masks[0] == 0 and masks[g] == (1 << g) - 1
        assert ((best - runner) > GR.MIN_GAP).all(), (name, reg, r, (best - runner).min())
    assert len({tuple(GB.truth(u[r], g)[0]) for r in range(GB.R)}) == GB.R      # the replicates do differ


def test_the_cases_are_the_grouped_selections_own():
    assert set(GB.NAMES) == {"gl0", "gl6", "mixed", "alllow", "nine", "rect"} and GB.R == 3
    assert GB.CASES == [(name, reg) for name in GB.NAMES for reg in (0.0, 0.1)]
    assert (GR.case_data("rect")[1].shape[0] < GR.case_data("rect")[0].shape[1])


# ---- the planner ---------------------------------------------------------------------------------------------------------
def rows_of(labels):
    """Rows of a high subset's matrix as the one-problem call counts its work (include/lsspa.h)."""
    from ls_spa._engine import debug_groups_best_plan
    q = debug_groups_best_plan(labels)
    p = len(labels)
    return (q["nb"] + q["ql"] + 1) + (p - q["nb"] - q["ql"] + 1) // 2


SWEEP = [labels_of([7, 7, 7]), labels_of([1] * 6 + [3, 4], 2), labels_of([1, 2, 3], 2), np.arange(12) // 3,
         np.repeat(np.arange(8), 5), labels_of([5] * 12, 4), np.repeat(np.arange(16), 3), np.repeat(np.arange(20), 3),
         np.arange(28), np.repeat(np.arange(32), 2), np.arange(32), labels_of([2] * 26 + [1] * 6, 6)]


@pytest.mark.parametrize("labels", SWEEP, ids=lambda a: f"p{len(a)}g{int(np.max(a)) + 1}")
def test_a_table_entry_counts_sixteen_bytes_and_the_three_bounds_hold(labels):
    g = int(labels.max()) + 1
    rows = rows_of(labels)
    for R, n, m, block in ((1, 1, 1, 0), (1000, 10 ** 4, 10 ** 4, 0), (200, 10 ** 5, 10 ** 5, 0), (5000, 300, 200, 64),
                           (10 ** 6, 2 ** 31 - 1, 5, 0), (7, 120, 90, 2)):
        best, phi = debug_boot_groups_best_plan(R, n, m, labels, block), debug_boot_groups_plan(R, n, m, labels, block)
        for k in ("cb", "ldz", "pairs", "rpw", "rps_train", "rps_test", "slices_train", "slices_test", "units", "per"):
            assert best[k] == phi[k]
        assert best["rep_bytes"] == phi["rep_bytes"] + best["units"] * (g + 1) * 8        # 16 bytes against 8
        assert 1 <= best["block"] <= min(R, 1024) and (block == 0 or best["block"] <= block)
        assert best["n_blocks"] == -(-R // best["block"])
        assert 1 <= best["enum_reps"] <= best["block"] and 1 <= best["steps"] <= best["per"]
        assert best["per"] <= 2 ** 18                                                     # GROUPS_BEST_CLASSES - 1 bits
        # 1. memory  2. workgroups a launch  3. the grouped work bound a launch (unless one step of one replicate is more)
        assert best["block"] == 1 or best["block"] * best["rep_bytes"] <= 256 << 20
        assert best["units"] * best["enum_reps"] <= 2 ** 20
        work = best["units"] * best["enum_reps"] * best["steps"] * rows * rows
        assert work <= 2 ** 26 or (best["enum_reps"] == 1 and best["steps"] == 1)
        # steps is the one-problem call's cut; the replicates fill what it leaves, so nothing is left idle by a factor 2
        assert best["steps"] == phi["steps"]
        if best["enum_reps"] < best["block"]:
            assert best["units"] * (best["enum_reps"] + 1) * best["steps"] * rows * rows > 2 ** 26 or \
                best["units"] * (best["enum_reps"] + 1) > 2 ** 20


def test_the_plans_of_the_gpu_cases_reach_the_three_edges():
    # the truth cases: one launch takes all replicates and all steps
    for name in GB.NAMES:
        _, _, _, (n, m, _) = GR.CASES[name]
        plan = debug_boot_groups_best_plan(GB.R, n, m, GR.case_labels(name))
        assert (plan["per"], plan["steps"]) == (1, 1) and plan["units"] == GR.PLAN[name]["units"]
        assert plan["block"] == plan["enum_reps"] == GB.R and plan["n_blocks"] == 1
    # edge 1: a unit's steps are cut into several launches a replicate, one replicate a launch
    name, R, n = BITS_PLANTED
    plan = debug_boot_groups_best_plan(R, n, n, GR.PLANTED[name][0])
    assert plan["per"] == 32 and plan["steps"] < plan["per"] and -(-plan["per"] // plan["steps"]) == 5
    assert plan["block"] == R and plan["enum_reps"] == 1 and plan["units"] == 8192
    # edge 2: the replicates of one block are split over enumeration launches
    name, n, m = BITS_SPLIT
    R = split_R()
    plan = debug_boot_groups_best_plan(R, n, m, GR.case_labels(name))
    assert plan["n_blocks"] == 1 and plan["block"] == R and 1 < plan["enum_reps"] == R - 2
    # edge 3: the run is cut into blocks
    name, R = INDEPENDENCE
    _, _, _, (n, m, _) = GR.CASES[name]
    for block, want in ((0, 7), (1, 1), (2, 2)):
        plan = debug_boot_groups_best_plan(R, n, m, GR.case_labels(name), block)
        assert plan["block"] == want and plan["enum_reps"] == want and plan["n_blocks"] == -(-R // want)


@pytest.mark.parametrize("bad", [
    (0, 5, 5, [0, 0, 1, 1], 0), (3, 0, 5, [0, 0, 1, 1], 0), (3, 5, 2 ** 31, [0, 0, 1, 1], 0), (3, 5, 5, [0, 0, 1, 1], -1),
    (3, 5, 5, [0, 0, 2, 2], 0), (3, 5, 5, [-2, 0, 0, 1], 0), (3, 5, 5, [-1, -1, -1], 0), (3, 5, 5, np.arange(33), 0),
    (3, 5, 5, np.zeros(65, dtype=int), 0)])
def test_the_planner_refuses_what_the_run_refuses(bad):
    with pytest.raises(ValueError, match="lsspa_debug_boot_groups_best_plan"):
        debug_boot_groups_best_plan(*bad)


# ---- the summaries on hand-made masks ------------------------------------------------------------------------------------
class Point:
    """Three groups over five columns: labels 0 0 1 -1 2."""
    sizes = np.array([0, 1, 2, 3])
    group_subsets = np.array([[0, 0, 0], [1, 0, 0], [1, 0, 1], [1, 1, 1]], dtype=bool)
    subsets = np.array([[0, 0, 0, 1, 0], [1, 1, 0, 1, 0], [1, 1, 0, 1, 1], [1, 1, 1, 1, 1]], dtype=bool)
    r_squared = np.array([0.1, 0.5, 0.6, 0.55])
    best_size = 2
    best_group_subset = np.array([1, 0, 1], dtype=bool)
    best_subset = np.array([1, 1, 0, 1, 1], dtype=bool)
    full_r_squared = 0.55
    baseline_r_squared = 0.1


MASKS = np.array([[0, 0b001, 0b101, 0b111],
                  [0, 0b100, 0b101, 0b111],
                  [0, 0b001, 0b011, 0b111],
                  [0, 0b010, 0b110, 0b111],
                  [0, 0b001, 0b101, 0]], dtype=np.uint32)
VALUES = np.array([[0.0, 0.5, 0.6, 0.55],
                   [0.0, 0.4, 0.4, 0.3],         # a tie between sizes 1 and 2: size 1
                   [0.0, 0.2, 0.3, 0.7],
                   [0.0, 0.9, 0.9, 0.9],
                   [0.0, 0.1, 0.2, 123.0]])      # the value beside found = False means nothing


def test_tallies_on_hand_made_masks_leave_a_failed_replicate_out():
    # five replicates at g = 3; replicate 3 failed (its rows would otherwise count), replicate 4 lacks size 3
    found = np.ones((5, 4), dtype=bool)
    found[4, 3] = False
    failed = np.array([False, False, False, True, False])
    full, base = np.arange(5.0), np.arange(5.0) / 10
    res = BestGroupSubsetsBootstrapResults.from_replicates(Point, VALUES, MASKS, found, full, base, failed)
    assert res.n_failed == 1 and res.group_subset_replicates.shape == (5, 4, 3)
    assert res.group_subset_replicates.dtype == bool
    assert not res.group_subset_replicates[3].any() and np.isnan(res.r_squared_replicates[3]).all()
    assert np.isnan(res.r_squared_replicates[4, 3]) and not res.group_subset_replicates[4, 3].any()
    assert res.group_subset_replicates[1, 1].tolist() == [False, False, True]
    assert res.best_size_replicates.tolist() == [2, 1, 3, -1, 2]
    assert np.isnan(res.full_r_squared_replicates[3]) and res.full_r_squared_replicates[[0, 1, 2, 4]].tolist() == [0, 1, 2, 4]
    assert np.isnan(res.baseline_r_squared_replicates[3])
    assert res.baseline_r_squared_replicates[[0, 1, 2, 4]].tolist() == [0.0, 0.1, 0.2, 0.4]
    np.testing.assert_array_equal(res.inclusion_frequency, np.array([[0, 0, 0], [3, 0, 1], [4, 1, 3], [3, 3, 3]]) / 4)
    np.testing.assert_array_equal(res.best_inclusion_frequency, np.array([3, 1, 4]) / 4)
    np.testing.assert_array_equal(res.best_size_frequency, np.array([0, 1, 2, 1]) / 4)
    np.testing.assert_array_equal(res.reselected, np.array([4, 3, 3, 3]) / 4)
    # the point estimate's fields, groups and columns apart
    np.testing.assert_array_equal(res.group_subsets, Point.group_subsets)
    np.testing.assert_array_equal(res.subsets, Point.subsets)
    np.testing.assert_array_equal(res.best_group_subset, Point.best_group_subset)
    np.testing.assert_array_equal(res.best_subset, Point.best_subset)
    assert res.best_size == 2 and res.full_r_squared == 0.55 and res.baseline_r_squared == 0.1
    assert "Best model: 2 groups" in repr(res) and "g = 3 groups over p = 5 columns" in repr(res)
    # the tallies are the column results' own, with the groups as the players
    class Players(Point):
        subsets, best_subset = Point.group_subsets, Point.best_group_subset
    col = BestSubsetsBootstrapResults.from_replicates(Players, VALUES, MASKS, found, full, failed)
    for a, b in (("group_subset_replicates", "subset_replicates"), ("inclusion_frequency",) * 2, ("reselected",) * 2,
                 ("best_inclusion_frequency",) * 2, ("best_size_frequency",) * 2, ("best_size_replicates",) * 2):
        np.testing.assert_array_equal(getattr(res, a), getattr(col, b))
    with pytest.raises(RuntimeError, match="3 of 5 bootstrap replicates"):
        BestGroupSubsetsBootstrapResults.from_replicates(Point, VALUES, MASKS, found, full, base,
                                                         np.array([True, True, False, True, False]))


# ---- driver plumbing on a test double --------------------------------------------------------------------------------------
class GroupBootBestOracleEngine(GroupBestOracleEngine):
    """GroupBestOracleEngine with the bootstrap of the grouped selection: a replicate's weights are integers 0 .. 3 drawn
    from (seed, replicate, side) -- or the caller's --, its result the brute-force truth on the repeated rows.  fail: the
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

    def boot_groups_best_run(self, labels, R, seed, w_train=None, w_test=None, *, first=0, block=0):
        assert isinstance(labels, np.ndarray) and labels.dtype == np.int32
        self.log.append(("boot_groups_best_run", R, first, w_train is not None, w_test is not None))
        g = int(labels.max()) + 1
        base_cols = np.nonzero(labels < 0)[0]
        u, masks = np.empty((R, g + 1)), np.zeros((R, g + 1), dtype=np.uint32)
        found, r2, base, info = np.zeros((R, g + 1), dtype=bool), np.empty(R), np.empty(R), np.zeros(R, dtype=np.int32)
        for r in range(R):
            wa = self.drawn(seed, first + r, 0) if w_train is None else w_train[r].astype(int)
            we = self.drawn(seed, first + r, 1) if w_test is None else w_test[r].astype(int)
            assert w_train is None or np.array_equal(wa, w_train[r])
            assert w_test is None or np.array_equal(we, w_test[r])
            rows = GB.repeated(self._rows, wa, we)
            vals = GR.all_group_values(rows, labels, self._reg)
            u[r], masks[r], found[r], _ = B.best_truth(vals, g)
            r2[r], base[r] = vals[-1], value(*gram_problem(*rows, reg=self._reg), base_cols)
            if first + r in self._fail:
                info[r] = 1
        return u, masks, found, r2, base, info


LABELS = labels_of([2, 1, 2], 1, seed=7)        # p = 6, g = 3, one baseline column


def test_result_shapes_fields_and_frequencies():
    p, g, n_boot = 6, 3, 6
    d = data(p, n=40, m=30, seed=3)
    eng = GroupBootBestOracleEngine()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        res = ls_spa_best_group_subsets_bootstrap(*d, LABELS, n_boot=n_boot, seed=7, _engine=eng)
    assert isinstance(res, BestGroupSubsetsBootstrapResults)
    assert len(eng.group_best_calls) == 1 and eng.best_calls == []              # the point estimate, by its own path
    point = ls_spa_best_subsets(*d, groups=LABELS, _engine=GroupBestOracleEngine())
    for name in ("sizes", "group_subsets", "subsets", "r_squared", "best_group_subset", "best_subset"):
        np.testing.assert_array_equal(getattr(res, name), getattr(point, name))
    assert res.best_size == point.best_size and res.full_r_squared == point.full_r_squared
    assert res.baseline_r_squared == point.baseline_r_squared and res.sizes.tolist() == [0, 1, 2, 3]
    assert res.group_subset_replicates.shape == (n_boot, g + 1, g) and res.group_subset_replicates.dtype == bool
    assert res.r_squared_replicates.shape == (n_boot, g + 1) and res.best_size_replicates.shape == (n_boot,)
    assert res.full_r_squared_replicates.shape == (n_boot,) and res.baseline_r_squared_replicates.shape == (n_boot,)
    assert res.inclusion_frequency.shape == (g + 1, g) and res.best_inclusion_frequency.shape == (g,)
    assert res.best_size_frequency.shape == (g + 1,) and res.reselected.shape == (g + 1,) and res.n_failed == 0
    np.testing.assert_array_equal(res.group_subset_replicates.sum(axis=2), np.tile(np.arange(g + 1), (n_boot, 1)))
    np.testing.assert_array_equal(res.r_squared_replicates[:, g], res.full_r_squared_replicates)
    np.testing.assert_allclose(res.r_squared_replicates[:, 0], res.baseline_r_squared_replicates, rtol=0, atol=1e-13)
    # a replicate is the truth on its repeated rows
    eng.boot_load(*d, 0.0)
    for r in (0, n_boot - 1):
        vals = GB.replicate_values(d, LABELS, eng.drawn(7, r, 0), eng.drawn(7, r, 1))
        best, masks, _, _ = B.best_truth(vals, g)
        np.testing.assert_array_equal(res.r_squared_replicates[r], best)
        assert [B.mask_of(np.nonzero(s)[0]) for s in res.group_subset_replicates[r]] == masks.tolist()
    # the frequencies, recomputed
    np.testing.assert_array_equal(res.inclusion_frequency, res.group_subset_replicates.mean(axis=0))
    np.testing.assert_array_equal(res.best_size_replicates, np.argmax(res.r_squared_replicates, axis=1))
    chosen = res.group_subset_replicates[np.arange(n_boot), res.best_size_replicates]
    np.testing.assert_array_equal(res.best_inclusion_frequency, chosen.mean(axis=0))
    np.testing.assert_array_equal(res.best_size_frequency, np.bincount(res.best_size_replicates, minlength=g + 1) / n_boot)
    np.testing.assert_array_equal(res.reselected,
                                  (res.group_subset_replicates == point.group_subsets[None]).all(axis=2).mean(axis=0))
    assert res.reselected[0] == res.reselected[g] == 1.0 and res.best_size_frequency.sum() == 1.0


def test_more_than_32_columns_are_taken():
    labels = labels_of([11, 11, 11], 1, seed=8)     # p = 34
    res = ls_spa_best_group_subsets_bootstrap(*data(34, n=150, m=110, seed=72), labels, n_boot=2,
                                              _engine=GroupBootBestOracleEngine())
    assert res.subsets.shape == (4, 34) and res.group_subset_replicates.shape == (2, 4, 3)


def test_a_failed_replicate_is_nan_false_left_out_and_warned_about():
    n_boot = 5
    d = data(6, n=30, m=20, seed=5)
    good = ls_spa_best_group_subsets_bootstrap(*d, LABELS, n_boot=n_boot, _engine=GroupBootBestOracleEngine())
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        res = ls_spa_best_group_subsets_bootstrap(*d, LABELS, n_boot=n_boot, _engine=GroupBootBestOracleEngine(fail=(2,)))
    assert len(seen) == 1 and issubclass(seen[0].category, RuntimeWarning) and seen[0].filename == __file__
    assert "1 of 5 bootstrap replicates had a Gram matrix that was not numerically positive definite" in str(seen[0].message)
    keep = [0, 1, 3, 4]
    assert res.n_failed == 1 and np.isnan(res.r_squared_replicates[2]).all() and not res.group_subset_replicates[2].any()
    assert res.best_size_replicates[2] == -1 and np.isnan(res.full_r_squared_replicates[2])
    assert np.isnan(res.baseline_r_squared_replicates[2])
    np.testing.assert_array_equal(res.group_subset_replicates[keep], good.group_subset_replicates[keep])
    np.testing.assert_array_equal(res.inclusion_frequency, good.group_subset_replicates[keep].mean(axis=0))
    np.testing.assert_array_equal(res.best_size_frequency,
                                  np.bincount(good.best_size_replicates[keep], minlength=4) / 4)
    with pytest.raises(RuntimeError, match="3 of 5 bootstrap replicates"):
        ls_spa_best_group_subsets_bootstrap(*d, LABELS, n_boot=n_boot, _engine=GroupBootBestOracleEngine(fail=(0, 2, 4)))


def test_the_point_estimates_warning_is_this_calls():
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        ls_spa_best_group_subsets_bootstrap(*data(6, n=30, m=20, seed=2), LABELS, n_boot=2,
                                            _engine=GroupBootBestOracleEngine(info=1))
    assert len(seen) == 1 and "not numerically positive definite" in str(seen[0].message)
    assert seen[0].filename == __file__


def test_weights_and_a_side_that_is_not_resampled(monkeypatch):
    n, m = 20, 15
    d = data(6, n=n, m=m, seed=6)
    rng = np.random.default_rng(0)
    wa, we = rng.integers(1, 4, size=(4, n)).astype(float), rng.integers(1, 4, size=(4, m)).astype(float)
    eng = GroupBootBestOracleEngine()
    both = ls_spa_best_group_subsets_bootstrap(*d, LABELS, n_boot=4, weights=(wa, we), _engine=eng)
    assert ("boot_groups_best_run", 4, 0, True, True) in eng.log
    eng = GroupBootBestOracleEngine()
    ones = ls_spa_best_group_subsets_bootstrap(*d, LABELS, n_boot=4, weights=(wa, np.ones((4, m))), _engine=eng)
    monkeypatch.setattr(_driver, "BOOT_ONES_BYTES", 8 * m * 3)        # three replicates of ones a call
    eng = GroupBootBestOracleEngine()
    train = ls_spa_best_group_subsets_bootstrap(*d, LABELS, n_boot=4, weights=(wa, None), resample="train", _engine=eng)
    runs = [e for e in eng.log if e[0] == "boot_groups_best_run"]
    assert runs == [("boot_groups_best_run", 3, 0, True, True), ("boot_groups_best_run", 1, 3, True, True)]
    np.testing.assert_array_equal(train.group_subset_replicates, ones.group_subset_replicates)
    np.testing.assert_array_equal(train.r_squared_replicates, ones.r_squared_replicates)
    np.testing.assert_array_equal(train.baseline_r_squared_replicates, ones.baseline_r_squared_replicates)
    assert both.group_subset_replicates.shape == train.group_subset_replicates.shape


def _zero_y(d):
    return d[0], d[1], d[2], np.zeros_like(d[3])


L4 = [0, 0, 1, 1]


@pytest.mark.parametrize("make, groups, kw, error, text", [
    (lambda: data(65, n=140, m=100, seed=1), np.arange(65) % 8, {}, ValueError, "at most p = 64"),
    (lambda: data(40, n=100, m=80, seed=1), np.minimum(np.arange(40), 32), {}, ValueError, "at most g = 32"),
    (lambda: data(4), [0, 2, 2, 0], {}, ValueError, "gap in its numbering.*label 1"),
    (lambda: data(4), [0, -2, 1, 1], {}, ValueError, "below -1"),
    (lambda: data(4), [-1, -1, -1, -1], {}, ValueError, "no group at all"),
    (lambda: data(4), [0, 1, 1], {}, ValueError, "length p = 4"),
    (lambda: data(4), [0.0, 1.0, 1.0, 0.0], {}, ValueError, "integer labels"),
    (lambda: _zero_y(data(4)), L4, {}, ValueError, "identically zero"),
    (lambda: data(4), L4, dict(n_boot=1), ValueError, "n_boot must be an integer >= 2"),
    (lambda: data(4), L4, dict(n_boot=2.5), ValueError, "n_boot must be an integer >= 2"),
    (lambda: data(4), L4, dict(resample="rows"), ValueError, "resample must name"),
    (lambda: data(4), L4, dict(resample=()), ValueError, "resample must name"),
    (lambda: data(4), L4, dict(n_boot=3, weights=(np.ones((3, 7)), None)), ValueError, "w_train must have shape"),
    (lambda: data(4), L4, dict(n_boot=3, weights=(None, -np.ones((3, data(4)[1].shape[0])))), ValueError,
     "w_test must be finite and >= 0"),
    (lambda: data(4), L4, dict(n_boot=3, weights=(np.zeros((3, data(4)[0].shape[0])), None)), ValueError, "sum to zero"),
    (lambda: data(4), L4, dict(weights=(None,)), ValueError, "weights must be a pair"),
    (lambda: (data(4)[0], data(5)[1]) + data(4)[2:], L4, {}, SizeIncompatible, None),
    (lambda: (data(4)[0][:-1],) + data(4)[1:], L4, {}, SizeIncompatible, None),
])
def test_refusals_come_before_any_engine_work(monkeypatch, make, groups, kw, error, text):
    def no_engine(*a, **k):
        raise AssertionError("an engine was acquired")
    monkeypatch.setattr(_driver, "_acquire_engine", no_engine)
    eng = GroupBootBestOracleEngine()
    with pytest.raises(error, match=text):
        ls_spa_best_group_subsets_bootstrap(*make(), groups, _engine=eng, **kw)
    assert eng.touched == 0 and eng.group_best_calls == [] and eng.log == []
    with pytest.raises(error, match=text):
        ls_spa_best_group_subsets_bootstrap(*make(), groups, **kw)      # no engine of the caller's: none is acquired either


def test_there_is_no_include():
    with pytest.raises(TypeError, match="include"):
        ls_spa_best_group_subsets_bootstrap(*data(4), L4, include=[0], _engine=GroupBootBestOracleEngine())


def test_the_call_frees_the_bootstrap_rows_on_success_and_on_failure():
    d = data(6, n=30, m=20, seed=4)
    eng = GroupBootBestOracleEngine()
    ls_spa_best_group_subsets_bootstrap(*d, LABELS, n_boot=2, _engine=eng)
    assert [e[0] for e in eng.log] == ["boot_load", "boot_groups_best_run", "boot_free"]
    assert eng.log[0] == ("boot_load", True)                     # the load that takes p <= 64

    class Broken(GroupBootBestOracleEngine):
        def boot_groups_best_run(self, *a, **k):
            self.log.append(("boot_groups_best_run",))
            raise RuntimeError("boom")

    eng = Broken()
    with pytest.raises(RuntimeError, match="boom"):
        ls_spa_best_group_subsets_bootstrap(*d, LABELS, n_boot=2, _engine=eng)
    assert [e[0] for e in eng.log] == ["boot_load", "boot_groups_best_run", "boot_free"]
