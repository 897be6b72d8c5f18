"""The host side of ls_spa_bootstrap(groups=), without a GPU: the argument checks that need no engine, the grouped block
planner (lsspa_debug_boot_groups_plan) and the summaries of BootstrapResults over groups."""
import numpy as np
import pytest

from ls_spa import BootstrapResults, ls_spa_bootstrap
from ls_spa._engine import debug_boot_groups_plan, debug_boot_plan
from test_groups_host import labels_of
from test_subsets_host import data


class NoEngine:
    def __getattr__(self, name):
        raise AssertionError(f"the engine was asked for {name} before the arguments were checked")


def call(d, groups, **k):
    return ls_spa_bootstrap(*d, groups=groups, _engine=NoEngine(), **k)


def test_argument_checks_need_no_engine():
    with pytest.raises(ValueError, match="at most p = 64 columns"):
        call(data(65, n=80, m=80, seed=1), labels_of([13] * 5))
    d = data(40, n=60, m=60, seed=2)
    with pytest.raises(ValueError, match="at most g = 32 groups"):
        call(d, labels_of([1] * 33, 7))
    bad = labels_of([5] * 8)
    bad[3] = -2
    with pytest.raises(ValueError, match="below -1"):
        call(d, bad)
    gap = labels_of([5] * 8)
    gap[gap == 2] = 3                                        # group 2 is empty
    with pytest.raises(ValueError, match="no column carries label 2"):
        call(d, gap)
    with pytest.raises(ValueError, match="one label per column"):
        call(d, labels_of([5] * 7))
    # the other options are checked as without groups, still before any engine call
    with pytest.raises(ValueError, match="n_boot"):
        call(d, labels_of([5] * 8), n_boot=1)
    # and without groups nothing has moved: p = 40 is still refused with the advice to group
    with pytest.raises(ValueError, match="at most p = 32.*group the columns"):
        ls_spa_bootstrap(*d, _engine=NoEngine())


def test_grouped_planner():
    """cb and rpw by the columns, blocks by memory, slices by the rows alone, launches within 2^20 workgroups."""
    got = {p: debug_boot_groups_plan(10, 100, 100, labels_of([p // 4] * 3 + [p - 3 * (p // 4)])) for p in (47, 48, 63, 64)}
    assert [got[p]["cb"] for p in (47, 48, 63, 64)] == [3, 4, 4, 5]
    assert [got[p]["rpw"] for p in (47, 48, 63, 64)] == [2, 1, 1, 1]
    assert [got[p]["pairs"] for p in (47, 48, 63, 64)] == [6, 10, 10, 15]
    assert all(v["ldz"] == 16 * v["cb"] for v in got.values())
    for sizes, base in (([2] * 20 + [4] * 6, 0), ([2] * 32, 0), ([8] * 8, 0), ([10, 20, 30], 4), ([1, 1, 1], 0)):
        labels = labels_of(sizes, base, seed=1)
        g = len(sizes)
        for R, n, m in ((1000, 10 ** 5, 10 ** 5), (7, 513, 77), (5, 2 ** 31 - 1, 3)):
            for block in (0, 1, 3, 10 ** 6):
                a = debug_boot_groups_plan(R, n, m, labels, block)
                assert a["block"] == 1 or a["block"] * a["rep_bytes"] <= 256 << 20
                assert 1 <= a["block"] <= min(R, 1024) and (block == 0 or a["block"] <= block)
                assert a["n_blocks"] == -(-R // a["block"])
                # the slices are those of the ungrouped plan for the same rows
                b = debug_boot_plan(R, n, m, 16, block)
                for k in ("rps_train", "rps_test", "slices_train", "slices_test"):
                    assert a[k] == b[k], k
                assert a["units"] * a["enum_reps"] <= 1 << 20 and 1 <= a["enum_reps"] <= a["block"]
                assert a["units"] <= 8192 and 1 <= a["steps"] <= a["per"]
                # units * per = 2^gh and a partial table g + 1 wide: the layout's high groups (all but the smallest
                # ones, whose columns total at most six)
                low, cols = 0, 0
                for s in sorted(sizes):
                    if cols + s > 6:
                        break
                    low, cols = low + 1, cols + s
                assert a["units"] * a["per"] == 1 << (g - low)
                c = len(labels) + 1
                assert a["rep_bytes"] == 8 * (n + m) + (a["slices_train"] + a["slices_test"]) * a["pairs"] * 2048 + \
                    a["units"] * (g + 1) * 8 + 64 * c * c
    big = debug_boot_groups_plan(1000, 10 ** 5, 10 ** 5, labels_of([2] * 20 + [4] * 6))     # 2^23 high subsets
    # a subset's matrix has 6 low columns + the right-hand side and on average half of the 58 high ones (+ 1, rounded
    # down): 36 rows, so a launch takes 2^26 // 36^2 = 51781 subsets: 6 steps of the 8192 units, as the one-problem call
    # cuts them, and then no room for a second replicate
    assert big["units"] == 8192 and big["per"] == 1 << 10 and big["steps"] == (2 ** 26 // 36 ** 2) // 8192 == 6
    assert big["enum_reps"] == 1


def test_the_cut_into_launches_depends_on_the_layout_alone():
    """A unit's row of the partial table is the sum of its launches' sums: `steps` must not move with R, the block or
    the rows, or the bits of a replicate would."""
    for sizes in ([1] * 20, [2] * 20 + [4] * 6, [4] * 4 + [3] * 16, [5] * 8):
        labels = labels_of(sizes)
        seen = {(debug_boot_groups_plan(R, n, n, labels, block)["steps"], debug_boot_groups_plan(R, n, n, labels, block)["per"])
                for R in (1, 2, 7, 22, 1000) for block in (0, 1, 3, 21) for n in (50, 10 ** 5)}
        assert len(seen) == 1, (sizes, seen)
    # 20 singletons: 2^14 high subsets, two a unit, both in one launch (2^26 // 14^2 // 8192 = 41 steps would fit)
    a = debug_boot_groups_plan(22, 300, 300, labels_of([1] * 20))
    assert (a["units"], a["per"], a["steps"]) == (8192, 2, 2) and a["enum_reps"] == 20      # 41 // 2 replicates
    # p = 64 in 20 groups: 2^18 high subsets, 32 a unit, 6 a launch: six launches
    a = debug_boot_groups_plan(7, 300, 300, labels_of([4] * 4 + [3] * 16))
    assert (a["units"], a["per"], a["steps"], a["enum_reps"]) == (8192, 32, 6, 1)


def test_grouped_planner_refusals():
    ok = labels_of([5] * 8)
    assert debug_boot_groups_plan(1, 5, 5, ok)["cb"] == 3
    for bad in ((0, 5, 5, ok, 0), (1, 0, 5, ok, 0), (1, 5, 2 ** 31, ok, 0), (1, 5, 5, ok, -1),
                (1, 5, 5, labels_of([13] * 5), 0),                       # p = 65
                (1, 5, 5, labels_of([1] * 33, 7), 0),                    # g = 33
                (1, 5, 5, np.full(10, -1), 0),                           # no group at all
                (1, 5, 5, np.array([0, 0, 2, 2]), 0),                    # an empty group
                (1, 5, 5, np.array([0, -2, 1]), 0), (1, 5, 5, np.zeros(0, dtype=np.int32), 0)):
        with pytest.raises(ValueError):
            debug_boot_groups_plan(*bad)
    # the ungrouped planner answers as before: p = 33 is refused there
    with pytest.raises(ValueError):
        debug_boot_plan(1, 5, 5, 33)
    assert debug_boot_plan(1, 5, 5, 32)["cb"] == 3


def test_results_summaries_over_groups():
    g, p = 3, 7
    rep = np.array([[1.0, 5.0, 2.0], [2.0, 4.0, 2.0], [9.0, 9.0, 9.0], [3.0, 3.0, 2.5], [4.0, 2.0, 3.0]])
    base = np.array([0.1, 0.2, 0.3, 0.4, 0.5])
    r2 = rep.sum(axis=1) + base
    failed = np.array([False, False, True, False, False])
    res = BootstrapResults.from_replicates(np.zeros(g), np.ones(p), 0.5, rep, r2, failed, 0.5, base)
    ok = rep[~failed]
    assert res.theta.shape == (p,) and res.attribution.shape == (g,) and res.replicates.shape == (5, g)
    assert res.std_error.shape == res.lower.shape == res.upper.shape == (g,) and res.prob_greater.shape == (g, g)
    np.testing.assert_array_equal(res.lower, np.quantile(ok, 0.25, axis=0))
    np.testing.assert_array_equal(res.upper, np.quantile(ok, 0.75, axis=0))
    assert res.prob_greater[0, 1] == 0.25 and res.prob_greater[1, 0] == 0.5
    assert np.isnan(res.baseline_r_squared_replicates[2]) and base[2] == 0.3          # masked in a copy
    np.testing.assert_array_equal(res.baseline_r_squared_replicates[~failed], base[~failed])
    np.testing.assert_allclose(res.replicates[~failed].sum(axis=1),
                               (res.r_squared_replicates - res.baseline_r_squared_replicates)[~failed], atol=1e-15)
    # without groups the field is None and the positional signature is the old one
    plain = BootstrapResults.from_replicates(np.zeros(g), np.ones(g), 0.5, rep, r2, failed, 0.5)
    assert plain.baseline_r_squared_replicates is None
