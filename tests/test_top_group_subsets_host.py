"""ls_spa_top_group_subsets: the n_best best sets of groups of every size -- CPU side.

The gaps of every case the GPU tests compare with the truth of tests/group_top_ref.py (no GPU assertion then meets a
near-tie); the exact-tie problem, whose ties straddle the cut under both numberings; what the layouts of those cases
reach, through the host-only planner lsspa_debug_groups_top_plan; and the driver's plumbing through a NumPy double of
the engine whose lists are that truth."""
import warnings
from math import comb

import numpy as np
import pytest

import best_ref as B
import group_best_ref as R
import group_top_ref as GT
import top_ref as T_
from ls_spa import SizeIncompatible, TopGroupSubsetsResults, _driver, ls_spa_best_subsets, ls_spa_top_group_subsets
from ls_spa._engine import GROUPS_TOP_PLAN_FIELDS, debug_groups_top_plan
from test_group_best_host import GroupBestOracleEngine
from test_groups_host import group_values, labels_of
from test_subsets_host import data, gram_problem

ALL = [(name, reg) for name in R.CASES for reg in R.REGS]


# ---- the truth ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, seed, T", GT.PLANTED_RUNS)
def test_planted_gaps(name, seed, T):
    _, labels, dk, vals, masks, gap = GT.planted_case(name, seed, T)
    g = int(labels.max()) + 1
    print(name, seed, T, "gap", gap)
    assert gap > 1e-6 and (dk > 0).any() and (dk < 0).any()
    assert np.isfinite(vals[1:g]).all() and vals[0, 0] == 0.0 and np.isnan(vals[0, 1:]).all()
    for k in range(g + 1):
        n = min(T, comb(g, k))
        assert (np.array([bin(int(m)).count("1") for m in masks[k, :n]]) == k).all()


@pytest.mark.parametrize("name, reg", ALL)
def test_every_gpu_case_has_distinct_neighbours(name, reg):
    _, labels, u = R.brute_case(name, reg)
    g = int(labels.max()) + 1
    gap = GT.neighbour_gap(u, g, 17)
    print(name, reg, "gap", gap)
    assert gap > 1e-8


def test_planted_groups_are_additive():
    labels = labels_of([2, 3, 1, 2, 2], 0, seed=3)
    d, dj, dk = GT.planted_groups(labels, 11)
    u = R.all_group_values(d, labels)
    bits = ((np.arange(32)[:, None] >> np.arange(5)) & 1).astype(bool)
    np.testing.assert_allclose(u, np.array([dk[b].sum() for b in bits]), rtol=0, atol=1e-13)
    assert abs(dj.sum() - dk.sum()) < 1e-15


# ---- the exact-tie problem ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", list(R.TIE_RUNS))
def test_ties_straddle_the_cut(run):
    _, _, u = R.tie_case(run)
    assert T_.ties_straddling_rank(u, 5, 1) == [1, 2]
    assert T_.ties_straddling_rank(u, 5, 2) == [1, 2, 3]
    assert T_.ties_straddling_rank(u, 5, 3) == [3, 4]


def test_tie_runs_list_different_masks():
    want = {"agree": [[1, 2], [3, 5], [7, 11]], "disagree": [[1, 4], [5, 17], [21, 7]]}
    for run in R.TIE_RUNS:
        _, tm, tc = T_.top_truth(R.tie_case(run)[2], 5, 2)
        assert tm[1:4].tolist() == want[run] and (tc[1:4] == 2).all()
        assert tm[1:4, 0].tolist() == R.tie_winners(run)


# ---- the plan hook -----------------------------------------------------------------------------------------------------
def all_plans():
    plans = {name: (R.case_labels(name), want) for name, want in R.PLAN.items()}
    plans.update(R.PLANTED)
    return plans


@pytest.mark.parametrize("T", [1, 4, 16])
@pytest.mark.parametrize("name", list(R.PLAN) + list(R.PLANTED))
def test_plan_of_every_case(name, T):
    labels, want = all_plans()[name]
    g = int(np.max(labels)) + 1
    got = debug_groups_top_plan(labels, T)
    assert tuple(got) == GROUPS_TOP_PLAN_FIELDS
    for key in ("gl", "gh", "ql", "nb", "units", "per", "launches"):
        assert got[key] == want[key], key
    assert got["units"] * got["per"] == 1 << got["gh"] and got["launches"] == -(-got["per"] // got["steps"])
    assert got["sizes"] == min(g, got["per"].bit_length() - 1 + got["gl"]) + 1 <= 25
    assert got["table_bytes"] == got["units"] * (g + 1) * (12 * T + 4)


def test_the_largest_plan_fits_the_kernels_lists():
    # 32 groups of 2: three low groups, gh = 29, per = 2^16 -- and the bound behind the 25: gh <= 31 over 8192 units
    q = debug_groups_top_plan(np.repeat(np.arange(32), 2), 16)
    assert q["gl"] == 3 and q["gh"] == 29 and q["per"] == 1 << 16 and q["sizes"] == 20
    assert q["table_bytes"] == 8192 * 33 * 196
    assert (19 - 1) + 6 + 1 == 25                # GROUPS_BEST_CLASSES - 1 + GROUPS_LOW_COLS + 1 (csrc/kernels.h)


@pytest.mark.parametrize("labels, T", [([0, 0, 2, 2], 4), ([-2, 0, 0, 1], 4), ([-1, -1, -1], 4), (np.arange(33), 4),
                                       (np.zeros(65, dtype=int), 4), ([0, 0, 1, 1], 0), ([0, 0, 1, 1], 17),
                                       ([0, 0, 1, 1], -1)])
def test_plan_refuses_what_the_call_refuses(labels, T):
    with pytest.raises(ValueError, match="lsspa_debug_groups_top_plan"):
        debug_groups_top_plan(labels, T)


# ---- driver plumbing on a test double -----------------------------------------------------------------------------------
class GroupTopOracleEngine(GroupBestOracleEngine):
    """GroupsOracleEngine (through the grouped selection's double) with the grouped top lists' entry point: top_truth of
    the oracle's u.  cut: counts are capped there (ranks a failed pivot took away)."""

    def __init__(self, cut=None, **kw):
        super().__init__(**kw)
        self.group_top_calls, self._cut = [], cut

    def all_group_values(self, labels):
        if self._values is not None:
            return np.asarray(self._values, dtype=np.float64)
        g = int(labels.max()) + 1
        return group_values(*self.gram(), self.y_norm_sq, labels, np.arange(1 << g))

    def groups_top(self, labels, n_best=10):
        assert isinstance(labels, np.ndarray) and labels.dtype == np.int32 and labels.shape == (self.p,)
        self.group_top_calls.append((labels.copy(), n_best))
        g = int(labels.max()) + 1
        u, masks, count = T_.top_truth(self.all_group_values(labels), g, n_best)
        if self._cut is not None:
            count = np.minimum(count, self._cut).astype(np.int32)
            for k in range(g + 1):
                u[k, count[k]:], masks[k, count[k]:] = np.nan, 0
        return u, masks, count, self._info


def test_result_shapes_and_fields():
    labels = labels_of([2, 3, 1, 2, 1], 2, seed=7)
    p, g, T = len(labels), 5, 4
    d = data(p, seed=70)
    eng = GroupTopOracleEngine()
    res = ls_spa_top_group_subsets(*d, labels, n_best=T, _engine=eng)
    assert isinstance(res, TopGroupSubsetsResults) and len(eng.group_top_calls) == 1 and eng.group_best_calls == []
    np.testing.assert_array_equal(eng.group_top_calls[0][0], labels)
    assert eng.group_top_calls[0][1] == T and eng.best_calls == []
    n = g + 1
    assert res.sizes.tolist() == list(range(n))
    assert res.n_models.tolist() == [min(T, comb(g, k)) for k in range(n)]
    assert res.group_subsets.shape == (n, T, g) and res.group_subsets.dtype == bool
    assert res.subsets.shape == (n, T, p) and res.subsets.dtype == bool and res.n_columns.shape == (n, T)
    assert res.r_squared.shape == res.gap.shape == (n, T) and res.theta.shape == (n, T, p)
    tv, tm, tc = T_.top_truth(eng.all_group_values(labels), g, T)
    np.testing.assert_array_equal(res.r_squared, tv)
    valid = np.arange(T)[None, :] < res.n_models[:, None]
    assert np.isnan(res.r_squared[~valid]).all() and np.isnan(res.theta[~valid]).all() and np.isnan(res.gap[~valid]).all()
    assert not res.subsets[~valid].any() and not res.group_subsets[~valid].any() and (res.n_columns[~valid] == 0).all()
    assert np.isfinite(res.theta[valid]).all()
    assert (res.group_subsets.sum(axis=2)[valid] == np.broadcast_to(res.sizes[:, None], valid.shape)[valid]).all()
    for k in range(n):
        for r in range(res.n_models[k]):
            assert B.mask_of(np.nonzero(res.group_subsets[k, r])[0]) == tm[k, r]
            np.testing.assert_array_equal(res.subsets[k, r], R.columns_of(labels, tm[k, r]))     # baseline + groups
            assert res.n_columns[k, r] == res.subsets[k, r].sum()
        assert (np.diff(res.r_squared[k, :res.n_models[k]]) <= 0).all()
    assert res.subsets[valid][:, labels < 0].all() and res.n_columns[0, 0] == 2 and res.n_columns[g, 0] == p
    assert (res.gap[:, 0] == 0.0).all() and (res.gap[valid] >= 0).all()
    np.testing.assert_array_equal(res.gap[valid], np.broadcast_to(tv[:, :1], tv.shape)[valid] - tv[valid])
    # rank 0 and best_* are the grouped selection's
    best = ls_spa_best_subsets(*d, groups=labels, _engine=GroupBestOracleEngine())
    assert res.best_size == best.best_size and res.full_r_squared == best.full_r_squared
    assert res.baseline_r_squared == best.baseline_r_squared == res.r_squared[0, 0]
    np.testing.assert_array_equal(res.best_group_subset, best.best_group_subset)
    np.testing.assert_array_equal(res.best_subset, best.best_subset)
    np.testing.assert_array_equal(res.group_subsets[:, 0], best.group_subsets)
    np.testing.assert_array_equal(res.subsets[:, 0], best.subsets)
    np.testing.assert_array_equal(res.n_columns[:, 0], best.n_columns)
    np.testing.assert_array_equal(res.r_squared[:, 0], best.r_squared)
    np.testing.assert_array_equal(res.theta[:, 0], best.theta)
    assert "next model" in repr(res) and "groups" in repr(res)


def test_theta_is_the_refit_with_exact_zeros():
    labels = labels_of([3, 1, 2, 2], 1, seed=5)
    p, g = len(labels), 4
    d = data(p, seed=5)
    res = ls_spa_top_group_subsets(*d, labels, reg=0.05, n_best=3, _engine=GroupTopOracleEngine())
    G, gv, H, h, yy = gram_problem(*d, reg=0.05)
    for k in range(g + 1):
        for r in range(res.n_models[k]):
            cols, out = np.nonzero(res.subsets[k, r])[0], np.nonzero(~res.subsets[k, r])[0]
            assert (res.theta[k, r, out] == 0.0).all() and not np.signbit(res.theta[k, r, out]).any()
            th = np.linalg.solve(G[np.ix_(cols, cols)], gv[cols])
            np.testing.assert_allclose(res.theta[k, r, cols], th, rtol=1e-9, atol=1e-12)
            r2 = (2.0 * th @ h[cols] - th @ H[np.ix_(cols, cols)] @ th) / yy
            assert abs(r2 - res.r_squared[k, r]) < 1e-12


def test_no_baseline_starts_at_zero():
    labels = labels_of([2, 2, 3], 0, seed=3)
    res = ls_spa_top_group_subsets(*data(7, seed=4), labels, _engine=GroupTopOracleEngine())
    assert res.r_squared[0, 0] == 0.0 and res.baseline_r_squared == 0.0 and not res.subsets[0].any()
    assert (res.theta[0, 0] == 0.0).all() and res.n_columns[0, 0] == 0 and res.n_models.tolist() == [1, 3, 3, 1]


def test_overall_list_is_the_merge_under_the_same_order():
    labels = np.array([0, 1, 1, 2])
    d = data(4, seed=2)
    u = np.array([0.0, 0.6, 0.1, 0.6, 0.2, 0.3, 0.1, 0.6])         # 0.6 at masks 1 (size 1), 3 (size 2), 7 (size 3)
    res = ls_spa_top_group_subsets(*d, labels, n_best=4, _engine=GroupTopOracleEngine(values=u))
    assert res.top_r_squared.tolist() == [0.6, 0.6, 0.6, 0.3]
    assert res.top_sizes.tolist() == [1, 2, 3, 2]                    # equal values: masks 1 < 3 < 7
    assert [B.mask_of(np.nonzero(s)[0]) for s in res.top_group_subsets] == [1, 3, 7, 5]
    for s, c in zip(res.top_group_subsets, res.top_subsets):
        np.testing.assert_array_equal(c, R.columns_of(labels, B.mask_of(np.nonzero(s)[0])))
    assert res.best_size == 1                                        # the smallest size of equal maxima
    res = ls_spa_top_group_subsets(*d, labels, n_best=16, _engine=GroupTopOracleEngine(values=u))
    assert len(res.top_sizes) == 8 and res.top_group_subsets.shape == (8, 3) and res.top_subsets.shape == (8, 4)
    order = np.lexsort((np.arange(8), -u))
    assert [B.mask_of(np.nonzero(s)[0]) for s in res.top_group_subsets] == order.tolist()
    np.testing.assert_array_equal(res.top_r_squared, u[order])
    # a larger problem: the overall list from all 2^g values
    labels = labels_of([2, 1, 3, 1, 2, 2, 1], 1, seed=9)
    eng = GroupTopOracleEngine()
    res = ls_spa_top_group_subsets(*data(len(labels), seed=9), labels, n_best=6, _engine=eng)
    ua = eng.all_group_values(labels)
    order = np.lexsort((np.arange(1 << 7), -ua))[:6]
    assert [B.mask_of(np.nonzero(s)[0]) for s in res.top_group_subsets] == order.tolist()
    np.testing.assert_array_equal(res.top_r_squared, ua[order])
    assert res.top_sizes.tolist() == B.popcounts(7)[order].tolist()


def test_more_than_32_columns_are_taken():
    labels = labels_of([5] * 7, 1, seed=8)     # p = 36
    res = ls_spa_top_group_subsets(*data(36, n=150, m=110, seed=72), labels, n_best=2, _engine=GroupTopOracleEngine())
    assert res.subsets.shape == (8, 2, 36) and res.n_columns[:, 0].tolist() == [1 + 5 * k for k in range(8)]
    assert res.n_models.tolist() == [1, 2, 2, 2, 2, 2, 2, 1]


def test_failed_pivots_warn_and_leave_nan_ranks():
    labels = np.array([0, 1, 1, 2])
    d = data(4, seed=2)
    u = np.array([0.0, 0.6, 0.1, 0.6, 0.2, 0.3, 0.1, 0.9])
    with pytest.warns(RuntimeWarning, match="not numerically positive definite"):
        res = ls_spa_top_group_subsets(*d, labels, n_best=2,
                                       _engine=GroupTopOracleEngine(values=u, info=1, cut=[1, 2, 1, 0]))
    assert res.n_models.tolist() == [1, 2, 1, 0] and np.isnan(res.r_squared[3]).all() and res.best_size == 1
    assert np.isnan(res.r_squared[2, 1]) and np.isnan(res.gap[2, 1]) and np.isnan(res.theta[3]).all()
    assert not res.subsets[3].any() and not res.group_subsets[3].any() and (res.n_columns[3] == 0).all()
    with pytest.warns(RuntimeWarning):
        res = ls_spa_top_group_subsets(*d, labels, n_best=2,
                                       _engine=GroupTopOracleEngine(values=u, info=1, cut=[0, 0, 0, 0]))
    assert res.best_size == -1 and not res.best_subset.any() and not res.best_group_subset.any()
    assert len(res.top_sizes) == 0 and np.isnan(res.baseline_r_squared)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        ls_spa_top_group_subsets(*data(5, seed=2), [0, 0, 1, 1, -1], _engine=GroupTopOracleEngine(info=1))
    assert len(seen) == 1 and issubclass(seen[0].category, RuntimeWarning) and seen[0].filename == __file__
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ls_spa_top_group_subsets(*data(5, seed=2), [0, 0, 1, 1, -1], _engine=GroupTopOracleEngine())


def _zero_y(d):
    return d[0], d[1], d[2], np.zeros_like(d[3])


G4 = [0, 0, 1, 1]


@pytest.mark.parametrize("make, groups, kw, error, text", [
    (lambda: data(65, n=140, m=100, seed=1), np.arange(65) % 8, {}, ValueError, "at most p = 64"),
    (lambda: data(40, n=100, m=80, seed=1), np.minimum(np.arange(40), 32), {}, ValueError, "at most g = 32"),
    (lambda: data(4), [0, 2, 2, 0], {}, ValueError, "gap in its numbering.*label 1"),
    (lambda: data(4), [0, -2, 1, 1], {}, ValueError, "below -1"),
    (lambda: data(4), [-1, -1, -1, -1], {}, ValueError, "no group at all"),
    (lambda: data(4), [0, 1, 1], {}, ValueError, "length p = 4"),
    (lambda: data(4), [0.0, 1.0, 1.0, 0.0], {}, ValueError, "integer labels"),
    (lambda: data(4), G4, dict(n_best=0), ValueError, "integer in 1 .. 16"),
    (lambda: data(4), G4, dict(n_best=17), ValueError, "integer in 1 .. 16"),
    (lambda: data(4), G4, dict(n_best=2.0), ValueError, "integer in 1 .. 16"),
    (lambda: data(4), G4, dict(n_best=True), ValueError, "integer in 1 .. 16"),
    (lambda: data(4), G4, dict(n_best=None), ValueError, "integer in 1 .. 16"),
    (lambda: data(4), G4, dict(include=[0]), TypeError, "include"),
    (lambda: _zero_y(data(4)), G4, {}, ValueError, "identically zero"),
    (lambda: (data(4)[0], data(5)[1]) + data(4)[2:], G4, {}, SizeIncompatible, None),
    (lambda: (data(4)[0][:-1],) + data(4)[1:], G4, {}, SizeIncompatible, None),
])
def test_refusals_come_before_any_engine_work(monkeypatch, make, groups, kw, error, text):
    def no_engine(*a, **k):
        raise AssertionError("an engine was acquired")
    monkeypatch.setattr(_driver, "_acquire_engine", no_engine)
    eng = GroupTopOracleEngine()
    with pytest.raises(error, match=text):
        ls_spa_top_group_subsets(*make(), groups, _engine=eng, **kw)
    assert eng.touched == 0 and eng.group_top_calls == [] and eng.group_best_calls == []
    with pytest.raises(error, match=text):
        ls_spa_top_group_subsets(*make(), groups, **kw)          # no engine of the caller's: none is acquired either


def test_numpy_integer_n_best_and_a_kept_engine_back_to_float64():
    class Float32Engine(GroupTopOracleEngine):
        precision = "float32"

        def set_precision(self, dtype):
            self.precision = np.dtype(dtype).name

        def full_fit(self):
            assert self.precision == "float64", "full fit with fp32 factorisation"
            return super().full_fit()

    eng = Float32Engine()
    res = ls_spa_top_group_subsets(*data(6, seed=3), [0, 0, 1, 1, -1, 2], n_best=np.int64(3), _engine=eng)
    assert eng.precision == "float64" and res.r_squared.shape == (4, 3) and eng.group_top_calls[0][1] == 3
