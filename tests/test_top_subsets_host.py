"""ls_spa_top_subsets: the n_best best subsets of every size -- CPU side.

The truth of tests/top_ref.py on hand-made values (ties, fewer candidates than ranks), against best_ref's arg-max and
against its own additive search; the integer design's exact ties; the cases the GPU tests take from the search (their
gaps, the launches and units their winners come from); the plan hook; and the driver's plumbing through a NumPy double
of the engine whose lists are that truth."""
import warnings
from math import comb

import numpy as np
import pytest

import best_ref as B
import top_ref as T_
from ls_spa import SizeIncompatible, TopSubsetsResults, _driver, ls_spa_best_subsets, ls_spa_top_subsets
from ls_spa._engine import debug_subsets_top_plan
from test_best_subsets_host import BestOracleEngine
from test_subsets_host import data, gram_problem, subset_values


# ---- the truth ---------------------------------------------------------------------------------------------------------
def test_truth_ties_and_short_lists():
    v = np.array([0.0, 0.5, 0.5, 0.2, 0.5, 0.7, 0.7, 0.1])          # p = 3; sizes: {0} {1,2,4} {3,5,6} {7}
    tv, tm, tc = T_.top_truth(v, 3, 2)
    assert tc.tolist() == [1, 2, 2, 1]
    assert tm.tolist() == [[0, 0], [1, 2], [5, 6], [7, 0]]           # equal values: the smaller mask first
    assert tv[1].tolist() == [0.5, 0.5] and tv[2].tolist() == [0.7, 0.7] and tv[0, 0] == 0.0 and np.isnan(tv[0, 1])
    tv, tm, tc = T_.top_truth(v, 3, 4)
    assert tc.tolist() == [1, 3, 3, 1] and tm[1].tolist() == [1, 2, 4, 0] and tm[2].tolist() == [5, 6, 3, 0]
    assert np.isnan(tv[1, 3]) and tv[2, :3].tolist() == [0.7, 0.7, 0.2]
    tv, tm, tc = T_.top_truth(v, 3, 2, include=0b010)
    assert tc.tolist() == [0, 1, 2, 1] and tm.tolist() == [[0, 0], [2, 0], [6, 3], [7, 0]]
    valid = np.ones(8, dtype=bool)
    valid[[5, 7]] = False
    tv, tm, tc = T_.top_truth(v, 3, 2, valid=valid)
    assert tc.tolist() == [1, 2, 2, 0] and tm[2].tolist() == [6, 3]
    w = v.copy()
    w[6] = np.nan                                                    # NaN is never listed
    assert T_.top_truth(w, 3, 3)[1][2].tolist() == [5, 3, 0]


@pytest.mark.parametrize("p, reg", [(5, 0.0), (9, 0.1), (12, 0.0)])
def test_rank_0_is_the_best_subset(p, reg):
    _, v = B.brute_case(p, reg)
    for inc in (0, 0b101):
        best, masks, found, _ = B.best_truth(v, p, inc)
        tv, tm, tc = T_.top_truth(v, p, 3, inc)
        np.testing.assert_array_equal(tc > 0, found)
        np.testing.assert_array_equal(tm[:, 0], masks)
        np.testing.assert_array_equal(tv[found, 0], best[found])
        size = B.popcounts(p)
        for k in range(p + 1):
            want = min(3, comb(p - 2, k - 2) if inc and k >= 2 else (0 if inc else comb(p, k)))
            assert tc[k] == want and (size[tm[k, :tc[k]]] == k).all()
            assert (np.diff(tv[k, :tc[k]]) <= 0).all()


@pytest.mark.parametrize("p, seed", [(6, 1), (9, 2), (12, 3)])
def test_additive_search_against_the_brute_force(p, seed):
    d = T_.generic_worths(p, seed)
    m = np.arange(1 << p, dtype=np.uint64)
    bits = ((m[:, None] >> np.arange(p, dtype=np.uint64)) & np.uint64(1)).astype(bool)
    v_all = np.array([d[b].sum() for b in bits])
    tv, tm, tc = T_.top_truth(v_all, p, 16)
    for k in range(p + 1):
        v, masks = T_.additive_top(d, k, 16)
        assert len(v) == tc[k] == min(16, comb(p, k))
        np.testing.assert_array_equal(masks, tm[k, :tc[k]])
        np.testing.assert_allclose(v, tv[k, :tc[k]], rtol=0, atol=1e-14)


# ---- the integer design --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [9, 12])
def test_integer_design_ties_are_exact_and_straddle_the_cut(p):
    d = T_.integer_design(p)
    G, g, H, h, yy = gram_problem(*d)
    np.testing.assert_array_equal(G, np.eye(p) / 16.0)
    np.testing.assert_array_equal(H, np.eye(p))
    w = T_.integer_values(p)
    v = subset_values(G, g, H, h, yy, np.arange(1 << p, dtype=np.uint64))
    # one value per integer worth, to the bit, in the same order
    for worth in np.unique(w):
        assert len(np.unique(v[w == worth])) == 1
    assert (np.diff(v[np.argsort(w, kind="stable")]) >= 0).all()
    assert T_.top_truth(v, p, 16)[1].tolist() == T_.top_truth(w, p, 16)[1].tolist()
    worth = T_.INT_WORTH[p]
    lo, hi = range(6), range(6, p)
    assert any(worth[i] == worth[j] for i in lo for j in lo if i < j)
    assert any(worth[i] == worth[j] for i in lo for j in hi)
    assert any(worth[i] == worth[j] for i in hi for j in hi if i < j)
    for T in (3, 16):
        assert len(T_.ties_straddling_rank(w, p, T)) > 0


# ---- the planted cases of the GPU tests ------------------------------------------------------------------------------------
def test_planted_p28_winners_span_launches_and_units():
    p, T = 28, 4
    _, d, vals, masks, gap = T_.planted_case(p, T, 2801)
    assert gap > 1e-8 and (d > 0).any() and (d < 0).any()
    plan = debug_subsets_top_plan(p, T)
    assert plan["launches"] > 1 and plan["units"] * plan["per"] == 1 << (p - 6)
    per_bits = plan["per"].bit_length() - 1
    listed = masks[np.isfinite(vals)].astype(np.int64)
    step = (listed >> 6) & ((1 << per_bits) - 1)
    units = listed >> (6 + per_bits)
    launch = step // plan["steps"]
    assert len(np.unique(units)) > 8 and launch.min() == 0 and launch.max() == plan["launches"] - 1
    assert step.min() < plan["per"] // 4 and step.max() >= 3 * plan["per"] // 4


def test_planted_p32_lists_with_and_without_the_last_feature():
    _, _, vals, masks, gap = T_.planted_case(32, 2, 3201)
    assert gap > 1e-8
    listed = masks[np.isfinite(vals)]
    assert (listed >> 31).any() and not (listed >> 31).all()


# ---- the plan hook -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [1, 5, 6, 7, 20, 28, 32])
@pytest.mark.parametrize("T", [1, 4, 16])
def test_plan(p, T):
    plan = debug_subsets_top_plan(p, T)
    q = min(p, 6)
    units = min(1 << (p - q), 8192)
    per = (1 << (p - q)) // units
    steps = max(1, (1 << 20) // units)
    assert plan["units"] == units and plan["per"] == per and plan["units"] * plan["per"] == 1 << (p - q)
    assert plan["steps"] == steps and plan["launches"] == -(-per // steps)
    assert plan["sizes"] == min(p, per.bit_length() - 1 + q) + 1 <= 20
    assert plan["table_bytes"] == units * (p + 1) * (12 * T + 4)
    assert plan["reduce_rounds"] == T
    if p == 32 and T == 16:
        assert plan["launches"] == 64 and plan["table_bytes"] == 8192 * 33 * 196


@pytest.mark.parametrize("p, T", [(0, 4), (33, 4), (12, 0), (12, 17), (12, -1)])
def test_plan_refusals(p, T):
    with pytest.raises(ValueError, match="lsspa_debug_subsets_top_plan"):
        debug_subsets_top_plan(p, T)


# ---- driver plumbing on a test double -----------------------------------------------------------------------------------
class TopOracleEngine(BestOracleEngine):
    """BestOracleEngine with the top-subsets entry point, computed by top_truth.  cut: counts are capped there (ranks a
    failed pivot took away)."""

    def __init__(self, cut=None, **kw):
        super().__init__(**kw)
        self.top_calls, self._cut = [], cut

    def all_values(self):
        if self._values is not None:
            return np.asarray(self._values, dtype=np.float64)
        return subset_values(*self.gram(), self.y_norm_sq, np.arange(1 << self.p, dtype=np.uint64))

    def subsets_top(self, include=0, n_best=10):
        self.top_calls.append((include, n_best))
        v, masks, count = T_.top_truth(self.all_values(), self.p, n_best, include)
        if self._cut is not None:
            count = np.minimum(count, self._cut).astype(np.int32)
            for k in range(self.p + 1):
                v[k, count[k]:], masks[k, count[k]:] = np.nan, 0
        return v, masks, count, self._info


def test_result_shapes_and_fields():
    p, T = 7, 5
    d = data(p, seed=3)
    eng = TopOracleEngine()
    res = ls_spa_top_subsets(*d, n_best=T, _engine=eng)
    assert isinstance(res, TopSubsetsResults) and eng.top_calls == [(0, T)] and eng.best_calls == []
    assert res.sizes.tolist() == list(range(p + 1))
    assert res.n_models.tolist() == [min(T, comb(p, k)) for k in range(p + 1)]
    assert res.subsets.shape == (p + 1, T, p) and res.subsets.dtype == bool
    assert res.r_squared.shape == res.gap.shape == (p + 1, T) and res.theta.shape == (p + 1, T, p)
    tv, tm, tc = T_.top_truth(eng.all_values(), p, T)
    np.testing.assert_array_equal(res.r_squared, tv)
    valid = np.arange(T)[None, :] < res.n_models[:, None]
    assert np.isnan(res.r_squared[~valid]).all() and np.isnan(res.theta[~valid]).all() and not res.subsets[~valid].any()
    assert np.isnan(res.gap[~valid]).all() and np.isfinite(res.theta[valid]).all()
    assert (res.subsets.sum(axis=2)[valid] == np.broadcast_to(res.sizes[:, None], valid.shape)[valid]).all()
    for i in range(p + 1):
        for r in range(res.n_models[i]):
            assert B.mask_of(np.nonzero(res.subsets[i, r])[0]) == tm[i, r]
        assert (np.diff(res.r_squared[i, :res.n_models[i]]) <= 0).all()
    assert (res.gap[:, 0] == 0.0).all() and (res.gap[valid] >= 0).all()
    np.testing.assert_array_equal(res.gap[valid], np.broadcast_to(tv[:, :1], tv.shape)[valid] - tv[valid])
    best = ls_spa_best_subsets(*d, _engine=BestOracleEngine())
    assert res.best_size == best.best_size and res.full_r_squared == best.full_r_squared
    np.testing.assert_array_equal(res.best_subset, best.best_subset)
    np.testing.assert_array_equal(res.subsets[:, 0], best.subsets)
    np.testing.assert_array_equal(res.r_squared[:, 0], best.r_squared)
    np.testing.assert_array_equal(res.theta[:, 0], best.theta)
    assert "next model" in repr(res)


def test_theta_is_the_refit_with_exact_zeros():
    p = 6
    d = data(p, seed=5)
    res = ls_spa_top_subsets(*d, reg=0.05, n_best=3, _engine=TopOracleEngine())
    G, g, H, h, yy = gram_problem(*d, reg=0.05)
    for i in range(p + 1):
        for r in range(res.n_models[i]):
            cols, out = np.nonzero(res.subsets[i, r])[0], np.nonzero(~res.subsets[i, r])[0]
            assert (res.theta[i, r, out] == 0.0).all() and not np.signbit(res.theta[i, r, out]).any()
            if len(cols):
                th = np.linalg.solve(G[np.ix_(cols, cols)], g[cols])
                np.testing.assert_allclose(res.theta[i, r, cols], th, rtol=1e-9, atol=1e-12)
                r2 = (2.0 * th @ h[cols] - th @ H[np.ix_(cols, cols)] @ th) / yy
                assert abs(r2 - res.r_squared[i, r]) < 1e-12


def test_overall_list_is_the_merge_under_the_same_order():
    p = 3
    d = data(p, seed=2)
    v = np.array([0.0, 0.6, 0.1, 0.6, 0.2, 0.3, 0.1, 0.6])         # 0.6 at masks 1 (size 1), 3 (size 2), 7 (size 3)
    res = ls_spa_top_subsets(*d, n_best=4, _engine=TopOracleEngine(values=v))
    assert res.top_r_squared.tolist() == [0.6, 0.6, 0.6, 0.3]
    assert res.top_sizes.tolist() == [1, 2, 3, 2]                    # equal values: masks 1 < 3 < 7
    assert [B.mask_of(np.nonzero(s)[0]) for s in res.top_subsets] == [1, 3, 7, 5]
    assert res.best_size == 1                                        # ls_spa_best_subsets': the smallest size of equal maxima
    res = ls_spa_top_subsets(*d, n_best=16, _engine=TopOracleEngine(values=v))
    assert len(res.top_sizes) == 8 and res.top_subsets.shape == (8, p)
    order = np.lexsort((np.arange(8), -v))
    assert [B.mask_of(np.nonzero(s)[0]) for s in res.top_subsets] == order.tolist()
    np.testing.assert_array_equal(res.top_r_squared, v[order])
    # a larger problem: the overall list from all 2^p values
    p = 8
    eng = TopOracleEngine()
    res = ls_spa_top_subsets(*data(p, seed=9), n_best=6, _engine=eng)
    va = eng.all_values()
    order = np.lexsort((np.arange(1 << p), -va))[:6]
    assert [B.mask_of(np.nonzero(s)[0]) for s in res.top_subsets] == order.tolist()
    np.testing.assert_array_equal(res.top_r_squared, va[order])
    assert res.top_sizes.tolist() == B.popcounts(p)[order].tolist()


@pytest.mark.parametrize("make", [lambda: [2], lambda: (5, 0), lambda: np.array([1, 3, 4]), lambda: range(6)])
def test_include_shifts_the_sizes(make):
    p, T = 6, 4
    d = data(p, seed=8)
    cols = sorted(int(j) for j in make())
    eng = TopOracleEngine()
    res = ls_spa_top_subsets(*d, n_best=T, include=make(), _engine=eng)
    assert eng.top_calls == [(B.mask_of(cols), T)]
    assert res.sizes.tolist() == list(range(len(cols), p + 1))
    assert res.n_models.tolist() == [min(T, comb(p - len(cols), k - len(cols))) for k in res.sizes]
    valid = np.arange(T)[None, :] < res.n_models[:, None]
    assert res.subsets[valid][:, cols].all()
    tv = T_.top_truth(eng.all_values(), p, T, B.mask_of(cols))[0]
    np.testing.assert_array_equal(res.r_squared, tv[len(cols):])


def test_failed_pivots_warn_and_leave_nan_ranks():
    p = 3
    d = data(p, seed=2)
    v = np.array([0.0, 0.6, 0.1, 0.6, 0.2, 0.3, 0.1, 0.9])
    with pytest.warns(RuntimeWarning, match="not numerically positive definite"):
        res = ls_spa_top_subsets(*d, n_best=2, _engine=TopOracleEngine(values=v, info=1, cut=[1, 2, 1, 0]))
    assert res.n_models.tolist() == [1, 2, 1, 0] and np.isnan(res.r_squared[3]).all() and res.best_size == 1
    assert np.isnan(res.r_squared[2, 1]) and np.isnan(res.gap[2, 1]) and np.isnan(res.theta[3]).all()
    with pytest.warns(RuntimeWarning):
        res = ls_spa_top_subsets(*d, n_best=2, include=[0, 1, 2],
                                 _engine=TopOracleEngine(values=v, info=1, cut=[0, 0, 0, 0]))
    assert res.best_size == -1 and not res.best_subset.any() and len(res.top_sizes) == 0
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        ls_spa_top_subsets(*data(5, seed=2), _engine=TopOracleEngine(info=1))
    assert len(seen) == 1 and seen[0].filename == __file__
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ls_spa_top_subsets(*data(5, seed=2), _engine=TopOracleEngine())


def _zero_y(d):
    return d[0], d[1], d[2], np.zeros_like(d[3])


@pytest.mark.parametrize("make, kw, error, text", [
    (lambda: data(33, n=80, m=50, seed=1), {}, ValueError, "at most p = 32"),
    (lambda: data(6), dict(n_best=0), ValueError, "integer in 1 .. 16"),
    (lambda: data(6), dict(n_best=17), ValueError, "integer in 1 .. 16"),
    (lambda: data(6), dict(n_best=2.0), ValueError, "integer in 1 .. 16"),
    (lambda: data(6), dict(n_best=True), ValueError, "integer in 1 .. 16"),
    (lambda: data(6), dict(n_best=None), ValueError, "integer in 1 .. 16"),
    (lambda: data(6), dict(include=[6]), ValueError, "outside 0 .. 5"),
    (lambda: data(6), dict(include=[1, 4, 1]), ValueError, "twice"),
    (lambda: data(6), dict(include=3), ValueError, "iterable of column indices"),
    (lambda: _zero_y(data(6)), {}, ValueError, "identically zero"),
    (lambda: (data(6)[0], data(5)[1]) + data(6)[2:], {}, SizeIncompatible, None),
    (lambda: (data(6)[0][:-1],) + data(6)[1:], {}, SizeIncompatible, None),
])
def test_refusals_come_before_any_engine_work(monkeypatch, make, kw, error, text):
    def no_engine(*a, **k):
        raise AssertionError("an engine was acquired")
    monkeypatch.setattr(_driver, "_acquire_engine", no_engine)
    eng = TopOracleEngine()
    with pytest.raises(error, match=text):
        ls_spa_top_subsets(*make(), _engine=eng, **kw)
    assert eng.touched == 0 and eng.top_calls == []
    with pytest.raises(error, match=text):
        ls_spa_top_subsets(*make(), **kw)          # no engine of the caller's: none is acquired either


def test_groups_is_not_a_parameter():
    with pytest.raises(TypeError, match="groups"):
        ls_spa_top_subsets(*data(6), groups=[0, 0, 1, 1, 2, 2])


def test_numpy_integer_n_best_and_a_kept_engine_back_to_float64():
    class Float32Engine(TopOracleEngine):
        precision = "float32"

        def set_precision(self, dtype):
            self.precision = np.dtype(dtype).name

        def full_fit(self):
            assert self.precision == "float64", "full fit with fp32 factorisation"
            return super().full_fit()

    eng = Float32Engine()
    res = ls_spa_top_subsets(*data(6, seed=3), n_best=np.int64(3), _engine=eng)
    assert eng.precision == "float64" and res.r_squared.shape == (7, 3) and eng.top_calls == [(0, 3)]
