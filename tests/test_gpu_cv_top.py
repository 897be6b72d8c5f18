"""Top lists by the K-fold cross-validated R^2 on the MI355X (lsspa_cv_top; subsets_cv_top_kernel in
csrc/k_subsets.hip): the lists against the sort of the device's own values, bit for bit, and against the long-double
truth; rank 0 against lsspa_cv_best; exact ties across the last rank; include; the cut into steps, units and launches;
a failed pivot in one fold; isolation; the public call."""
from math import comb

import numpy as np
import pytest

import cv_top_ref as CT
from ls_spa import TopSubsetsCVResults, ls_spa_top_subsets_cv

pytestmark = pytest.mark.gpu

NOT_PD = 1
GRID = [(p, K) for p in (1, 6, 7, 12) for K in (2, 5)]


def all_masks(p):
    return np.arange(1 << p, dtype=np.uint64)


def check_lists(engine, p, T, dv, df, include=0, steps=0, valid=None):
    """cv_top against the host sort of the debug values dv [2^p], df [2^p][K] under (larger value, smaller mask)."""
    got = engine.cv_top(include, T, steps)
    v, masks, count, v_fold, info = got
    want_v, want_m, want_c = CT.top_lists(dv, p, T, include, valid)
    np.testing.assert_array_equal(count, want_c)
    np.testing.assert_array_equal(masks, want_m)
    np.testing.assert_array_equal(v, want_v)                  # (NaN past the count on both sides)
    listed = np.arange(T)[None, :] < count[:, None]
    assert np.isnan(v[~listed]).all() and (masks[~listed] == 0).all() and np.isnan(v_fold[~listed]).all()
    np.testing.assert_array_equal(v_fold[listed], df[masks[listed].astype(np.int64)])
    return got


def same(a, b):
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


# ---- 1. the lists against the device's own values, bit for bit -------------------------------------------------------
@pytest.mark.parametrize("p, K", GRID)
def test_lists_against_own_values(engine, p, K):
    X, y, ids, _, _ = CT.truth_case(p, K)
    engine.cv_load(X, y, ids, K, 0.0)
    dv, df = engine.debug_cv_values(all_masks(p))
    for T in (1, 4, 16):
        v, masks, count, v_fold, info = check_lists(engine, p, T, dv, df)
        assert (info == 0).all() and count.tolist() == [min(T, comb(p, k)) for k in range(p + 1)]
        assert v[0, 0] == 0.0 and masks[p, 0] == (1 << p) - 1
        same((v, masks, count, v_fold, info), engine.cv_top(0, T))       # two calls agree bitwise
    engine.cv_free()


# ---- 2. against the truth --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p, K", GRID)
def test_lists_against_the_truth(engine, p, K):
    T = 16
    X, y, ids, tv, _ = CT.truth_case(p, K)
    m = CT.margin(tv, p, T)
    print("p", p, "K", K, "margin of the truth's lists", m)
    assert m > 1e-9                                           # asserted, never skipped: tests/test_cv_top_host.py too
    engine.cv_load(X, y, ids, K, 0.0)
    v, masks, count, _, info = engine.cv_top(0, T)
    engine.cv_free()
    want_v, want_m, want_c = CT.top_lists(tv, p, T)
    np.testing.assert_array_equal(count, want_c)
    np.testing.assert_array_equal(masks, want_m)
    listed = np.arange(T)[None, :] < count[:, None]
    err = np.abs(v[listed] - want_v[listed]).max()
    print("max |value - truth|", err)
    assert err <= 1e-11 and (info == 0).all()


# ---- 3. consistency --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p, K", GRID)
def test_rank_zero_is_cv_best_and_prefix(engine, p, K):
    X, y, ids, _, _ = CT.truth_case(p, K)
    engine.cv_load(X, y, ids, K, 0.0)
    bv, bm, found, bf, _ = engine.cv_best()
    v4, m4, c4, f4, _ = engine.cv_top(0, 4)
    v16, m16, c16, f16, _ = engine.cv_top(0, 16)
    engine.cv_free()
    assert found.all() and (c16 >= 1).all()
    same((bv, bm, bf), (v16[:, 0], m16[:, 0], f16[:, 0]))
    same((v4, m4, f4), (v16[:, :4], m16[:, :4], f16[:, :4]))
    np.testing.assert_array_equal(c4, np.minimum(c16, 4))


# ---- 4. exact ties across the last rank ------------------------------------------------------------------------------
def test_exact_ties_straddling_the_last_rank(engine):
    p, K = 8, 3
    X, _, ids, _, _ = CT.case(p, K)
    X = X.copy()
    X[:, 5] = X[:, 0]                   # two identical columns, both among the low ones: {0} and {5} tie exactly
    rng = np.random.default_rng(1)
    y = 4.0 * X[:, 0] + 0.3 * X[:, 3] + 0.2 * rng.standard_normal(len(X))
    engine.cv_load(X, y, ids, K, 0.5)   # reg > 0: the subsets that hold both copies stay positive definite
    dv, df = engine.debug_cv_values(all_masks(p))
    sv, sm, sc = CT.top_lists(dv, p, 17)                      # the device's own order, one rank beyond the longest list
    ties = sorted({(T, k) for k in range(p + 1) for T in range(1, 17) if sc[k] > T and sv[k, T - 1] == sv[k, T]})
    print("bitwise-equal pairs at ranks T - 1 and T (T, size):", ties)
    assert (1, 1) in ties and int(sm[1, 0]) == 1 << 0 and int(sm[1, 1]) == 1 << 5      # the construction's own pair
    for T in sorted({T for T, _ in ties})[:4]:
        v, masks, count, _, _ = check_lists(engine, p, T, dv, df)
        for k in (k for t, k in ties if t == T):
            pair = np.array([sm[k, T - 1], sm[k, T]], dtype=np.uint64)
            pv, _ = engine.debug_cv_values(pair, folds=False)
            assert pv[0] == pv[1] and pair[0] < pair[1]       # the pair is equal, and of it the smaller mask is listed
            assert int(masks[k, T - 1]) == int(pair[0]) and v[k, T - 1] == pv[0]
            assert int(pair[1]) not in masks[k].tolist()
    engine.cv_free()


# ---- 5. include ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", [(1,), (8,), (0, 4, 7, 11)])
def test_include(engine, cols):
    p, K, T = 12, 2, 4
    X, y, ids, _, _ = CT.truth_case(p, K)
    inc = sum(1 << j for j in cols)
    engine.cv_load(X, y, ids, K, 0.0)
    dv, df = engine.debug_cv_values(all_masks(p))
    v, masks, count, _, _ = check_lists(engine, p, T, dv, df, include=inc)      # the filtered sort
    engine.cv_free()
    nc = len(cols)
    assert (count[:nc] == 0).all() and np.isnan(v[:nc]).all()
    assert count[nc:].tolist() == [min(T, comb(p - nc, k - nc)) for k in range(nc, p + 1)]
    listed = np.arange(T)[None, :] < count[:, None]
    assert ((masks[listed] & inc) == inc).all()


# ---- 6. the cut ------------------------------------------------------------------------------------------------------
def test_lists_do_not_depend_on_steps(engine):
    p, K, T = 14, 3, 16
    X, y, ids, _, _ = CT.case(p, K)
    engine.cv_load(X, y, ids, K, 0.0)
    plan = engine.debug_cv_top_plan(p, K, T)
    runs = [engine.cv_top(0, T, s) for s in (1, 3, plan["steps"], 0)]
    engine.cv_free()
    assert (runs[0][2] == np.minimum(T, [comb(p, k) for k in range(p + 1)])).all()
    for other in runs[1:]:
        same(runs[0], other)


def test_several_units_and_launches(engine):
    """p = 20, K = 2: 8192 units of two steps each -- forced to one step a launch, the cut goes through a unit's subsets
    and the second launch merges into the lists the first one stored."""
    p, K, T = 20, 2, 4
    X, y, ids, _, _ = CT.case(p, K, n=200)
    engine.cv_load(X, y, ids, K, 0.0)
    plan = engine.debug_cv_top_plan(p, K, T)
    assert plan["units"] == 8192 and plan["per"] == 2 and plan["steps"] == 2 and plan["launches"] == 1
    whole = engine.cv_top(0, T)
    assert engine.cv_timing()["launches"] == 1
    cut = engine.cv_top(0, T, 1)
    assert engine.cv_timing()["launches"] == 2
    same(whole, cut)
    dv, df = engine.debug_cv_values(all_masks(p))
    engine.cv_free()
    want_v, want_m, want_c = CT.top_lists(dv, p, T)
    v, masks, count, v_fold, info = whole
    np.testing.assert_array_equal(count, want_c)
    np.testing.assert_array_equal(masks, want_m)
    np.testing.assert_array_equal(v, want_v)
    listed = np.arange(T)[None, :] < count[:, None]
    np.testing.assert_array_equal(v_fold[listed], df[masks[listed].astype(np.int64)])
    assert (info == 0).all() and count.tolist() == [min(T, comb(p, k)) for k in range(p + 1)]


# ---- 7. a failed pivot in one fold -----------------------------------------------------------------------------------
def test_failed_pivot_in_one_fold(engine):
    p, K, n, T = 8, 3, 120, 16
    X, y, _, _, _ = CT.case(p, K)
    ids = (np.arange(n) % K).astype(np.int32)
    X = X.copy()
    X[ids != 1, 7] = 0.0                 # column 7 is constant zero in the training complement of fold 1
    engine.cv_load(X, y, ids, K, 0.0)
    v, masks, count, v_fold, info = engine.cv_top(0, T)
    engine.cv_free()
    assert info[1] & NOT_PD and info[0] == 0 and info[2] == 0
    listed = np.arange(T)[None, :] < count[:, None]
    assert ((masks[listed] >> 7) & 1 == 0).all()
    assert count[p] == 0 and np.isnan(v[p]).all() and np.isnan(v_fold[p]).all()     # the only subset of size p holds 7
    assert count[:p].tolist() == [min(T, comb(p - 1, k)) for k in range(p)]
    with pytest.warns(RuntimeWarning, match="fold.* 1 "):
        res = ls_spa_top_subsets_cv(X, y, folds=ids, n_best=T)
    assert res.n_models.tolist() == count.tolist() and np.isnan(res.r_squared[p]).all() and not res.subsets[p].any()
    np.testing.assert_array_equal(res.r_squared, v)
    assert not res.subsets[:, :, 7].any() and res.best_size >= 0


# ---- 8. isolation ----------------------------------------------------------------------------------------------------
def test_isolation(engine):
    from test_subsets_host import data
    d = data(9, seed=2)
    engine.load_data(*d, 0.0)
    split_before = engine.subsets_top(0, 5)
    X, y, ids, _, _ = CT.case(7, 2)
    engine.cv_load(X, y, ids, 2, 0.0)
    before = engine.cv_best(), engine.cv_shapley()
    first = engine.cv_top(0, 16)
    after = engine.cv_best(), engine.cv_shapley()
    same(before[0] + before[1], after[0] + after[1])
    same(first, engine.cv_top(0, 16))                         # ... and the list call after them
    engine.load_data(*d, 0.0)
    same(split_before, engine.subsets_top(0, 5))
    same(first, engine.cv_top(0, 16))
    engine.cv_free()
    with pytest.raises(Exception, match="lsspa_cv_load comes first"):
        engine.cv_top()
    with pytest.raises(Exception, match="lsspa_cv_load comes first"):
        engine.cv_top(0, 99, -1)                              # the state comes before the arguments


def test_engine_refusals(engine):
    X, y, ids, _, _ = CT.case(7, 2)
    engine.cv_load(X, y, ids, 2, 0.0)
    with pytest.raises(Exception, match="include names a feature beyond p"):
        engine.cv_top(1 << 7, 4)
    for T in (0, 17, -3):
        with pytest.raises(Exception, match="lsspa_cv_top keeps 1 .. 16 subsets of every size"):
            engine.cv_top(0, T)
    with pytest.raises(Exception, match="lsspa_cv_top: steps must be >= 0"):
        engine.cv_top(0, 4, -1)
    good = engine.cv_top(0, 4)                                # a refusal leaves the loaded folds usable
    assert (good[2] == np.minimum(4, [comb(7, k) for k in range(8)])).all()
    engine.cv_free()


# ---- 9. the public call ----------------------------------------------------------------------------------------------
def test_public_call(engine):
    p, K, n, T = 9, 4, 120, 6
    X, y, _, _, _ = CT.case(p, K)
    res = ls_spa_top_subsets_cv(X, y, folds=K, n_best=T, seed=7, include=[3])
    assert isinstance(res, TopSubsetsCVResults) and res.sizes.tolist() == list(range(1, p + 1))
    ids = CT.R.fold_ids(n, K, seed=7)
    np.testing.assert_array_equal(res.fold_ids, ids)
    engine.cv_load(X, y, ids, K, 0.0)
    v, masks, count, v_fold, info = engine.cv_top(1 << 3, T)
    full, _ = engine.debug_cv_values(np.array([(1 << p) - 1], dtype=np.uint64), folds=False)
    engine.cv_free()
    np.testing.assert_array_equal(res.n_models, count[1:])
    np.testing.assert_array_equal(res.r_squared, v[1:])
    np.testing.assert_array_equal(res.fold_r_squared, v_fold[1:])
    got_masks = (res.subsets.astype(np.int64) << np.arange(p)).sum(axis=2)
    np.testing.assert_array_equal(got_masks, masks[1:].astype(np.int64))
    assert res.full_r_squared == full[0] and res.subsets[np.arange(T)[None, :] < count[1:, None]][:, 3].all()
    listed = np.arange(T)[None, :] < res.n_models[:, None]
    for i, r in zip(*np.nonzero(listed)):
        cols = np.nonzero(res.subsets[i, r])[0]
        np.testing.assert_allclose(res.theta[i, r, cols], np.linalg.lstsq(X[:, cols], y, rcond=None)[0], rtol=1e-9)
        assert (res.theta[i, r, ~res.subsets[i, r]] == 0.0).all()
    b, gap, se, within, one = CT.one_se(res.sizes, res.n_models, res.r_squared, res.fold_r_squared)
    assert res.best_size == int(res.sizes[b]) and res.one_se_size == int(res.sizes[one]) <= res.best_size
    np.testing.assert_array_equal(res.best_gap, gap)
    np.testing.assert_allclose(res.best_gap_std_error, se, rtol=1e-12, atol=0)
    np.testing.assert_array_equal(res.within_one_se, within)
    np.testing.assert_array_equal(res.one_se_subset, res.subsets[one, 0])
    np.testing.assert_array_equal(res.best_subset, res.subsets[b, 0])
    flat_v, flat_m = res.r_squared[listed], got_masks[listed]
    order = np.lexsort((flat_m, -flat_v))[:T]
    np.testing.assert_array_equal(res.top_r_squared, flat_v[order])
    assert res.top_r_squared[0] == res.r_squared[b, 0] and "one standard error" in repr(res)
