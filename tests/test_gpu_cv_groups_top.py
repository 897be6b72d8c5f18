"""Top lists by the K-fold cross-validated R^2 over groups of columns on the MI355X (lsspa_cv_groups_top;
groups_cv_top_kernel in csrc/k_groups.hip): the lists against the sort of the device's own values, bit for bit, and
against the truth of tests/cv_groups_ref.py; rank 0 against lsspa_cv_groups_best; exact ties across the last rank in two
numberings; the cut into steps, units and launches; a failed pivot in one fold; isolation; singletons against the
column call; the engine's refusals; the public call."""
from math import comb

import numpy as np
import pytest

import cv_groups_ref as CG
import cv_groups_top_ref as GT
import cv_ref as R
import cv_top_ref as CT
from ls_spa import (TopGroupSubsetsCVResults, TopSubsetsCVResults, ls_spa_top_group_subsets_cv,
                    ls_spa_top_subsets_cv)

pytestmark = pytest.mark.gpu

NOT_PD = 1
TOL = dict(rtol=0, atol=1e-11)          # the project's bound for these enumerations (tests/test_gpu_cv_groups.py)
GRID = [(name, K) for name in GT.NAMES for K in GT.KS]
n_groups, all_masks = GT.n_groups, GT.all_masks


def check_lists(engine, labels, T, du, df, steps=0, ok=None):
    """cv_groups_top against the host sort of the debug values du [2^g], df [2^g][K] under (larger value, smaller
    mask) over the candidates `ok`."""
    g = n_groups(labels)
    got = engine.cv_groups_top(labels, T, steps)
    u, masks, count, u_fold, info = got
    want_u, want_m, want_c = GT.top_lists(du, g, T, ok)
    np.testing.assert_array_equal(count, want_c)
    np.testing.assert_array_equal(masks, want_m)
    np.testing.assert_array_equal(u, want_u)                  # (NaN past the count on both sides)
    listed = np.arange(T)[None, :] < count[:, None]
    assert np.isnan(u[~listed]).all() and (masks[~listed] == 0).all() and np.isnan(u_fold[~listed]).all()
    np.testing.assert_array_equal(u_fold[listed], df[masks[listed].astype(np.int64)])
    np.testing.assert_array_equal(u[listed], CG.seq_sum(u_fold[listed]))
    return got


def same(a, b):
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


# ---- 1. the lists against the device's own values, bit for bit -------------------------------------------------------
@pytest.mark.parametrize("name, K", GRID)
def test_lists_against_own_values(engine, name, K):
    X, y, ids, labels, _, _ = GT.case(name, K)
    g = n_groups(labels)
    engine.cv_groups_load(X, y, ids, K, 0.0)
    du, df = engine.debug_cv_group_values(labels, all_masks(g))
    for T in (1, 4, 16):
        u, masks, count, u_fold, info = check_lists(engine, labels, T, du, df)
        assert (info == 0).all() and count.tolist() == [min(T, comb(g, k)) for k in range(g + 1)]
        assert int(masks[0, 0]) == 0 and int(masks[g, 0]) == (1 << g) - 1
        same((u, masks, count, u_fold, info), engine.cv_groups_top(labels, T))      # two calls agree bitwise
    engine.cv_free()


# ---- 2. against the truth --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, K", GRID)
def test_lists_against_the_truth(engine, name, K):
    T = 16
    X, y, ids, labels, tu, _ = GT.case(name, K)
    g = n_groups(labels)                                      # (the margin of these lists: test_cv_groups_top_host.py)
    engine.cv_groups_load(X, y, ids, K, 0.0)
    u, masks, count, _, info = engine.cv_groups_top(labels, T)
    engine.cv_free()
    want_u, want_m, want_c = GT.top_lists(tu, g, T)
    np.testing.assert_array_equal(count, want_c)
    np.testing.assert_array_equal(masks, want_m)
    listed = np.arange(T)[None, :] < count[:, None]
    print(name, "K", K, "max |value - truth|", np.abs(u[listed] - want_u[listed]).max())
    np.testing.assert_allclose(u[listed], want_u[listed], **TOL)
    assert (info == 0).all()


# ---- 3. rank 0 is cv_groups_best, and prefix -------------------------------------------------------------------------
@pytest.mark.parametrize("name, K", GRID)
def test_rank_zero_is_cv_groups_best_and_prefix(engine, name, K):
    X, y, ids, labels, _, _ = GT.case(name, K)
    engine.cv_groups_load(X, y, ids, K, 0.0)
    bu, bm, found, bf, _ = engine.cv_groups_best(labels)
    u4, m4, c4, f4, _ = engine.cv_groups_top(labels, 4)
    u16, m16, c16, f16, _ = engine.cv_groups_top(labels, 16)
    engine.cv_free()
    assert found.all() and (c16 >= 1).all()
    same((bu, bm, bf), (u16[:, 0], m16[:, 0], f16[:, 0]))
    same((u4, m4, f4), (u16[:, :4], m16[:, :4], f16[:, :4]))
    np.testing.assert_array_equal(c4, np.minimum(c16, 4))


# ---- 4. exact ties across the last rank ------------------------------------------------------------------------------
@pytest.mark.parametrize("run", list(CG.TIE_RUNS))
def test_exact_ties_straddling_the_last_rank(engine, run):
    """Groups a, b, c tie bitwise at the maximum of size 1 and their pairs at size 2; a is a low group, b and c are high
    ones, and the two runs number them differently: what is listed goes by the caller's masks, not by the layout's."""
    X, y, ids, labels, _ = CG.tie_case(run)
    g = 5
    engine.cv_groups_load(X, y, ids, 2, 0.0)
    du, df = engine.debug_cv_group_values(labels, all_masks(g))
    lab = CG.TIE_RUNS[run]
    a, b, c = (1 << lab[k] for k in "abc")
    size = np.array([bin(m).count("1") for m in range(32)])
    # the ties this test is about exist on the device: distinct masks of one size, bit-equal at the maximum
    assert du[a] == du[b] == du[c] == du[size == 1].max()
    assert du[a | b] == du[a | c] == du[b | c] == du[size == 2].max()
    for T in (1, 2):
        u, masks, count, _, info = check_lists(engine, labels, T, du, df)
        assert (info == 0).all()
        for k, tied in ((1, sorted([a, b, c])), (2, sorted([a | b, a | c, b | c]))):
            assert masks[k].tolist() == tied[:T]              # the smallest caller masks of the tied set, in order
            assert tied[2] not in masks[k].tolist() and (u[k] == du[tied[0]]).all()
    engine.cv_free()


# ---- 5. the cut ------------------------------------------------------------------------------------------------------
def test_lists_do_not_depend_on_steps(engine):
    K, T = 5, 16
    X, y, ids, labels, _, _ = GT.case("nine", K)
    engine.cv_groups_load(X, y, ids, K, 0.0)
    runs = [engine.cv_groups_top(labels, T, s) for s in (1, 3, 0)]
    engine.cv_free()
    assert (runs[0][2] == np.minimum(T, [comb(9, k) for k in range(10)])).all()
    for other in runs[1:]:
        same(runs[0], other)


def test_several_units_and_launches(engine):
    """g = 18 over p = 64, K = 2: 8192 units of four steps each, two steps a launch -- the cut goes through a unit and
    the second launch merges into the lists the first one stored."""
    labels, K, n, T = CG.multi_labels(), CG.MULTI_K, CG.MULTI_N, 4
    g = n_groups(labels)
    X, y = R.data(len(labels), n, seed=CG.MULTI_SEED)
    ids = R.fold_ids(n, K, seed=CG.FOLD_SEED)
    plan = engine.debug_cv_groups_top_plan(labels, K, T)
    assert plan["units"] == 8192 and plan["per"] == 4 and plan["steps"] == 2 and plan["launches"] == 2
    engine.cv_groups_load(X, y, ids, K, 0.0)
    whole = engine.cv_groups_top(labels, T)
    assert engine.cv_timing()["launches"] == 2
    cut = engine.cv_groups_top(labels, T, 1)
    assert engine.cv_timing()["launches"] == 4
    same(whole, cut)
    du, df = engine.debug_cv_group_values(labels, all_masks(g))      # all 2^18 masks of the device's own table
    engine.cv_free()
    want_u, want_m, want_c = GT.top_lists(du, g, T)
    u, masks, count, u_fold, info = whole
    np.testing.assert_array_equal(count, want_c)
    np.testing.assert_array_equal(masks, want_m)
    np.testing.assert_array_equal(u, want_u)
    listed = np.arange(T)[None, :] < count[:, None]
    np.testing.assert_array_equal(u_fold[listed], df[masks[listed].astype(np.int64)])
    assert (info == 0).all() and count.tolist() == [min(T, comb(g, k)) for k in range(g + 1)]


# ---- 6. a failed pivot in one fold -----------------------------------------------------------------------------------
def test_failed_pivot_in_one_fold(engine):
    K, n, T = 3, CG.N_ROWS, 16
    labels = CG.case_labels("mixed")
    g = n_groups(labels)
    X, y = R.data(len(labels), n, seed=921)
    ids = (np.arange(n) % K).astype(np.int32)
    a, b = int(np.nonzero(labels == 1)[0][0]), int(np.nonzero(labels == 4)[0][0])    # a low and a high group
    X = X.copy()
    X[ids != 1, b] = X[ids != 1, a]      # two columns that are copies of each other on the training rows of fold 1 only
    both = (1 << 1) | (1 << 4)
    ok = (np.arange(1 << g) & both) != both
    engine.cv_groups_load(X, y, ids, K, 0.0)
    du, df = engine.debug_cv_group_values(labels, all_masks(g))
    u, masks, count, u_fold, info = check_lists(engine, labels, T, du, df, ok=ok)    # the ok-filtered sort
    engine.cv_free()
    assert info[1] & NOT_PD and info[0] == 0 and info[2] == 0
    listed = np.arange(T)[None, :] < count[:, None]
    assert ((masks[listed] & both) != both).all()             # no listed set holds both copies
    assert count[g] == 0 and np.isnan(u[g]).all() and np.isnan(u_fold[g]).all()      # the only set of size g does
    assert (count[:g] >= 1).all()
    with pytest.warns(RuntimeWarning, match="fold.* 1 "):
        res = ls_spa_top_group_subsets_cv(X, y, labels, folds=ids, n_best=T)
    assert res.n_models.tolist() == count.tolist() and not res.subsets[g].any() and np.isnan(res.theta[g]).all()
    np.testing.assert_array_equal(res.r_squared, u)


# ---- 7. isolation ----------------------------------------------------------------------------------------------------
def test_isolation(engine):
    from test_subsets_host import data
    X, y, ids, labels, _, _ = GT.case("mixed", 5)
    d = data(len(labels), seed=2)
    engine.load_data(*d, 0.0)
    split_before = engine.groups_shapley(labels), engine.groups_best(labels), engine.groups_top(labels, 5)
    engine.cv_groups_load(X, y, ids, 5, 0.0)
    before = engine.cv_groups_shapley(labels), engine.cv_groups_best(labels)
    first = engine.cv_groups_top(labels, 16)
    after = engine.cv_groups_shapley(labels), engine.cv_groups_best(labels)
    same(before[0] + before[1], after[0] + after[1])
    same(first, engine.cv_groups_top(labels, 16))             # ... and the list call after them
    split_after = engine.groups_shapley(labels), engine.groups_best(labels), engine.groups_top(labels, 5)
    for ra, rb in zip(split_before, split_after):
        same(ra, rb)
    same(first, engine.cv_groups_top(labels, 16))
    engine.cv_free()
    with pytest.raises(Exception, match="lsspa_cv_load comes first"):
        engine.cv_groups_top([0])                             # (nothing loaded: the wrapper knows no p)
    with pytest.raises(Exception, match="lsspa_cv_load comes first"):
        engine.cv_groups_top([0], 99, -1)                     # the state comes before the arguments


# ---- 8. singletons are the column call -------------------------------------------------------------------------------
def test_singletons_are_the_column_call(engine):
    """Every column a group of its own: the grouped lists are the column lists, under the caller's numbering of the
    groups.  Two different kernels with different elimination orders, so the values agree to rounding, not bitwise; the
    truth's lists have a margin far above that (asserted), so the masks agree exactly."""
    p, K, n, T = 9, 3, 120, 16
    X, y = R.data(p, n, seed=900)
    ids = R.fold_ids(n, K, seed=7)
    tv, _ = R.cv_values(X, y, ids, K, 0.0)
    assert CT.margin(tv, p, T) > 1e-9
    engine.cv_load(X, y, ids, K, 0.0)
    v, masks, count, v_fold, _ = engine.cv_top(0, T)
    listed = np.arange(T)[None, :] < count[:, None]
    for labels in (np.arange(p), np.random.default_rng(5).permutation(p)):
        u, gmasks, gcount, u_fold, ginfo = engine.cv_groups_top(labels, T)
        # column mask -> group mask: column j is group labels[j]
        want = np.zeros_like(masks)
        for j in range(p):
            want |= ((masks >> np.uint32(j)) & np.uint32(1)) << np.uint32(labels[j])
        assert (ginfo == 0).all()
        np.testing.assert_array_equal(gcount, count)
        np.testing.assert_array_equal(gmasks, want)
        np.testing.assert_allclose(u[listed], v[listed], **TOL)
        np.testing.assert_allclose(u_fold[listed], v_fold[listed], **TOL)
    engine.cv_free()


# ---- 9. the engine's refusals ----------------------------------------------------------------------------------------
def test_engine_refusals(engine):
    X, y, ids, labels, _, _ = GT.case("mixed", 2)
    g = n_groups(labels)
    engine.cv_groups_load(X, y, ids, 2, 0.0)
    for T in (0, 17, -3):
        with pytest.raises(Exception, match="lsspa_cv_groups_top keeps 1 .. 16 subsets of every size"):
            engine.cv_groups_top(labels, T)
    with pytest.raises(Exception, match="lsspa_cv_groups_top: steps must be >= 0"):
        engine.cv_groups_top(labels, 4, -1)
    gap = np.where(labels == 1, g, labels)                    # group 1 has no column
    with pytest.raises(Exception, match="group labels: a group of 0 .. g-1 has no column"):
        engine.cv_groups_top(gap, 4)
    with pytest.raises(Exception, match="group labels: a group of 0 .. g-1 has no column"):
        engine.cv_groups_top(gap, 99, -1)                     # the labels come before T and steps
    with pytest.raises(Exception, match="lsspa_cv_groups_top keeps 1 .. 16"):
        engine.cv_groups_top(labels, 99, -1)                  # and T before steps
    with pytest.raises(Exception, match="labels must have length p"):
        engine.cv_groups_top(labels[:-1], 4)
    good = engine.cv_groups_top(labels, 4)                    # a refusal leaves the loaded folds usable
    assert (good[2] == np.minimum(4, [comb(g, k) for k in range(g + 1)])).all()
    engine.cv_free()


# ---- 10. the public call ---------------------------------------------------------------------------------------------
def test_public_call(engine):
    K, T = 4, 6
    X, y, _, labels, _, _ = GT.case("nine", 5)
    g, n, p = n_groups(labels), len(y), len(labels)
    res = ls_spa_top_group_subsets_cv(X, y, labels, folds=K, n_best=T, seed=7)
    assert isinstance(res, TopGroupSubsetsCVResults) and res.sizes.tolist() == list(range(g + 1))
    ids = R.fold_ids(n, K, seed=7)
    np.testing.assert_array_equal(res.fold_ids, ids)
    engine.cv_groups_load(X, y, ids, K, 0.0)
    u, masks, count, u_fold, info = engine.cv_groups_top(labels, T)
    full, _ = engine.debug_cv_group_values(labels, np.array([(1 << g) - 1], dtype=np.uint64), folds=False)
    engine.cv_free()
    np.testing.assert_array_equal(res.n_models, count)
    np.testing.assert_array_equal(res.r_squared, u)
    np.testing.assert_array_equal(res.fold_r_squared, u_fold)
    got_masks = GT.masks_of(res.group_subsets)
    np.testing.assert_array_equal(got_masks, masks.astype(np.int64))
    assert res.full_r_squared == full[0] == res.r_squared[g, 0] and res.baseline_r_squared == res.r_squared[0, 0]
    listed = np.arange(T)[None, :] < res.n_models[:, None]
    base = np.asarray(labels) < 0
    for i, r in zip(*np.nonzero(listed)):
        want_cols = base | res.group_subsets[i, r][np.maximum(labels, 0)]        # baseline | listed groups
        np.testing.assert_array_equal(res.subsets[i, r], want_cols)
        np.testing.assert_array_equal(res.subsets[i, r], GT.columns_of(labels, res.group_subsets[i, r]))
        assert res.n_columns[i, r] == want_cols.sum() and res.group_subsets[i, r].sum() == i
        cols = np.nonzero(want_cols)[0]
        np.testing.assert_allclose(res.theta[i, r, cols], np.linalg.lstsq(X[:, cols], y, rcond=None)[0], rtol=1e-9)
        assert (res.theta[i, r, ~want_cols] == 0.0).all()
    assert np.isnan(res.theta[~listed]).all() and not res.subsets[~listed].any() and (res.n_columns[~listed] == 0).all()
    np.testing.assert_array_equal(res.gap[listed], (res.r_squared[:, :1] - res.r_squared)[listed])
    b, gap, se, within, one = GT.one_se(res.sizes, res.n_models, res.r_squared, res.fold_r_squared)
    assert res.best_size == int(res.sizes[b]) and res.one_se_size == int(res.sizes[one]) <= res.best_size
    np.testing.assert_array_equal(res.best_gap, gap)
    np.testing.assert_allclose(res.best_gap_std_error, se, rtol=1e-12, atol=0)
    np.testing.assert_array_equal(res.within_one_se, within)
    np.testing.assert_array_equal(res.one_se_group_subset, res.group_subsets[one, 0])
    np.testing.assert_array_equal(res.one_se_subset, res.subsets[one, 0])
    np.testing.assert_array_equal(res.best_group_subset, res.group_subsets[b, 0])
    np.testing.assert_array_equal(res.best_subset, res.subsets[b, 0])
    flat_v, flat_m = res.r_squared[listed], got_masks[listed]
    order = np.lexsort((flat_m, -flat_v))[:T]
    np.testing.assert_array_equal(res.top_r_squared, flat_v[order])
    np.testing.assert_array_equal(GT.masks_of(res.top_group_subsets), flat_m[order])
    np.testing.assert_array_equal(res.top_sizes, res.top_group_subsets.sum(axis=1))
    np.testing.assert_array_equal(res.top_subsets,
                                  np.array([GT.columns_of(labels, gs) for gs in res.top_group_subsets]))
    assert res.top_r_squared[0] == res.r_squared[b, 0] and "one standard error" in repr(res)
    # the column call returns what it returned before: the column lists of the engine, bit for bit
    Xc = np.ascontiguousarray(X[:, :10])
    plain = ls_spa_top_subsets_cv(Xc, y, folds=K, n_best=T, seed=7)
    assert type(plain) is TopSubsetsCVResults
    engine.cv_load(Xc, y, ids, K, 0.0)
    v, cmasks, ccount, v_fold, _ = engine.cv_top(0, T)
    engine.cv_free()
    np.testing.assert_array_equal(plain.n_models, ccount)
    np.testing.assert_array_equal(plain.r_squared, v)
    np.testing.assert_array_equal(plain.fold_r_squared, v_fold)
    np.testing.assert_array_equal((plain.subsets.astype(np.int64) << np.arange(10)).sum(axis=2), cmasks.astype(np.int64))
