"""K-fold cross-validation over groups of columns on the MI355X (lsspa_cv_groups_*; groups_cv_best_kernel in
csrc/k_groups.hip): the fold problems of a wide load, the attribution against the truth of tests/cv_groups_ref.py and,
bit for bit, against the one-problem grouped enumeration of every fold problem; the values and the selection against the
device's own values and the truth; exact ties, cuts, a failed pivot in one fold, isolation, singletons against the column
calls, and the public calls."""
import warnings

import numpy as np
import pytest

import cv_groups_ref as CG
import cv_ref as R
from ls_spa import (CVBestGroupSubsetsResults, CVGroupResults, ls_spa, ls_spa_best_subsets_cv, ls_spa_cv)
from test_gpu_cv import check_problems, load_reduced_fold

pytestmark = pytest.mark.gpu

NOT_PD = 1
TOL = dict(rtol=0, atol=1e-11)          # the project's bound for these enumerations (tests/test_gpu_groups.py)
RUNS = [(name, K, CG.N_ROWS) for name in CG.NAMES for K in CG.KS]


def popcount(masks):
    return np.array([bin(int(m)).count("1") for m in masks])


def n_groups(labels):
    return int(np.max(labels)) + 1


def all_masks(g):
    return np.arange(1 << g, dtype=np.uint64)


# ---- 1. the fold problems of a wide load, and who may use it ---------------------------------------------------------
@pytest.mark.parametrize("K, n", [(2, 101), (3, 130)])
def test_fold_problems_p40(engine, K, n):
    p = 40
    X, y = R.data(p, n, seed=40 + K)
    if K == 3:          # unequal folds, one of them a single row
        ids = np.zeros(n, dtype=np.int32)
        ids[5] = 1
        ids[70:] = 2
    else:
        ids = R.fold_ids(n, K, seed=3)
    engine.cv_groups_load(X, y, ids, K, 0.25)
    check_problems(engine, X, y, ids, K, 0.25)
    engine.cv_free()


def test_column_calls_after_grouped_loads(engine):
    X, y = R.data(40, 120, seed=41)
    ids = R.fold_ids(120, 3, seed=3)
    with pytest.raises(Exception, match="at most p = 32"):
        engine.cv_load(X, y, ids, 3, 0.0)                      # the column load keeps its limit
    engine.cv_groups_load(X, y, ids, 3, 0.0)
    for call in (engine.cv_shapley, engine.cv_best, lambda: engine.debug_cv_values(np.array([1], dtype=np.uint64))):
        with pytest.raises(Exception, match="lsspa_cv_groups_load"):
            call()
    phi, _, r2, base, info = engine.cv_groups_shapley(np.arange(40) % 8)   # the grouped calls work on it
    assert (info == 0).all() and abs(phi.sum() - (r2.sum() - base.sum())) < 1e-11 and (base == 0.0).all()
    engine.cv_free()
    with pytest.raises(Exception, match="at most p = 64"):
        engine.cv_groups_load(np.ones((80, 65)), np.ones(80), np.arange(80) % 2, 2, 0.0)
    # p <= 32: either load serves both families, with the same bits
    X, y = R.data(12, 120, seed=42)
    labels = np.arange(12) % 5
    engine.cv_load(X, y, ids, 3, 0.0)
    a = engine.cv_shapley(), engine.cv_best(), engine.cv_groups_shapley(labels), engine.cv_groups_best(labels)
    engine.cv_free()
    engine.cv_groups_load(X, y, ids, 3, 0.0)
    b = engine.cv_shapley(), engine.cv_best(), engine.cv_groups_shapley(labels), engine.cv_groups_best(labels)
    engine.cv_free()
    for ra, rb in zip(a, b):
        for xa, xb in zip(ra, rb):
            np.testing.assert_array_equal(xa, xb)


# ---- 2. the attribution ----------------------------------------------------------------------------------------------
def check_attribution(engine, name, K, n):
    X, y, ids, labels, u, uf = CG.case(name, K, n)
    g = n_groups(labels)
    engine.cv_groups_load(X, y, ids, K, 0.0)
    phi, phi_fold, r2_fold, base_fold, info = engine.cv_groups_shapley(labels)
    probs = [engine.cv_get_problem(f) for f in range(K)]
    engine.cv_free()
    truth = CG.shapley(u, g)
    print(name, "K", K, "max |phi - truth|", np.abs(phi - truth).max())
    assert (info == 0).all() and phi.shape == (g,) and phi_fold.shape == (K, g)
    np.testing.assert_allclose(phi, truth, **TOL)
    np.testing.assert_allclose(r2_fold, uf[-1], **TOL)
    np.testing.assert_allclose(base_fold, uf[0], **TOL)
    assert abs(phi.sum() - (CG.seq_sum(r2_fold[None, :])[0] - CG.seq_sum(base_fold[None, :])[0])) < 1e-11
    np.testing.assert_array_equal(phi, CG.seq_sum(phi_fold.T))
    for f in range(K):
        load_reduced_fold(engine, probs[f])
        one, bits = engine.groups_shapley(labels)
        assert bits == 0
        np.testing.assert_array_equal(phi_fold[f], one)


@pytest.mark.parametrize("name, K, n", RUNS)
def test_attribution_truth_and_bits(engine, name, K, n):
    check_attribution(engine, name, K, n)


def test_attribution_32_folds(engine):
    check_attribution(engine, *CG.WIDE)


# ---- 3. the values ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["nine", "gl0"])
def test_values_bitwise(engine, name):
    K = 5
    X, y, ids, labels, u, uf = CG.case(name, K)
    g = n_groups(labels)
    masks = all_masks(g) if name == "nine" else np.array([0, 1, 2, 5, 6, 7], dtype=np.uint64)
    engine.cv_groups_load(X, y, ids, K, 0.0)
    got_u, got_f = engine.debug_cv_group_values(labels, masks)
    only_u, none = engine.debug_cv_group_values(labels, masks, folds=False)
    probs = [engine.cv_get_problem(f) for f in range(K)]
    engine.cv_free()
    assert none is None
    np.testing.assert_array_equal(only_u, got_u)
    np.testing.assert_array_equal(got_u, CG.seq_sum(got_f))
    np.testing.assert_allclose(got_f, uf[masks.astype(np.int64)], **TOL)
    for f in range(K):
        load_reduced_fold(engine, probs[f])
        np.testing.assert_array_equal(got_f[:, f], engine.debug_group_values(labels, masks))


# ---- 4. the selection ------------------------------------------------------------------------------------------------
def check_selection(engine, labels, steps=0, ok=None):
    """cv_groups_best against the arg-best of the device's own table of all 2^g values, bitwise"""
    g = n_groups(labels)
    got = engine.cv_groups_best(labels, steps)
    u, masks, found, u_fold, info = got
    du, df = engine.debug_cv_group_values(labels, all_masks(g))
    best, want_masks, want_found, _ = CG.best(du, g, ok)
    np.testing.assert_array_equal(found, want_found)
    np.testing.assert_array_equal(masks, want_masks)
    np.testing.assert_array_equal(u[found], best[found])
    assert np.isnan(u[~found]).all() and (masks[~found] == 0).all() and np.isnan(u_fold[~found]).all()
    np.testing.assert_array_equal(u_fold[found], df[masks[found].astype(np.int64)])
    np.testing.assert_array_equal(u[found], CG.seq_sum(u_fold[found]))
    assert (popcount(masks[found]) == np.nonzero(found)[0]).all()
    return got


@pytest.mark.parametrize("name, K, n", RUNS)
def test_selection_against_own_values_and_truth(engine, name, K, n):
    X, y, ids, labels, u, uf = CG.case(name, K, n)
    g = n_groups(labels)
    engine.cv_groups_load(X, y, ids, K, 0.0)
    got_u, masks, found, _, info = check_selection(engine, labels)
    again = engine.cv_groups_best(labels)
    engine.cv_free()
    for a, b in zip((got_u, masks, found), again[:3]):
        np.testing.assert_array_equal(a, b)                   # two calls agree bitwise
    best, want_masks, want_found, _ = CG.best(u, g)           # (the gap: tests/test_cv_groups_host.py)
    assert (info == 0).all() and found.all()
    np.testing.assert_array_equal(masks, want_masks)
    np.testing.assert_allclose(got_u, best, **TOL)
    assert int(masks[0]) == 0 and int(masks[g]) == (1 << g) - 1


@pytest.mark.parametrize("run", list(CG.TIE_RUNS))
def test_exact_ties_go_to_the_smallest_caller_mask(engine, run):
    X, y, ids, labels, u_all = CG.tie_case(run)
    engine.cv_groups_load(X, y, ids, 2, 0.0)
    u, masks, found, _, info = check_selection(engine, labels)
    du, _ = engine.debug_cv_group_values(labels, all_masks(5), folds=False)
    engine.cv_free()
    print(run, "masks", list(masks), "u", list(u))
    lab = CG.TIE_RUNS[run]
    a, b, c = (1 << lab[k] for k in "abc")
    # the pairs this test is about exist on the device: distinct masks of one size, bit-equal at the maximum
    assert du[a] == du[b] == du[c] == du[[m for m in range(32) if popcount([m])[0] == 1]].max()
    assert du[a | b] == du[a | c] == du[b | c] == du[[m for m in range(32) if popcount([m])[0] == 2]].max()
    assert (info == 0).all() and found.all()
    assert list(masks[1:4]) == CG.tie_winners(run) and (u[:4] == 0.0).all()
    np.testing.assert_array_equal(masks, CG.best(u_all, 5)[1])


# ---- 5. cuts ---------------------------------------------------------------------------------------------------------
def test_selection_does_not_depend_on_steps(engine):
    X, y, ids, labels, _, _ = CG.case("nine", 5)
    engine.cv_groups_load(X, y, ids, 5, 0.0)
    runs = [engine.cv_groups_best(labels, s) for s in (1, 0)]
    engine.cv_free()
    for a, b in zip(*runs):
        np.testing.assert_array_equal(a, b)


def test_selection_several_units_and_launches(engine):
    """g = 18 over p = 64, K = 2: 8192 units of four steps each, two steps a launch -- the cut goes through a unit."""
    labels, K, n = CG.multi_labels(), CG.MULTI_K, CG.MULTI_N
    X, y = R.data(len(labels), n, seed=CG.MULTI_SEED)
    ids = R.fold_ids(n, K, seed=CG.FOLD_SEED)
    plan = engine.debug_cv_groups_plan(labels, K)
    assert plan["units"] == 8192 and plan["per"] == 4 and plan["steps"] == 2 and plan["launches"] == 2
    engine.cv_groups_load(X, y, ids, K, 0.0)
    u, masks, found, u_fold, info = check_selection(engine, labels)      # all 2^18 masks of the device's own table
    assert engine.cv_timing()["launches"] == 2
    cut = engine.cv_groups_best(labels, 1)
    assert engine.cv_timing()["launches"] == 4
    engine.cv_free()
    for a, b in zip((u, masks, found, u_fold), cut[:4]):
        np.testing.assert_array_equal(a, b)
    assert (info == 0).all() and found.all()


# ---- 6. a failed pivot in one fold -----------------------------------------------------------------------------------
def test_failed_pivot_in_one_fold(engine):
    K, n = 3, CG.N_ROWS
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
    u, masks, found, u_fold, info = check_selection(engine, labels, ok=ok)
    engine.cv_free()
    assert info[1] & NOT_PD and info[0] == 0 and info[2] == 0
    assert found[:g].all() and not found[g] and np.isnan(u[g])            # the only set of size g holds both copies
    assert ((masks[:g] & both) != both).all()
    truth, _ = CG.cv_values(X, y, ids, K, labels, masks=np.nonzero(ok)[0])
    table = np.full(1 << g, np.nan)
    table[ok] = truth
    best, want_masks, want_found, runner = CG.best(table, g, ok)
    assert ((best - runner)[np.isfinite(runner)] > CG.MIN_GAP).all()
    np.testing.assert_array_equal(masks[:g], want_masks[:g])
    np.testing.assert_allclose(u[:g], best[:g], **TOL)
    with pytest.warns(RuntimeWarning, match="fold.* 1 "):
        res = ls_spa_best_subsets_cv(X, y, folds=ids, groups=labels)
    assert np.isnan(res.r_squared[g]) and not res.subsets[g].any() and np.isnan(res.theta[g]).all()
    np.testing.assert_array_equal(res.r_squared[:g], u[:g])


# ---- 7. isolation ----------------------------------------------------------------------------------------------------
def test_isolation(engine):
    from test_subsets_host import data
    X, y, ids, labels, _, _ = CG.case("mixed", 5)
    d = data(len(labels), seed=2)
    engine.load_data(*d, 0.0)
    before = engine.groups_shapley(labels), engine.groups_best(labels)
    Xc, yc = R.data(9, 120, seed=43)
    idc = R.fold_ids(120, 3, seed=3)
    engine.cv_load(Xc, yc, idc, 3, 0.0)
    cv_before = engine.cv_shapley(), engine.cv_best()
    engine.cv_free()
    engine.cv_groups_load(X, y, ids, 5, 0.0)
    first = engine.cv_groups_shapley(labels), engine.cv_groups_best(labels)
    second = engine.cv_groups_shapley(labels), engine.cv_groups_best(labels)
    engine.cv_free()
    for ra, rb in zip(first, second):
        for xa, xb in zip(ra, rb):
            np.testing.assert_array_equal(xa, xb)             # two calls agree bitwise
    with pytest.raises(Exception, match="lsspa_cv_load comes first"):
        engine.cv_groups_best([0])                            # (nothing loaded: the wrapper knows no p)
    after = engine.groups_shapley(labels), engine.groups_best(labels)
    engine.cv_load(Xc, yc, idc, 3, 0.0)
    cv_after = engine.cv_shapley(), engine.cv_best()
    engine.cv_free()
    for ra, rb in zip(before + cv_before, after + cv_after):
        for xa, xb in zip(ra, rb):
            np.testing.assert_array_equal(xa, xb)


def test_kept_engine_sampling_unchanged_by_grouped_cv_calls():
    from test_subsets_host import data
    d = data(12, n=200, m=100, seed=12)
    kw = dict(method="argsort", seed=7, max_samples=512, batch_size=128, tolerance=0.0)
    before = ls_spa(*d, **kw)
    X, y, ids, labels, _, _ = CG.case("mixed", 2)
    ls_spa_cv(X, y, folds=ids, groups=labels)
    ls_spa_best_subsets_cv(X, y, folds=ids, groups=labels)
    after = ls_spa(*d, **kw)
    np.testing.assert_array_equal(before.attribution, after.attribution)
    np.testing.assert_array_equal(before.error_history, after.error_history)
    np.testing.assert_array_equal(before.attribution_errors, after.attribution_errors)


# ---- 8. singletons against the column calls --------------------------------------------------------------------------
def test_singletons_are_the_column_calls(engine):
    p, K, n = 9, 3, 120
    X, y = R.data(p, n, seed=900)
    ids = R.fold_ids(n, K, seed=7)
    labels = np.arange(p)
    engine.cv_load(X, y, ids, K, 0.0)
    phi, phi_fold, r2_fold, _ = engine.cv_shapley()
    v, masks, found, v_fold, _ = engine.cv_best()
    gphi, gfold, gr2, gbase, ginfo = engine.cv_groups_shapley(labels)
    u, gmasks, gfound, u_fold, _ = engine.cv_groups_best(labels)
    engine.cv_free()
    assert (ginfo == 0).all() and (gbase == 0.0).all()
    np.testing.assert_allclose(gphi, phi, **TOL)
    np.testing.assert_allclose(gfold, phi_fold, **TOL)
    np.testing.assert_allclose(gr2, r2_fold, **TOL)
    np.testing.assert_array_equal(gmasks, masks)
    np.testing.assert_array_equal(gfound, found)
    np.testing.assert_allclose(u, v, **TOL)
    np.testing.assert_allclose(u_fold, v_fold, **TOL)


# ---- 9. the public calls ---------------------------------------------------------------------------------------------
def test_public_calls():
    K = 5
    X, y, ids, labels, u, uf = CG.case("gl6", K)
    g, p = n_groups(labels), len(labels)
    res = ls_spa_cv(X, y, folds=K, seed=CG.FOLD_SEED, groups=labels)
    assert isinstance(res, CVGroupResults)
    np.testing.assert_array_equal(res.fold_ids, ids)
    np.testing.assert_allclose(res.attribution, CG.shapley(u, g), **TOL)
    assert abs(res.r_squared - u[-1]) < 1e-11 and abs(res.baseline_r_squared - u[0]) < 1e-11
    assert abs(res.attribution.sum() - (res.r_squared - res.baseline_r_squared)) < 1e-11
    assert res.r_squared == float(CG.seq_sum(res.fold_r_squared[None, :])[0])
    assert res.baseline_r_squared == float(CG.seq_sum(res.fold_baseline_r_squared[None, :])[0])
    np.testing.assert_array_equal(res.attribution, CG.seq_sum(res.fold_attribution.T))
    np.testing.assert_allclose(res.theta, np.linalg.lstsq(X, y, rcond=None)[0], rtol=1e-9)
    sel = ls_spa_best_subsets_cv(X, y, folds=K, seed=CG.FOLD_SEED, groups=labels)
    assert isinstance(sel, CVBestGroupSubsetsResults) and sel.sizes.tolist() == list(range(g + 1))
    best, masks, found, _ = CG.best(u, g)
    for k in range(g + 1):
        assert sum(1 << int(j) for j in np.nonzero(sel.group_subsets[k])[0]) == masks[k]
        np.testing.assert_array_equal(sel.subsets[k], CG.columns_of(labels, masks[k]))
        cols = np.nonzero(sel.subsets[k])[0]
        np.testing.assert_allclose(sel.theta[k, cols], np.linalg.lstsq(X[:, cols], y, rcond=None)[0], rtol=1e-9)
        assert (sel.theta[k, ~sel.subsets[k]] == 0.0).all()
    np.testing.assert_allclose(sel.r_squared, best, **TOL)
    np.testing.assert_array_equal(sel.r_squared, CG.seq_sum(sel.fold_r_squared))
    np.testing.assert_array_equal(sel.n_columns, sel.subsets.sum(axis=1))
    assert sel.full_r_squared == res.r_squared and sel.baseline_r_squared == res.baseline_r_squared
    assert sel.best_size == int(np.argmax(sel.r_squared))
    with pytest.raises(ValueError, match="include= cannot be combined with groups="):
        ls_spa_best_subsets_cv(X, y, folds=K, include=[0], groups=labels)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ls_spa_cv(X, y, folds=ids, groups=labels)
