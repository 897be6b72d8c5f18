"""K-fold cross-validation on the MI355X (lsspa_cv_*; csrc/k_cv.hip, subsets_cv_best_kernel in csrc/k_subsets.hip):
the fold problems against tests/cv_ref.py, the attribution against the long-double truth and, bit for bit, against the
one-problem enumeration of every fold problem; the values and the selection against the device's own values and the
truth; failed pivots; isolation from the loaded problem and the bootstrap's rows; the public calls."""
import functools
import warnings

import numpy as np
import pytest

import cv_ref as R
from ls_spa import CVBestSubsetsResults, CVResults, ls_spa_best_subsets_cv, ls_spa_cv

pytestmark = pytest.mark.gpu

NOT_PD = 1


def popcount(masks):
    return np.array([bin(int(m)).count("1") for m in masks])


def seq_sum(cols):
    """fp64 sum of the columns of cols [n][K] in ascending order, as the device forms it"""
    total = cols[:, 0].copy()
    for f in range(1, cols.shape[1]):
        total = total + cols[:, f]
    return total


@functools.lru_cache(maxsize=None)
def case(p, K, n=120, seed=0, reg=0.0):
    X, y = R.data(p, n, seed=100 * p + seed)
    ids = R.fold_ids(n, K, seed=7)
    v, vf = R.cv_values(X, y, ids, K, reg) if p <= 12 else (None, None)
    return X, y, ids, v, vf


def load_reduced_fold(engine, prob):
    """Fold problem `prob` = cv_get_problem(f) as the loaded problem, with a ||y||^2 whose reciprocal has the bits of
    the pooled 1 / ||y||^2 the fold problems carry."""
    G, g, H, h, inv_yy = prob
    yy = 1.0 / inv_yy
    for _ in range(8):
        if 1.0 / yy == inv_yy:
            break
        yy = np.nextafter(yy, np.inf if 1.0 / yy > inv_yy else -np.inf)
    assert 1.0 / yy == inv_yy
    engine.load_reduced(G, g, float(g @ np.linalg.solve(G, g)) * (1 + 1e-9) + 1e-300, yy, H=H, h=h)


def arg_best(v, p, include=0, ok=None):
    best, masks, found, _ = R.best(np.asarray(v, dtype=np.float64), p, include, ok)
    return best, masks, found


# ---- 1. the fold problems --------------------------------------------------------------------------------------------
def check_problems(engine, X, y, ids, K, reg):
    want, yy = R.problems(X, y, ids, K, reg)
    worst = 0.0
    for f in range(K):
        G, g, H, h, inv_yy = engine.cv_get_problem(f)
        for got, ref in zip((G, g, H, h), want[f]):
            ref = ref.astype(np.float64)
            worst = max(worst, float(np.abs(got - ref).max() / np.abs(ref).max()))
        assert abs(inv_yy * float(yy) - 1.0) < 1e-13
        np.testing.assert_array_equal(G, G.T)
        np.testing.assert_array_equal(H, H.T)
    print("fold problems: max relative deviation", worst)
    assert worst < 1e-13


@pytest.mark.parametrize("K, n", [(2, 61), (3, 90), (32, 400)])
def test_fold_problems(engine, K, n):
    p = 9
    X, y = R.data(p, n, seed=K)
    if K == 3:          # unequal folds, one of them a single row
        ids = np.zeros(n, dtype=np.int32)
        ids[5] = 1
        ids[40:] = 2
    else:
        ids = R.fold_ids(n, K, seed=3)
    engine.cv_load(X, y, ids, K, 0.25)
    check_problems(engine, X, y, ids, K, 0.25)
    engine.cv_free()


@pytest.mark.parametrize("variant", ["f32", "strided", "device_f64", "device_f32_strided"])
def test_fold_problems_loader_variants(engine, variant):
    p, n, K = 11, 200, 4
    X, y = R.data(p, n, seed=11)
    ids = R.fold_ids(n, K, seed=5)
    f32 = "f32" in variant
    dt = np.float32 if f32 else np.float64
    ld = p + 5 if "strided" in variant else p
    buf = np.full((n, ld), 7.0, dtype=dt)          # what lies between the rows must not be read as data
    buf[:, :p] = X.astype(dt)
    yb = y.astype(dt)
    Xr, yr = buf[:, :p].astype(np.float64), yb.astype(np.float64)     # the values the device sees
    if variant.startswith("device"):
        import torch
        tx, ty = torch.from_numpy(buf).cuda(), torch.from_numpy(yb).cuda()
        torch.cuda.synchronize()
        engine.cv_load_ptr(tx.data_ptr(), ld, ty.data_ptr(), n, p, ids, K, 0.0, f32=f32, location=1)
    else:
        engine.cv_load_ptr(buf.ctypes.data, ld, yb.ctypes.data, n, p, ids, K, 0.0, f32=f32, location=0)
    check_problems(engine, Xr, yr, ids, K, 0.0)
    engine.cv_free()


# ---- 2. the attribution ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [1, 6, 7, 12])
def test_attribution_truth_and_bits(engine, p):
    K = 3
    X, y, ids, v, vf = case(p, K)
    engine.cv_load(X, y, ids, K, 0.0)
    phi, phi_fold, r2_fold, info = engine.cv_shapley()
    probs = [engine.cv_get_problem(f) for f in range(K)]
    engine.cv_free()
    truth = R.shapley(v, p).astype(np.float64)
    print("p", p, "max |phi - truth|", np.abs(phi - truth).max())
    assert (info == 0).all()
    np.testing.assert_allclose(phi, truth, rtol=0, atol=1e-11)
    np.testing.assert_allclose(r2_fold, vf[-1].astype(np.float64), rtol=0, atol=1e-11)
    assert abs(phi.sum() - float(v[-1])) < 1e-11
    np.testing.assert_array_equal(phi, seq_sum(phi_fold.T))
    for f in range(K):
        load_reduced_fold(engine, probs[f])
        one, bits = engine.subsets_shapley()
        assert bits == 0
        np.testing.assert_array_equal(phi_fold[f], one)


def test_attribution_against_the_bootstrap_route(engine):
    p, K = 8, 4
    X, y, ids, v, vf = case(p, K)
    engine.cv_load(X, y, ids, K, 0.0)
    phi, phi_fold, _, _ = engine.cv_shapley()
    engine.cv_free()
    ind = (ids[None, :] == np.arange(K)[:, None]).astype(np.float64)
    engine.boot_load(X, X, y, y, 0.0)
    boot, _, info = engine.boot_run(K, 0, w_train=1.0 - ind, w_test=ind)
    engine.boot_free()
    assert (info == 0).all()
    share = np.array([(y[ids == f] ** 2).sum() for f in range(K)]) / (y ** 2).sum()
    np.testing.assert_allclose(phi_fold, boot * share[:, None], rtol=0, atol=1e-11)
    np.testing.assert_allclose(phi, (boot * share[:, None]).sum(axis=0), rtol=0, atol=1e-11)


# ---- 3. the values ---------------------------------------------------------------------------------------------------
def test_values_bitwise(engine):
    p, K = 10, 3
    X, y, ids, v, vf = case(p, K)
    masks = np.arange(1 << p, dtype=np.uint64)
    engine.cv_load(X, y, ids, K, 0.0)
    got_v, got_f = engine.debug_cv_values(masks)
    only_v, none = engine.debug_cv_values(masks, folds=False)
    probs = [engine.cv_get_problem(f) for f in range(K)]
    engine.cv_free()
    assert none is None
    np.testing.assert_array_equal(only_v, got_v)
    np.testing.assert_array_equal(got_v, seq_sum(got_f))
    np.testing.assert_allclose(got_f, vf.astype(np.float64), rtol=0, atol=1e-11)
    for f in range(K):
        load_reduced_fold(engine, probs[f])
        np.testing.assert_array_equal(got_f[:, f], engine.debug_subset_values(masks))


# ---- 4. the selection ------------------------------------------------------------------------------------------------
def check_selection(engine, p, K, include=0, steps=0):
    got = engine.cv_best(include, steps)
    v, masks, found, v_fold, info = got
    dv, df = engine.debug_cv_values(np.arange(1 << p, dtype=np.uint64))
    best, want_masks, want_found = arg_best(dv, p, include)
    assert (info == 0).all()
    np.testing.assert_array_equal(found, want_found)
    np.testing.assert_array_equal(masks, want_masks)
    np.testing.assert_array_equal(v[found], best[found])
    assert np.isnan(v[~found]).all() and (masks[~found] == 0).all() and np.isnan(v_fold[~found]).all()
    np.testing.assert_array_equal(v_fold[found], df[masks[found].astype(np.int64)])
    assert (popcount(masks[found]) == np.nonzero(found)[0]).all()
    return got


@pytest.mark.parametrize("K", [2, 5])
@pytest.mark.parametrize("p", [1, 6, 7, 12])
def test_selection_against_own_values_and_truth(engine, p, K):
    X, y, ids, v, vf = case(p, K)
    engine.cv_load(X, y, ids, K, 0.0)
    got_v, masks, found, _, _ = check_selection(engine, p, K)
    again = engine.cv_best()
    engine.cv_free()
    for a, b in zip((got_v, masks, found), again[:3]):
        np.testing.assert_array_equal(a, b)                   # two calls agree bitwise
    best, want_masks, want_found, runner = R.best(v, p)
    gap = (best.astype(np.float64) - runner)[1:p]
    print("p", p, "K", K, "smallest gap between winner and runner-up", gap.min() if len(gap) else None)
    assert (gap > 1e-9).all()                                 # a clear margin: the truth's winner is the device's
    np.testing.assert_array_equal(masks, want_masks)
    np.testing.assert_allclose(got_v, best.astype(np.float64), rtol=0, atol=1e-11)
    assert found.all() and got_v[0] == 0.0


def test_selection_exact_tie_smaller_mask_wins(engine):
    p, K = 8, 3
    X, _, ids, _, _ = case(p, K)
    X = X.copy()
    X[:, 5] = X[:, 0]                   # two identical columns, both among the low ones: the models {0} and {5} run
    rng = np.random.default_rng(1)      # the same operations on the same numbers and tie exactly
    y = 4.0 * X[:, 0] + 0.3 * X[:, 3] + 0.2 * rng.standard_normal(len(X))
    engine.cv_load(X, y, ids, K, 0.5)   # reg > 0: the subsets that hold both copies stay positive definite
    v, masks, found, _, _ = check_selection(engine, p, K)
    dv, _ = engine.debug_cv_values(np.array([1 << 0, 1 << 5, 1 << 3], dtype=np.uint64), folds=False)
    engine.cv_free()
    assert dv[0] == dv[1] and dv[0] > dv[2]
    assert int(masks[1]) == 1 << 0 and v[1] == dv[0]        # of the two equal winners of size 1 the smaller mask


@pytest.mark.parametrize("cols", [(1,), (8,), (0, 4, 7, 11)])
def test_selection_include(engine, cols):
    p, K = 12, 2
    X, y, ids, _, _ = case(p, K)
    inc = sum(1 << j for j in cols)
    engine.cv_load(X, y, ids, K, 0.0)
    _, masks, found, _, _ = check_selection(engine, p, K, include=inc)
    engine.cv_free()
    assert not found[:len(cols)].any() and found[len(cols):].all()
    assert ((masks[len(cols):] & inc) == inc).all()


def test_selection_does_not_depend_on_steps(engine):
    p, K = 14, 3
    X, y, ids, _, _ = case(p, K)
    engine.cv_load(X, y, ids, K, 0.0)
    plan = engine.debug_cv_plan(p, K)
    runs = [engine.cv_best(0, s) for s in (1, 3, plan["steps"], 0)]
    engine.cv_free()
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            np.testing.assert_array_equal(a, b)


def test_selection_several_units_and_launches(engine):
    """p = 20, K = 2: 8192 units of two steps each -- forced to one step a launch, the cut goes through a unit's subsets."""
    p, K = 20, 2
    X, y, ids, _, _ = case(p, K, n=200)
    engine.cv_load(X, y, ids, K, 0.0)
    plan = engine.debug_cv_plan(p, K)
    assert plan["units"] == 8192 and plan["per"] == 2 and plan["steps"] == 2 and plan["launches"] == 1
    v, masks, found, v_fold, info = engine.cv_best()
    cut = engine.cv_best(0, 1)
    assert engine.cv_timing()["launches"] == 2
    for a, b in zip((v, masks, found, v_fold), cut[:4]):
        np.testing.assert_array_equal(a, b)
    assert (info == 0).all() and found.all() and (popcount(masks) == np.arange(p + 1)).all()
    dv, df = engine.debug_cv_values(masks.astype(np.uint64))
    np.testing.assert_array_equal(v, dv)                    # the winner's value has the bits of its mask's debug value
    np.testing.assert_array_equal(v_fold, df)
    rng = np.random.default_rng(5)
    for k in range(1, p):                                   # no mask among 4096 random ones of its size beats it
        picks = np.array([sum(1 << int(j) for j in rng.choice(p, size=k, replace=False)) for _ in range(4096)],
                         dtype=np.uint64)
        rv, _ = engine.debug_cv_values(picks, folds=False)
        better = (rv > v[k]) | ((rv == v[k]) & (picks < masks[k]))
        assert not better.any(), (k, picks[better][:3], rv[better][:3], v[k])
    engine.cv_free()


# ---- 5. failed pivots ------------------------------------------------------------------------------------------------
def test_failed_pivot_in_one_fold(engine):
    p, K, n = 8, 3, 120
    X, y, _, _, _ = case(p, K)
    ids = (np.arange(n) % K).astype(np.int32)
    X = X.copy()
    X[ids != 1, 7] = 0.0                 # column 7 is constant zero in the training complement of fold 1
    engine.cv_load(X, y, ids, K, 0.0)
    v, masks, found, v_fold, info = engine.cv_best()
    engine.cv_free()
    assert info[1] & NOT_PD and info[0] == 0 and info[2] == 0
    assert found[:p].all() and not found[p] and np.isnan(v[p])          # the only subset of size p holds column 7
    assert ((masks[:p] >> 7) & 1 == 0).all()
    with pytest.warns(RuntimeWarning, match="fold.* 1 "):
        res = ls_spa_best_subsets_cv(X, y, folds=ids)
    assert np.isnan(res.r_squared[p]) and not res.subsets[p].any() and np.isnan(res.theta[p]).all()
    assert not np.isnan(res.r_squared[:p]).any() and res.best_size >= 0
    np.testing.assert_array_equal(res.r_squared[:p], v[:p])


# ---- 6. isolation ----------------------------------------------------------------------------------------------------
def test_isolation_and_reload(engine):
    from test_subsets_host import data
    d = data(9, seed=2)
    engine.load_data(*d, 0.0)
    before = engine.subsets_shapley(), engine.subsets_best()
    engine.boot_load(*d, 0.0)
    boot_before = engine.boot_run(3, 11)
    X, y, ids, _, _ = case(7, 2)
    engine.cv_load(X, y, ids, 2, 0.0)
    engine.cv_shapley()
    first = engine.cv_best()
    after = engine.subsets_shapley(), engine.subsets_best()
    boot_after = engine.boot_run(3, 11)
    for a, b in zip(before[0] + before[1] + boot_before, after[0] + after[1] + boot_after):
        np.testing.assert_array_equal(a, b)
    engine.cv_free()
    with pytest.raises(Exception, match="lsspa_cv_load comes first"):
        engine.cv_best()
    X2, y2, ids2, _, _ = case(12, 5)
    engine.cv_load(X2, y2, ids2, 5, 0.0)
    check_selection(engine, 12, 5)
    engine.cv_free()
    engine.cv_load(X, y, ids, 2, 0.0)
    for a, b in zip(first, engine.cv_best()):
        np.testing.assert_array_equal(a, b)
    engine.cv_free()
    engine.boot_free()


# ---- 7. the public calls ---------------------------------------------------------------------------------------------
def test_public_calls():
    p, K, n = 7, 5, 120
    X, y = R.data(p, n, seed=700)
    res = ls_spa_cv(X, y, folds=K, seed=7)
    assert isinstance(res, CVResults)
    ids = R.fold_ids(n, K, seed=7)
    np.testing.assert_array_equal(res.fold_ids, ids)
    v, vf = R.cv_values(X, y, ids, K)
    np.testing.assert_allclose(res.attribution, R.shapley(v, p).astype(np.float64), rtol=0, atol=1e-11)
    assert abs(res.r_squared - float(v[-1])) < 1e-11 and abs(res.attribution.sum() - res.r_squared) < 1e-11
    assert res.r_squared == float(seq_sum(res.fold_r_squared[None, :])[0])
    np.testing.assert_allclose(res.theta, np.linalg.lstsq(X, y, rcond=None)[0], rtol=1e-9)
    sel = ls_spa_best_subsets_cv(X, y, folds=K, seed=7, include=[3])
    assert isinstance(sel, CVBestSubsetsResults) and sel.sizes.tolist() == list(range(1, p + 1))
    best, masks, found, _ = R.best(v, p, include=1 << 3)
    for i, k in enumerate(sel.sizes):
        assert sum(1 << int(j) for j in np.nonzero(sel.subsets[i])[0]) == masks[k]
        cols = np.nonzero(sel.subsets[i])[0]
        np.testing.assert_allclose(sel.theta[i, cols], np.linalg.lstsq(X[:, cols], y, rcond=None)[0], rtol=1e-9)
        assert (sel.theta[i, ~sel.subsets[i]] == 0.0).all()
    np.testing.assert_allclose(sel.r_squared, best[1:].astype(np.float64), rtol=0, atol=1e-11)
    np.testing.assert_array_equal(sel.r_squared, seq_sum(sel.fold_r_squared))
    assert sel.full_r_squared == res.r_squared and sel.best_size == int(sel.sizes[np.argmax(sel.r_squared)])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ls_spa_cv(X, y, folds=ids, shuffle=False)
