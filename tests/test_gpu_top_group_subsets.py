"""ls_spa_top_group_subsets on the MI355X: the n_best best sets of groups of every size over all 2^g group subsets
(csrc/k_groups.hip, groups_top_kernel, and k_subsets.hip's subsets_top_reduce_kernel) against the brute-force truth of
tests/group_best_ref.py, against the device's own values bit for bit (insert, threshold, shift, store-back and reduce
under the total order), on exact ties under two numberings, on planted additive truths where brute force cannot go
(g = 20 over several launches; g = 28, per = 512), its contract with groups_best, against the column call on
singletons, a Gram matrix that is not positive definite, and the public call."""
import warnings
from math import comb

import numpy as np
import pytest

import best_ref as B
import group_best_ref as R
import group_top_ref as GT
import top_ref as T_
from ls_spa import TopGroupSubsetsResults, ls_spa, ls_spa_best_subsets, ls_spa_top_group_subsets
from ls_spa._engine import debug_groups_top_plan
from test_groups_host import group_values
from test_subsets_host import data, gram_problem

pytestmark = pytest.mark.gpu

ORACLE_TOL = 1e-11      # the project's bound for these enumerations (tests/test_gpu_groups.py)
NAMES = [n for n in R.CASES if n not in R.RECT]


def popcount(masks):
    return np.array([bin(int(m)).count("1") for m in np.ravel(masks)]).reshape(np.shape(masks))


def check_shape(got, g, T):
    """What holds of every result: counts, padding, sizes, distinct masks, the strict order."""
    u, masks, count, info = got
    assert u.shape == masks.shape == (g + 1, T) and count.shape == (g + 1,) and masks.dtype == np.uint32
    for k in range(g + 1):
        c = int(count[k])
        assert np.isnan(u[k, c:]).all() and (masks[k, c:] == 0).all() and not np.isnan(u[k, :c]).any()
        assert (popcount(masks[k, :c]) == k).all() and len(set(masks[k, :c].tolist())) == c
        lv, lm = u[k, :c], masks[k, :c]
        assert ((lv[1:] < lv[:-1]) | ((lv[1:] == lv[:-1]) & (lm[1:] > lm[:-1]))).all()
        if info == 0:
            assert c == min(T, comb(g, k))


def check_against_truth(engine, labels, u_all, T):
    g = int(labels.max()) + 1
    got = engine.groups_top(labels, T)
    tv, tm, tc = T_.top_truth(u_all, g, T)
    sel = np.arange(T)[None, :] < tc[:, None]
    print("T", T, "max |u - truth|", np.abs(got[0][sel] - tv[sel]).max())
    assert got[3] == 0
    check_shape(got, g, T)
    np.testing.assert_array_equal(got[2], tc)
    np.testing.assert_array_equal(got[1], tm)            # the host test vouches for the gaps: masks compare exactly
    np.testing.assert_allclose(got[0][sel], tv[sel], rtol=0, atol=ORACLE_TOL)
    best = engine.groups_best(labels)
    np.testing.assert_array_equal(got[0][:, 0], best[0])
    np.testing.assert_array_equal(got[1][:, 0], best[1])
    np.testing.assert_array_equal(got[2] > 0, best[2])


# ---- 1. brute force ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reg", R.REGS)
@pytest.mark.parametrize("name", NAMES)
def test_against_brute_force(engine, name, reg):
    d, labels, u_all = R.brute_case(name, reg)
    engine.load_data(*d, reg)
    assert engine.tri
    for T in (1, 3, 16):
        check_against_truth(engine, labels, u_all, T)


@pytest.mark.parametrize("reg", R.REGS)
def test_against_brute_force_in_rect_mode(engine, reg):
    d, labels, u_all = R.brute_case(R.RECT[0], reg)
    engine.load_data(*d, reg)
    assert not engine.tri
    for T in (1, 3, 16):
        check_against_truth(engine, labels, u_all, T)


def test_the_cases_reach_the_edges():
    plans = {name: debug_groups_top_plan(R.case_labels(name), 16) for name in R.CASES}
    assert plans["gl0"]["gl"] == 0 and plans["gl6"]["gl"] == 6 and plans["alllow"]["gh"] == 0
    assert plans["alllow"]["units"] == 1 and plans["g12p64"]["units"] == 2048
    assert any(q["nb"] > 0 for q in plans.values()) and any(q["nb"] == 0 for q in plans.values())


# ---- 2. the device's own order, bitwise ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["g12p64", "gl0", "gl6"])
def test_lists_are_the_top_of_the_devices_own_values(engine, name):
    T = 16
    d, labels, _ = R.brute_case(name, 0.0)
    g = int(labels.max()) + 1
    engine.load_data(*d, 0.0)
    got = engine.groups_top(labels, T)
    u_dev = engine.debug_group_values(labels, np.arange(1 << g, dtype=np.uint64))
    tv, tm, tc = T_.top_truth(u_dev, g, T)
    assert got[3] == 0
    check_shape(got, g, T)
    np.testing.assert_array_equal(got[2], tc)
    np.testing.assert_array_equal(got[1], tm)
    np.testing.assert_array_equal(got[0], tv)            # NaN past count on both sides


# ---- 3. exact ties -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 2, 3, 16])
@pytest.mark.parametrize("run", list(R.TIE_RUNS))
def test_exact_ties_go_to_the_smaller_caller_mask(engine, run, T):
    d, labels, u_all = R.tie_case(run)
    engine.load_data(*d, 0.0)
    got = engine.groups_top(labels, T)
    tv, tm, tc = T_.top_truth(u_all, 5, T)
    print(run, T, "masks", got[1].tolist())
    assert got[3] == 0
    check_shape(got, 5, T)
    np.testing.assert_array_equal(got[2], tc)
    np.testing.assert_array_equal(got[1], tm)
    lab = R.TIE_RUNS[run]
    abc = sum(1 << lab[k] for k in "abc")
    sel = np.arange(T)[None, :] < tc[:, None]
    inside = sel & ((got[1] & ~np.uint32(abc)) == 0)
    assert inside.sum() >= min(T, 3) and (got[0][inside] == 0.0).all()
    np.testing.assert_array_equal(got[0][sel], engine.debug_group_values(labels, got[1][sel].astype(np.uint64)))


# ---- 4. planted truth over several launches ------------------------------------------------------------------------------
@pytest.mark.parametrize("name, seed, T", GT.PLANTED_RUNS)
def test_planted_truth_over_several_launches(engine, name, seed, T):
    d, labels, _, vals, masks, gap = GT.planted_case(name, seed, T)
    plan = R.PLANTED[name][1]
    g = int(labels.max()) + 1
    assert gap > 1e-6
    engine.load_data(*d, 0.0)
    got = engine.groups_top(labels, T)
    sel = np.isfinite(vals)
    print("max |u - planted|", np.abs(got[0][sel] - vals[sel]).max(), "gap", gap)
    assert got[3] == 0
    check_shape(got, g, T)
    np.testing.assert_array_equal(got[1], masks)
    np.testing.assert_allclose(got[0][sel], vals[sel], rtol=0, atol=ORACLE_TOL)
    assert engine.groups_timing()[2] == plan["launches"] > 1
    assert debug_groups_top_plan(labels, T)["launches"] == plan["launches"]
    # equal sizes: the low groups are labels 0 .. gl-1, the high ones follow in order, so hi = mask >> gl; a unit's
    # steps are the low bits of hi: the lists are loaded, extended and stored across early and late launches, in many units
    per_bits = plan["per"].bit_length() - 1
    hi = got[1][sel].astype(np.int64) >> plan["gl"]
    step, units = hi & (plan["per"] - 1), hi >> per_bits
    assert len(np.unique(units)) > 8 and step.min() < plan["per"] // 4 and step.max() >= 3 * plan["per"] // 4
    launch = step // debug_groups_top_plan(labels, T)["steps"]
    assert launch.min() == 0 and launch.max() == plan["launches"] - 1


# ---- 5. contract ---------------------------------------------------------------------------------------------------------
def test_contract_with_groups_best_and_the_other_grouped_calls(engine):
    d, labels, _ = R.brute_case("g12p64", 0.0)
    g = 12
    d16 = data(16, n=200, m=120, seed=716)
    engine.load_data(*d, 0.0)
    phi0, _ = engine.groups_shapley(labels)
    best0 = engine.groups_best(labels)
    first = engine.groups_top(labels, 16)
    timing = engine.groups_timing()
    assert timing[2] >= 1 and timing[0] > 0
    again = engine.groups_top(labels, 16)
    for a, b in zip(first, again):
        np.testing.assert_array_equal(a, b)
    for T in (1, 3):
        u, masks, count, info = engine.groups_top(labels, T)
        np.testing.assert_array_equal(u, first[0][:, :T])
        np.testing.assert_array_equal(masks, first[1][:, :T])
        np.testing.assert_array_equal(count, np.minimum(first[2], T))
        assert info == first[3] == 0
    best1 = engine.groups_best(labels)
    phi1, _ = engine.groups_shapley(labels)
    for a, b in zip(best0, best1):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(phi0, phi1)
    np.testing.assert_array_equal(first[0][:, 0], best0[0])
    np.testing.assert_array_equal(first[1][:, 0], best0[1])
    np.testing.assert_array_equal(first[2] > 0, best0[2])
    assert first[0].shape == (g + 1, 16)
    engine.load_data(*d16, 0.0)
    sub0, _ = engine.subsets_shapley()
    engine.groups_top(np.arange(16) // 2, 5)
    np.testing.assert_array_equal(engine.subsets_shapley()[0], sub0)


def test_kept_engine_sampling_unchanged_by_a_public_call():
    d = data(12, n=200, m=100, seed=12)
    kw = dict(method="argsort", seed=7, max_samples=512, batch_size=128, tolerance=0.0)
    before = ls_spa(*d, **kw)
    ls_spa_top_group_subsets(*d, np.arange(12) // 3, n_best=4)
    after = ls_spa(*d, **kw)
    np.testing.assert_array_equal(before.attribution, after.attribution)
    np.testing.assert_array_equal(before.error_history, after.error_history)
    np.testing.assert_array_equal(before.attribution_errors, after.attribution_errors)


# ---- 6. all singletons ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [9, 12])
def test_singletons_list_what_the_column_call_lists(engine, p):
    T = 16
    d, _ = B.brute_case(p, 0.0)
    engine.load_data(*d, 0.0)
    v, cmasks, ccount, _ = engine.subsets_top(0, T)
    u, masks, count, info = engine.groups_top(np.arange(p), T)
    assert info == 0
    check_shape((u, masks, count, info), p, T)
    np.testing.assert_array_equal(count, ccount)
    sel = np.arange(T)[None, :] < count[:, None]
    np.testing.assert_allclose(u[sel], v[sel], rtol=0, atol=ORACLE_TOL)       # (another arithmetic: not bitwise)
    # ranks whose value is clear of both neighbours list the same mask
    clear = np.zeros_like(sel)
    for k in range(p + 1):
        step = np.abs(np.diff(v[k, :count[k]]))
        clear[k, :count[k]] = (np.concatenate([[np.inf], step]) > 1e-8) & (np.concatenate([step, [np.inf]]) > 1e-8)
    assert clear.sum() > sel.sum() // 2
    np.testing.assert_array_equal(masks[clear], cmasks[clear])


# ---- 7. not positive definite ---------------------------------------------------------------------------------------------
# sizes 1, 2, 2 are low (5 columns), 4 and 4 high; the copy of a column of group a replaces a column of group b
@pytest.mark.parametrize("a, b", [(0, 1), (3, 4), (2, 3)])       # both low, both high (the workgroup's pivot), one of each
def test_duplicate_column(engine, a, b):
    T = 16
    labels = np.repeat(np.arange(5), [1, 2, 2, 4, 4])
    g, p = 5, 13
    plan = debug_groups_top_plan(labels, T)
    assert plan["gl"] == 3 and plan["gh"] == 2
    Xa, Xe, ya, ye = data(p, seed=81)
    ja, jb = np.nonzero(labels == a)[0][0], np.nonzero(labels == b)[0][-1]
    Xa[:, jb], Xe[:, jb] = Xa[:, ja], Xe[:, ja]
    engine.load_data(Xa, Xe, ya, ye, 0.0)
    got = engine.groups_top(labels, T)
    u, masks, count, info = got
    both = (1 << a) | (1 << b)
    assert info & 1
    check_shape(got, g, T)
    sel = np.arange(T)[None, :] < count[:, None]
    assert ((masks[sel] & both) != both).all()
    assert count.tolist() == [comb(5, k) - (comb(3, k - 2) if k >= 2 else 0) for k in range(g + 1)] and count[g] == 0
    all_masks = np.arange(1 << g)
    valid = (all_masks & both) != both
    u_all = np.full(1 << g, np.nan)
    u_all[valid] = group_values(*gram_problem(Xa, Xe, ya, ye), labels, all_masks[valid])
    tv, tm, tc = T_.top_truth(u_all, g, T, valid=valid)
    np.testing.assert_array_equal(count, tc)
    np.testing.assert_allclose(u[sel], tv[sel], rtol=0, atol=ORACLE_TOL)
    np.testing.assert_allclose(u[sel], u_all[masks[sel].astype(np.int64)], rtol=0, atol=ORACLE_TOL)
    with pytest.warns(RuntimeWarning, match="not numerically positive definite"):
        res = ls_spa_top_group_subsets(Xa, Xe, ya, ye, labels, n_best=T)
    assert res.n_models[g] == 0 and np.isnan(res.r_squared[g]).all() and np.isnan(res.theta[g]).all()
    assert 0 <= res.best_size < g and np.isfinite(res.theta[:g, 0]).all()


# ---- 8. the public call ---------------------------------------------------------------------------------------------------
def test_public_call():
    reg, T = 0.1, 5
    d, labels, u_all = R.brute_case("nine", reg)
    g, p = int(labels.max()) + 1, len(labels)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        res = ls_spa_top_group_subsets(*d, labels, reg=reg, n_best=T)
        best = ls_spa_best_subsets(*d, reg=reg, groups=labels)
        full = ls_spa(*d, reg=reg, method="subsets", groups=labels)
    assert isinstance(res, TopGroupSubsetsResults)
    tv, tm, tc = T_.top_truth(u_all, g, T)
    n = g + 1
    assert res.sizes.tolist() == list(range(n)) and res.n_models.tolist() == tc.tolist()
    assert res.group_subsets.shape == (n, T, g) and res.subsets.shape == (n, T, p) and res.theta.shape == (n, T, p)
    valid = np.arange(T)[None, :] < tc[:, None]
    np.testing.assert_allclose(res.r_squared[valid], tv[valid], rtol=0, atol=ORACLE_TOL)
    assert np.isnan(res.r_squared[~valid]).all() and np.isnan(res.theta[~valid]).all() and np.isnan(res.gap[~valid]).all()
    assert not res.subsets[~valid].any() and not res.group_subsets[~valid].any() and (res.n_columns[~valid] == 0).all()
    np.testing.assert_array_equal(res.gap[valid], np.broadcast_to(res.r_squared[:, :1], (n, T))[valid] - res.r_squared[valid])
    G, gv, H, h, yy = gram_problem(*d, reg=reg)
    for k in range(n):
        for r in range(tc[k]):
            assert B.mask_of(np.nonzero(res.group_subsets[k, r])[0]) == tm[k, r]
            np.testing.assert_array_equal(res.subsets[k, r], R.columns_of(labels, tm[k, r]))
            cols = np.nonzero(res.subsets[k, r])[0]
            assert res.n_columns[k, r] == len(cols) and (res.theta[k, r, ~res.subsets[k, r]] == 0.0).all()
            np.testing.assert_allclose(res.theta[k, r, cols], np.linalg.solve(G[np.ix_(cols, cols)], gv[cols]),
                                       rtol=1e-9, atol=1e-12)
    # the overall list: the merge of all 2^g values under the same order
    order = np.lexsort((np.arange(1 << g), -u_all))[:T]
    assert [B.mask_of(np.nonzero(s)[0]) for s in res.top_group_subsets] == order.tolist()
    assert res.top_sizes.tolist() == popcount(order).tolist()
    np.testing.assert_allclose(res.top_r_squared, u_all[order], rtol=0, atol=ORACLE_TOL)
    for s, c in zip(res.top_group_subsets, res.top_subsets):
        np.testing.assert_array_equal(c, R.columns_of(labels, B.mask_of(np.nonzero(s)[0])))
    # rank 0 and best_* are ls_spa_best_subsets(groups=)'s, bit for bit
    np.testing.assert_array_equal(res.r_squared[:, 0], best.r_squared)
    np.testing.assert_array_equal(res.group_subsets[:, 0], best.group_subsets)
    np.testing.assert_array_equal(res.subsets[:, 0], best.subsets)
    np.testing.assert_array_equal(res.n_columns[:, 0], best.n_columns)
    np.testing.assert_array_equal(res.theta[:, 0], best.theta)
    assert res.best_size == best.best_size and res.baseline_r_squared == best.baseline_r_squared
    np.testing.assert_array_equal(res.best_group_subset, best.best_group_subset)
    np.testing.assert_array_equal(res.best_subset, best.best_subset)
    assert res.full_r_squared == best.full_r_squared == full.r_squared


def test_refused_by_the_library(engine):
    engine.load_data(*data(9, seed=1), 0.0)
    with pytest.raises(ValueError, match="no column"):
        engine.groups_top([0, 0, 0, 2, 2, 2, 3, 3, 3], 4)
    with pytest.raises(ValueError, match="outside -1 .. g-1"):
        engine.groups_top([0, 0, 0, 1, 1, 1, -2, 2, 2], 4)
    with pytest.raises(ValueError, match="length p = 9"):
        engine.groups_top([0, 1], 4)
    for T in (0, 17, -3):
        with pytest.raises(ValueError, match="keeps 1 .. 16 subsets of every size"):
            engine.groups_top(np.arange(9) // 3, T)


def test_refused_by_the_driver():
    with pytest.raises(ValueError, match="at most p = 64"):
        ls_spa_top_group_subsets(*data(65, n=140, m=100, seed=1), np.arange(65) % 8)
    with pytest.raises(ValueError, match="integer in 1 .. 16"):
        ls_spa_top_group_subsets(*data(6), [0, 0, 1, 1, 2, 2], n_best=17)
    with pytest.raises(TypeError, match="include"):
        ls_spa_top_group_subsets(*data(6), [0, 0, 1, 1, 2, 2], include=[0])
