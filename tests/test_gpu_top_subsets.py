"""ls_spa_top_subsets on the MI355X: the n_best best subsets of every size over all 2^p subsets (csrc/k_subsets.hip,
subsets_top_kernel and subsets_top_reduce_kernel) against the brute-force truth of tests/top_ref.py by value, against
the device's own values bit for bit (insert, threshold and reduce under the total order), on an integer design whose
ties are exact, with include sets, on planted additive truths where brute force cannot go (p = 28, several launches;
p = 32, mask bit 31), its contract with subsets_best, a Gram matrix that is not positive definite, and the public call."""
import warnings
from math import comb

import numpy as np
import pytest

import best_ref as B
import top_ref as T_
from ls_spa import TopSubsetsResults, ls_spa, ls_spa_best_subsets, ls_spa_top_subsets
from ls_spa._engine import debug_subsets_top_plan
from test_best_subsets_host import CASES
from test_subsets_host import data, gram_problem

pytestmark = pytest.mark.gpu

ORACLE_TOL = 1e-11


def popcount(masks):
    return np.array([bin(int(m)).count("1") for m in np.ravel(masks)]).reshape(np.shape(masks))


def check_shape(got, p, T, include=0):
    """What holds of every result: counts, padding, sizes, distinct masks that contain include, the order."""
    v, masks, count, info = got
    assert v.shape == masks.shape == (p + 1, T) and count.shape == (p + 1,)
    ni = bin(include).count("1")
    for k in range(p + 1):
        c = int(count[k])
        assert np.isnan(v[k, c:]).all() and (masks[k, c:] == 0).all() and not np.isnan(v[k, :c]).any()
        assert (popcount(masks[k, :c]) == k).all() and len(set(masks[k, :c].tolist())) == c
        assert ((masks[k, :c] & include) == include).all()
        lv, lm = v[k, :c], masks[k, :c]
        assert ((lv[1:] < lv[:-1]) | ((lv[1:] == lv[:-1]) & (lm[1:] > lm[:-1]))).all()
        if info == 0:
            assert c == (min(T, comb(p - ni, k - ni)) if k >= ni else 0)


def check_by_value(got, v_all, p, T, include=0, valid=None):
    """Near-ties in the truth cannot fail this: rank by rank the listed values are the truth's T largest of that size,
    and every listed mask has (nearly) the value listed for it."""
    v, masks, count, _ = got
    tv, _, tc = T_.top_truth(v_all, p, T, include, valid)
    np.testing.assert_array_equal(count, tc)
    sel = np.arange(T)[None, :] < count[:, None]
    err_rank = np.abs(v[sel] - tv[sel]).max()
    err_mask = np.abs(v_all[masks[sel].astype(np.int64)] - v[sel]).max()
    print("T", T, "max |v - truth| by rank", err_rank, "by mask", err_mask)
    assert err_rank <= ORACLE_TOL and err_mask <= ORACLE_TOL


# ---- 1. brute force ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p, reg", CASES)
def test_against_brute_force(engine, p, reg):
    d, v_all = B.brute_case(p, reg)
    n = d[0].shape[1]
    engine.load_data(*d, reg)
    assert engine.tri == (p != "edge")
    for T in (1, 3, 16):
        got = engine.subsets_top(0, T)
        assert got[3] == 0
        check_shape(got, n, T)
        check_by_value(got, v_all, n, T)
        assert got[0][0, 0] == 0.0 and got[1][0, 0] == 0 and got[1][n, 0] == (1 << n) - 1


# ---- 2. the device's own order, bitwise ----------------------------------------------------------------------------------
def own_order_data(kind, p):
    if kind == "random":
        return data(p, n=300, m=150, seed=900 + p)
    t = np.linspace(-1.0, 1.5, p)                 # ascending worths: later subsets are better, nearly every step inserts
    return T_.planted(t if kind == "ascending" else t[::-1], 910 + p)[0]


@pytest.mark.parametrize("kind", ["random", "ascending", "descending"])
@pytest.mark.parametrize("p", [16, 20])
def test_lists_are_the_top_of_the_devices_own_values(engine, p, kind):
    T = 16
    engine.load_data(*own_order_data(kind, p), 0.0)
    got = engine.subsets_top(0, T)
    v_dev = engine.debug_subset_values(np.arange(1 << p, dtype=np.uint64))
    tv, tm, tc = T_.top_truth(v_dev, p, T)
    assert got[3] == 0
    check_shape(got, p, T)
    np.testing.assert_array_equal(got[2], tc)
    np.testing.assert_array_equal(got[1], tm)
    np.testing.assert_array_equal(got[0], tv)            # NaN past count on both sides


# ---- 3. exact ties ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [3, 16])
@pytest.mark.parametrize("p", [9, 12])
def test_exact_ties_go_to_the_smaller_mask(engine, p, T):
    """Masks against the integer truth under "larger value, smaller mask".  Should the device's bits for two
    integer-tied subsets ever differ, test_lists_are_the_top_of_the_devices_own_values (the device's own values) remains
    the arbiter of the order: this test is not to be loosened for it."""
    engine.load_data(*T_.integer_design(p), 0.0)
    w = T_.integer_values(p)
    assert len(T_.ties_straddling_rank(w, p, T)) > 0           # the rule is exercised: a tie across the cut
    got = engine.subsets_top(0, T)
    _, tm, tc = T_.top_truth(w, p, T)
    assert got[3] == 0
    check_shape(got, p, T)
    np.testing.assert_array_equal(got[2], tc)
    np.testing.assert_array_equal(got[1], tm)
    sel = np.arange(T)[None, :] < tc[:, None]
    yy = float(T_.integer_design(p)[3] @ T_.integer_design(p)[3])
    np.testing.assert_allclose(got[0][sel], w[tm[sel].astype(np.int64)] / yy, rtol=0, atol=1e-14)
    np.testing.assert_array_equal(got[0][sel], engine.debug_subset_values(tm[sel].astype(np.uint64)))


# ---- 4. include ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1, 2])
@pytest.mark.parametrize("p", B.INCLUDE_P)
def test_include(engine, p, which):
    d, v_all = B.brute_case(p, 0.0)
    cols = B.include_sets(p)[which]
    inc = B.mask_of(cols)
    engine.load_data(*d, 0.0)
    for T in (3, 16):
        got = engine.subsets_top(inc, T)
        assert got[3] == 0
        check_shape(got, p, T, inc)
        check_by_value(got, v_all, p, T, inc)
        assert (got[2][:len(cols)] == 0).all() and (got[2][len(cols):] > 0).all()


# ---- 5. several launches -------------------------------------------------------------------------------------------------
def check_planted(engine, p, T, seed):
    d, _, vals, masks, gap = T_.planted_case(p, T, seed)
    assert gap > 1e-8                              # far above the few p eps by which the device's sums differ
    engine.load_data(*d, 0.0)
    got = engine.subsets_top(0, T)
    sel = np.isfinite(vals)
    print("max |v - planted|", np.abs(got[0][sel] - vals[sel]).max())
    assert got[3] == 0
    check_shape(got, p, T)
    np.testing.assert_array_equal(got[1], masks)
    np.testing.assert_allclose(got[0][sel], vals[sel], rtol=0, atol=ORACLE_TOL)
    assert engine.subsets_timing()[2] == debug_subsets_top_plan(p, T)["launches"]
    return got[1][sel]


def test_planted_truth_p28_over_several_launches(engine):
    listed = check_planted(engine, 28, 4, 2801).astype(np.int64)
    assert engine.subsets_timing()[2] > 1
    per_bits = 28 - 6 - 13                       # a unit's steps are the low bits of hi: early and late launches both win
    step = (listed >> 6) & ((1 << per_bits) - 1)
    units = listed >> (6 + per_bits)
    assert len(np.unique(units)) > 8 and step.min() < (1 << per_bits) // 4 and step.max() >= 3 * (1 << per_bits) // 4


def test_planted_truth_p32(engine):
    listed = check_planted(engine, 32, 2, 3201)
    assert (listed >> 31).any() and not (listed >> 31).all()
    assert engine.subsets_timing()[2] == 64


# ---- 6. contract ---------------------------------------------------------------------------------------------------------
def test_contract_with_subsets_best_prefixes_determinism_and_isolation(engine):
    d = data(20, n=300, m=150, seed=720)
    engine.load_data(*d, 0.0)
    phi0, _ = engine.subsets_shapley()
    best0 = engine.subsets_best()
    top16 = engine.subsets_top(0, 16)
    timing = engine.subsets_timing()
    assert timing[2] >= 1 and timing[0] > 0
    again = engine.subsets_top(0, 16)
    phi1, _ = engine.subsets_shapley()
    best1 = engine.subsets_best()
    for a, b in zip(top16, again):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(phi0, phi1)
    for a, b in zip(best0, best1):
        np.testing.assert_array_equal(a, b)
    for inc in (0, 0b1000001):
        v, masks, found, _ = engine.subsets_best(inc)
        tv, tm, tc, _ = engine.subsets_top(inc, 16)
        np.testing.assert_array_equal(tc > 0, found)
        np.testing.assert_array_equal(tm[:, 0], masks)
        np.testing.assert_array_equal(tv[:, 0], v)                     # NaN where nothing was found on both sides
        for T in (1, 3):
            sv, sm, sc, _ = engine.subsets_top(inc, T)
            np.testing.assert_array_equal(sv, tv[:, :T])
            np.testing.assert_array_equal(sm, tm[:, :T])
            np.testing.assert_array_equal(sc, np.minimum(tc, T))
    np.testing.assert_array_equal(engine.subsets_shapley()[0], phi0)


def test_kept_engine_sampling_unchanged_by_a_top_subsets_call():
    d = data(12, n=200, m=100, seed=12)
    kw = dict(method="argsort", seed=7, max_samples=512, batch_size=128, tolerance=0.0)
    before = ls_spa(*d, **kw)
    ls_spa_top_subsets(*d, n_best=4)
    after = ls_spa(*d, **kw)
    np.testing.assert_array_equal(before.attribution, after.attribution)
    np.testing.assert_array_equal(before.error_history, after.error_history)
    np.testing.assert_array_equal(before.attribution_errors, after.attribution_errors)


# ---- 7. not positive definite ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a, b", [(2, 7), (6, 7), (1, 4)])       # low and high, both high (the wave's pivot), both low
def test_duplicate_column(engine, a, b):
    p, T = 8, 16
    Xa, Xe, ya, ye = data(p, seed=80)
    Xa[:, b], Xe[:, b] = Xa[:, a], Xe[:, a]
    engine.load_data(Xa, Xe, ya, ye, 0.0)
    got = engine.subsets_top(0, T)
    v, masks, count, info = got
    both = (1 << a) | (1 << b)
    all_masks = np.arange(1 << p, dtype=np.int64)
    valid = (all_masks & both) != both
    assert info & 1
    check_shape(got, p, T)
    sel = np.arange(T)[None, :] < count[:, None]
    assert ((masks[sel] & both) != both).all() and count[p] == 0 and (count[:p] > 0).all()
    # the truth without the copy: a valid subset with b in place of a has the value of the one with a
    keep = [j for j in range(p) if j != b]
    v7 = B.all_values((Xa[:, keep], Xe[:, keep], ya, ye))
    swapped = np.where(all_masks & (1 << b), (all_masks & ~(1 << b)) | (1 << a), all_masks)
    squeeze = ((swapped >> (b + 1)) << b) | (swapped & ((1 << b) - 1))           # drop bit b (0 everywhere now)
    v8 = np.where(valid, v7[np.where(valid, squeeze, 0)], np.nan)
    check_by_value(got, v8, p, T, valid=valid)
    if a >= 6:       # the hook refuses a high subset if ANY of its 64 lanes fails: it can answer for two high copies only
        v_dev = np.full(1 << p, np.nan)
        v_dev[valid] = engine.debug_subset_values(all_masks[valid].astype(np.uint64))
        tv, tm, tc = T_.top_truth(v_dev, p, T, valid=valid)
        np.testing.assert_array_equal(count, tc)
        np.testing.assert_array_equal(masks, tm)
        np.testing.assert_array_equal(v, tv)
    with pytest.warns(RuntimeWarning, match="not numerically positive definite"):
        res = ls_spa_top_subsets(Xa, Xe, ya, ye, n_best=3)
    assert res.n_models[p] == 0 and np.isnan(res.r_squared[p]).all() and np.isnan(res.theta[p]).all()
    assert res.best_size < p and np.isfinite(res.theta[:p, 0]).all()


# ---- 8. the public call ---------------------------------------------------------------------------------------------------
def test_public_call():
    p, reg, T = 12, 0.1, 5
    d, v_all = B.brute_case(p, reg)
    inc = B.mask_of((3, 8))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        res = ls_spa_top_subsets(*d, reg=reg, n_best=T, include=[3, 8])
        best = ls_spa_best_subsets(*d, reg=reg, include=[3, 8])
    assert isinstance(res, TopSubsetsResults)
    n = p - 1
    assert res.sizes.tolist() == list(range(2, p + 1))
    assert res.n_models.tolist() == [min(T, comb(p - 2, k - 2)) for k in res.sizes]
    assert res.subsets.shape == (n, T, p) and res.theta.shape == (n, T, p) and res.subsets.dtype == bool
    assert res.r_squared.shape == res.gap.shape == (n, T)
    valid = np.arange(T)[None, :] < res.n_models[:, None]
    assert np.isnan(res.r_squared[~valid]).all() and np.isnan(res.theta[~valid]).all() and not res.subsets[~valid].any()
    assert np.isnan(res.gap[~valid]).all() and (res.gap[:, 0] == 0.0).all() and (res.gap[valid] >= 0.0).all()
    tv = T_.top_truth(v_all, p, T, inc)[0][2:]
    np.testing.assert_allclose(res.r_squared[valid], tv[valid], rtol=0, atol=ORACLE_TOL)
    G, g, H, h, yy = gram_problem(*d, reg=reg)
    listed = np.zeros((n, T), dtype=np.int64)
    for i in range(n):
        for r in range(res.n_models[i]):
            cols = np.nonzero(res.subsets[i, r])[0]
            listed[i, r] = B.mask_of(cols)
            assert len(cols) == res.sizes[i] and res.subsets[i, r, [3, 8]].all()
            assert (res.theta[i, r, ~res.subsets[i, r]] == 0.0).all()
            np.testing.assert_allclose(res.theta[i, r, cols], np.linalg.solve(G[np.ix_(cols, cols)], g[cols]),
                                       rtol=1e-9, atol=1e-12)
    # best_* and rank 0 are ls_spa_best_subsets', bit for bit
    assert res.best_size == best.best_size and res.full_r_squared == best.full_r_squared
    np.testing.assert_array_equal(res.best_subset, best.best_subset)
    np.testing.assert_array_equal(res.subsets[:, 0], best.subsets)
    np.testing.assert_array_equal(res.r_squared[:, 0], best.r_squared)
    np.testing.assert_array_equal(res.theta[:, 0], best.theta)
    # the overall list: a host merge of the per-size lists under the same order
    order = np.lexsort((listed[valid], -res.r_squared[valid]))[:T]
    np.testing.assert_array_equal(res.top_r_squared, res.r_squared[valid][order])
    assert [B.mask_of(np.nonzero(s)[0]) for s in res.top_subsets] == listed[valid][order].tolist()
    assert res.top_sizes.tolist() == popcount(listed[valid][order]).tolist()
    assert res.top_r_squared[0] == np.nanmax(res.r_squared) and (np.diff(res.top_r_squared) <= 0).all()


def test_refusals(engine):
    with pytest.raises(ValueError, match="at most p = 32"):
        ls_spa_top_subsets(*data(33, n=80, m=60, seed=33))
    with pytest.raises(ValueError, match="integer in 1 .. 16"):
        ls_spa_top_subsets(*data(9), n_best=17)
    with pytest.raises(ValueError, match="outside 0 .. 8"):
        ls_spa_top_subsets(*data(9), include=[9])
    engine.load_data(*data(9, seed=1), 0.0)
    with pytest.raises(ValueError, match="include names a feature beyond p"):
        engine.subsets_top(1 << 9, 4)
    for T in (0, 17, -3):
        with pytest.raises(ValueError, match="1 .. 16 subsets of every size"):
            engine.subsets_top(0, T)
    engine.load_data(*data(33, n=80, m=60, seed=33), 0.0)
    with pytest.raises(ValueError, match="at most p = 32"):
        engine.subsets_top(0, 4)
