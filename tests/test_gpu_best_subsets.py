"""ls_spa_best_subsets on the MI355X: the best subset of every size over all 2^p subsets (csrc/k_subsets.hip,
subsets_best_kernel) against the brute-force truth of tests/best_ref.py, against the device's own values, against a
planted additive truth where brute force cannot go (p = 28, several launches; p = 32, mask bit 31), its determinism and
isolation, a Gram matrix that is not positive definite, and the public call."""
import warnings

import numpy as np
import pytest

import best_ref as B
from ls_spa import BestSubsetsResults, ls_spa, ls_spa_best_subsets
from test_best_subsets_host import CASES
from test_subsets_host import data, gram_problem

pytestmark = pytest.mark.gpu

ORACLE_TOL = dict(rtol=0, atol=1e-11)


def popcount(masks):
    return np.array([bin(int(m)).count("1") for m in masks])


def check_against_truth(got, v_all, p, include=0):
    v, masks, found, info = got
    best, want_masks, want_found, _ = B.best_truth(v_all, p, include)
    print("max |v - truth|", np.nanmax(np.abs(v - best)), "masks", [hex(int(m)) for m in masks])
    assert info == 0
    np.testing.assert_array_equal(found, want_found)
    np.testing.assert_array_equal(masks, want_masks)
    np.testing.assert_allclose(v[found], best[found], **ORACLE_TOL)
    assert np.isnan(v[~found]).all() and (masks[~found] == 0).all()


# ---- 1. brute force ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p, reg", CASES)
def test_against_brute_force(engine, p, reg):
    d, v_all = B.brute_case(p, reg)
    n = d[0].shape[1]
    engine.load_data(*d, reg)
    assert engine.tri == (p != "edge")
    got = engine.subsets_best()
    check_against_truth(got, v_all, n)
    assert got[0][0] == 0.0 and got[1][0] == 0 and got[1][n] == (1 << n) - 1


# ---- 2. include --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1, 2])
@pytest.mark.parametrize("p", B.INCLUDE_P)
def test_include(engine, p, which):
    d, v_all = B.brute_case(p, 0.0)
    cols = B.include_sets(p)[which]
    inc = B.mask_of(cols)
    engine.load_data(*d, 0.0)
    got = engine.subsets_best(inc)
    check_against_truth(got, v_all, p, inc)
    assert not got[2][:len(cols)].any() and got[2][len(cols):].all()
    assert ((got[1][len(cols):] & inc) == inc).all()


# ---- 3. the device's own values ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [16, 20])
def test_winners_carry_the_devices_own_values_and_beat_their_neighbours(engine, p):
    d = data(p, n=300, m=150, seed=700 + p)
    engine.load_data(*d, 0.0)
    v, masks, found, info = engine.subsets_best()
    assert info == 0 and found.all()
    np.testing.assert_array_equal(popcount(masks), np.arange(p + 1))
    np.testing.assert_array_equal(v, engine.debug_subset_values(masks.astype(np.uint64)))
    nb, size = [], []
    for k in range(1, p):
        m = int(masks[k])
        ins = [i for i in range(p) if (m >> i) & 1]
        outs = [j for j in range(p) if not (m >> j) & 1]
        nb += [(m ^ (1 << i)) | (1 << j) for i in ins for j in outs]
        size += [k] * (len(ins) * len(outs))
    nb, size = np.array(nb, dtype=np.uint64), np.array(size)
    assert len(nb) < 5000
    nv = engine.debug_subset_values(nb)
    assert (nv <= v[size]).all()
    equal = nv == v[size]
    assert (nb[equal] > masks[size[equal]]).all()


# ---- 4. planted truth --------------------------------------------------------------------------------------------------
def planted(p, seed):
    """Orthonormal columns on both sides: G = I / N and H = I to rounding, so v(K) = sum_{j in K} d_j with
    d_j = (2 a_j b_j - a_j^2) / ||y_test||^2, a = X_train^T y_train, b = X_test^T y_test.  With a_j = 1 and
    b_j = (1 + t_j) / 2 that is d_j = t_j / ||y_test||^2: the t_j are p values from -1 to 1.5 in a shuffled order, more
    than 0.08 apart, and ||y_test||^2 < 60, so the d_j are more than 1e-3 apart (the issue asks for 1e-6) and of both
    signs."""
    rng = np.random.default_rng(seed)
    n = 2 * p + 8
    Qa = np.linalg.qr(rng.standard_normal((n, p)))[0]
    Qe = np.linalg.qr(rng.standard_normal((n, p)))[0]
    t = np.linspace(-1.0, 1.5, p)[rng.permutation(p)]
    noise = rng.standard_normal(n)
    noise -= Qe @ (Qe.T @ noise)
    ya, ye = Qa @ np.ones(p), Qe @ ((1.0 + t) / 2.0) + noise
    a, b, yy = Qa.T @ ya, Qe.T @ ye, float(ye @ ye)
    dj = (2.0 * a * b - a * a) / yy
    assert yy < 60 and np.diff(np.sort(dj)).min() > 1e-6 and (dj > 0).any() and (dj < 0).any()
    return (Qa, Qe, ya, ye), dj


def check_planted(engine, p, seed):
    d, dj = planted(p, seed)
    engine.load_data(*d, 0.0)
    v, masks, found, info = engine.subsets_best()
    order = np.argsort(-dj)
    want_v = np.concatenate([[0.0], np.cumsum(dj[order])])
    want_masks = np.concatenate([np.zeros(1, dtype=np.uint64),
                                 np.cumsum(np.uint64(1) << order.astype(np.uint64))]).astype(np.uint32)
    print("max |v - planted|", np.abs(v - want_v).max(), "winners", [hex(int(m)) for m in masks])
    assert info == 0 and found.all()
    np.testing.assert_array_equal(masks, want_masks)
    np.testing.assert_allclose(v, want_v, **ORACLE_TOL)        # additivity holds to a few p eps: G, H diagonal to rounding
    assert int(np.argmax(v)) == int((dj > 0).sum())
    return masks


def test_planted_truth_p28_over_several_launches(engine):
    masks = check_planted(engine, 28, seed=2800)
    assert engine.subsets_timing()[2] > 1
    per_bits = 28 - 6 - 13                       # a unit's steps are the low bits of hi: early and late launches both win
    step = (masks.astype(np.int64) >> 6) & ((1 << per_bits) - 1)
    units = masks.astype(np.int64) >> (6 + per_bits)
    assert len(np.unique(units)) > 8 and step.min() < (1 << per_bits) // 4 and step.max() >= 3 * (1 << per_bits) // 4


def test_planted_truth_p32(engine):
    masks = check_planted(engine, 32, seed=3200)
    assert masks[32] == 0xFFFFFFFF and (masks[1:] >> 31).any() and not (masks[1:] >> 31).all()
    assert engine.subsets_timing()[2] == 64


# ---- 5. determinism and isolation -----------------------------------------------------------------------------------------
def test_two_calls_agree_and_shapley_is_untouched(engine):
    d = data(20, n=300, m=150, seed=720)
    engine.load_data(*d, 0.0)
    phi0, _ = engine.subsets_shapley()
    first = engine.subsets_best()
    timing = engine.subsets_timing()
    assert timing[2] >= 1 and timing[0] > 0
    again = engine.subsets_best()
    phi1, _ = engine.subsets_shapley()
    for a, b in zip(first, again):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(phi0, phi1)
    inc = engine.subsets_best(0b1000001)
    np.testing.assert_array_equal(engine.subsets_shapley()[0], phi0)
    assert (inc[0][2:] <= first[0][2:]).all()          # fewer candidates never win more


def test_kept_engine_sampling_unchanged_by_a_best_subsets_call():
    d = data(12, n=200, m=100, seed=12)
    kw = dict(method="argsort", seed=7, max_samples=512, batch_size=128, tolerance=0.0)
    before = ls_spa(*d, **kw)
    ls_spa_best_subsets(*d)
    after = ls_spa(*d, **kw)
    np.testing.assert_array_equal(before.attribution, after.attribution)
    np.testing.assert_array_equal(before.error_history, after.error_history)
    np.testing.assert_array_equal(before.attribution_errors, after.attribution_errors)


# ---- 6. not positive definite ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("a, b", [(2, 7), (6, 7), (1, 4)])       # low and high, both high (the wave's pivot), both low
def test_duplicate_column(engine, a, b):
    p = 8
    Xa, Xe, ya, ye = data(p, seed=80)
    Xa[:, b], Xe[:, b] = Xa[:, a], Xe[:, a]
    engine.load_data(Xa, Xe, ya, ye, 0.0)
    v, masks, found, info = engine.subsets_best()
    both = (1 << a) | (1 << b)
    assert info & 1
    assert found[:p].all() and not found[p] and np.isnan(v[p]) and masks[p] == 0
    assert ((masks[:p] & both) != both).all()
    np.testing.assert_array_equal(popcount(masks[:p]), np.arange(p))
    if a >= 6:       # the hook refuses a high subset if ANY of its 64 lanes fails: it can answer for two high copies only
        np.testing.assert_array_equal(v[:p], engine.debug_subset_values(masks[:p].astype(np.uint64)))
    keep = [j for j in range(p) if j != b]              # the truth without the copy: b never wins a tie against a < b
    v7 = B.all_values((Xa[:, keep], Xe[:, keep], ya, ye))
    best7 = B.best_truth(v7, p - 1)[0]
    np.testing.assert_allclose(v[:p], best7, **ORACLE_TOL)
    with pytest.warns(RuntimeWarning, match="not numerically positive definite"):
        res = ls_spa_best_subsets(Xa, Xe, ya, ye)
    assert np.isnan(res.r_squared[p]) and np.isnan(res.theta[p]).all() and res.best_size < p
    assert np.isfinite(res.theta[:p]).all()


# ---- 7. the public call ---------------------------------------------------------------------------------------------------
def test_public_call():
    p, reg = 12, 0.1
    d, v_all = B.brute_case(p, reg)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        res = ls_spa_best_subsets(*d, reg=reg, include=[3, 8])
        full = ls_spa(*d, reg=reg, method="subsets")
    assert isinstance(res, BestSubsetsResults)
    best, masks, found, _ = B.best_truth(v_all, p, B.mask_of((3, 8)))
    assert res.sizes.tolist() == list(range(2, p + 1))
    assert res.subsets.shape == (p - 1, p) and res.theta.shape == (p - 1, p)
    np.testing.assert_allclose(res.r_squared, best[2:], **ORACLE_TOL)
    G, g, H, h, yy = gram_problem(*d, reg=reg)
    for i, k in enumerate(res.sizes):
        assert B.mask_of(np.nonzero(res.subsets[i])[0]) == masks[k]
        cols = np.nonzero(res.subsets[i])[0]
        assert (res.theta[i, ~res.subsets[i]] == 0.0).all()
        np.testing.assert_allclose(res.theta[i, cols], np.linalg.solve(G[np.ix_(cols, cols)], g[cols]), rtol=1e-9,
                                   atol=1e-12)
    assert res.best_size == 2 + int(np.argmax(best[2:]))
    np.testing.assert_array_equal(res.best_subset, res.subsets[res.best_size - 2])
    assert res.full_r_squared == full.r_squared
    assert abs(res.r_squared[-1] - full.r_squared) < 1e-12
    np.testing.assert_allclose(res.theta[-1], full.theta, rtol=1e-9, atol=1e-12)


def test_refusals(engine):
    with pytest.raises(ValueError, match="at most p = 32"):
        ls_spa_best_subsets(*data(33, n=80, m=60, seed=33))
    with pytest.raises(ValueError, match="outside 0 .. 8"):
        ls_spa_best_subsets(*data(9), include=[9])
    with pytest.raises(ValueError, match="twice"):
        ls_spa_best_subsets(*data(9), include=[1, 1])
    engine.load_data(*data(9, seed=1), 0.0)
    with pytest.raises(ValueError, match="include names a feature beyond p"):
        engine.subsets_best(1 << 9)
    engine.load_data(*data(33, n=80, m=60, seed=33), 0.0)
    with pytest.raises(ValueError, match="at most p = 32"):
        engine.subsets_best()
