"""ls_spa_best_subsets_bootstrap on the MI355X (the REPS instantiation of subsets_best_kernel in csrc/k_subsets.hip,
lsspa_boot_best_run of include/lsspa.h): every replicate against the brute-force truth on the repeated rows
(tests/best_boot_ref.py), against the one-problem selection bit for bit, independence of block, `first` and the form of
the weights, a failed replicate, isolation, and the public call."""
import warnings

import numpy as np
import pytest

import best_boot_ref as BB
import best_ref as B
import hp_ref
from ls_spa import BestSubsetsBootstrapResults, ls_spa, ls_spa_best_subsets, ls_spa_best_subsets_bootstrap
from ls_spa._engine import HipEngine, debug_boot_best_plan
from ls_spa._native import LSSPANativeError
from test_best_subsets_bootstrap_host import BITS_BIG
from test_gpu_best_subsets import ORACLE_TOL
from test_gpu_bootstrap import one_hot_case
from test_subsets_host import data

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = HipEngine(0)
    yield e
    e.close()


def same(a, b):
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


# ---- 1. truth ----------------------------------------------------------------------------------------------------------
def check_against_truth(got, v_all, p, include=0):
    v, masks, found, r2, info = got
    assert not info.any()
    for r in range(len(v)):
        best, want_masks, want_found, _ = B.best_truth(v_all[r], p, include)
        print("replicate", r, "max |v - truth|", np.nanmax(np.abs(v[r] - best)), "masks", [hex(int(m)) for m in masks[r]])
        np.testing.assert_array_equal(found[r], want_found)
        np.testing.assert_array_equal(masks[r], want_masks)
        np.testing.assert_allclose(v[r][found[r]], best[found[r]], **ORACLE_TOL)
        assert np.isnan(v[r][~found[r]]).all() and (masks[r][~found[r]] == 0).all()
        assert abs(r2[r] - v_all[r][-1]) <= ORACLE_TOL["atol"]


@pytest.mark.parametrize("p, reg", BB.CASES)
def test_every_replicate_against_brute_force(eng, p, reg):
    d, wa, we, v_all = BB.boot_case(p, reg)
    eng.boot_load(*d, reg)
    got = eng.boot_best_run(BB.R, 0, wa.astype(np.float64), we.astype(np.float64))
    check_against_truth(got, v_all, p)
    assert (got[0][:, 0] == 0.0).all() and (got[1][:, p] == (1 << p) - 1).all()


@pytest.mark.parametrize("which", [0, 1, 2])
@pytest.mark.parametrize("p", B.INCLUDE_P)
def test_include(eng, p, which):
    d, wa, we, v_all = BB.boot_case(p, 0.0)
    cols = B.include_sets(p)[which]
    inc = B.mask_of(cols)
    eng.boot_load(*d, 0.0)
    got = eng.boot_best_run(BB.R, 0, wa.astype(np.float64), we.astype(np.float64), include=inc)
    check_against_truth(got, v_all, p, inc)
    assert not got[2][:, :len(cols)].any() and got[2][:, len(cols):].all()
    assert ((got[1][:, len(cols):] & inc) == inc).all()


# ---- 2. same G, same bits ----------------------------------------------------------------------------------------------
def launch_edges(plan, R):
    """The first and last replicate of every enumeration launch of a run of R replicates."""
    out = set()
    for b0 in range(0, R, plan["block"]):
        nb = min(plan["block"], R - b0)
        for e0 in range(0, nb, plan["enum_reps"]):
            out |= {b0 + e0, b0 + min(e0 + plan["enum_reps"], nb) - 1}
    return sorted(out)


@pytest.mark.parametrize("p, R, block", [(p, 3, 0) for p in B.BRUTE_P] + [(20, 70, 0), BITS_BIG + (0,)])
def test_a_replicate_has_the_bits_of_the_one_problem_selection(eng, p, R, block):
    n, m, reg = 50, 40, 0.25
    d = data(p, n=n, m=m, seed=40 + p)
    rng = np.random.default_rng(p)
    wa, we = rng.integers(0, 4, size=(R, n)).astype(np.float64), rng.integers(0, 4, size=(R, m)).astype(np.float64)
    plan = debug_boot_best_plan(R, n, m, p, block)
    if p == 20:       # several launches (sets of replicates) in the one block
        assert plan["n_blocks"] == 1 and plan["enum_reps"] < R
    edges = launch_edges(plan, R)
    eng.boot_load(*d, reg)
    Sa, Se, W = eng.boot_debug_grams(R, wa, we)
    v, masks, found, r2, info = eng.boot_best_run(R, 0, wa, we, block=block)
    other = HipEngine(0)
    try:
        for r in edges:
            G = Sa[r, :p, :p] / W[r] + reg * np.eye(p)
            g = Sa[r, :p, p] / W[r]
            other.load_reduced(G, g, float(g @ np.linalg.solve(G, g)) * 1.01 + 1.0, Se[r, p, p], H=Se[r, :p, :p],
                               h=Se[r, :p, p])
            want = other.subsets_best()
            assert want[3] == 0 and info[r] == 0
            same((v[r], masks[r], found[r]), want[:3])
    finally:
        other.close()


# ---- 3. independence ---------------------------------------------------------------------------------------------------
def test_bits_do_not_depend_on_the_run_the_block_or_the_form_of_the_weights(eng):
    p, n, m, R, seed = 9, 300, 270, 7, 11
    eng.boot_load(*data(p, n=n, m=m, seed=3), 0.0)
    base = eng.boot_best_run(R, seed)
    assert not base[4].any()
    same(base, eng.boot_best_run(R, seed))
    for block in (0, 1, 3):
        same(base, eng.boot_best_run(R, seed, block=block))
    tail = eng.boot_best_run(R - 2, seed, first=2)                  # a run cut into calls
    same(tail, [a[2:] for a in base])
    wa = np.array([eng.boot_debug_counts(seed, r, 0) for r in range(R)], dtype=np.float64)
    we = np.array([eng.boot_debug_counts(seed, r, 1) for r in range(R)], dtype=np.float64)
    same(eng.boot_best_run(R, 999, wa, we)[:4], base[:4])
    phi, r2, info = eng.boot_run(R, seed)
    np.testing.assert_array_equal(base[3], r2)
    np.testing.assert_array_equal(base[4], info)
    assert len({tuple(row) for row in base[1]}) > 1                 # the replicates do differ


# ---- 4. a bad replicate stays alone --------------------------------------------------------------------------------------
def test_a_failed_replicate_is_flagged_alone_and_keeps_its_candidates(eng):
    d, wa, we = one_hot_case()
    p, j = 6, 4
    eng.boot_load(*d, 0.0)
    v, masks, found, r2, info = eng.boot_best_run(len(wa), 0, wa, we)
    keep = [0, 1, 3, 4]
    assert info[2] & 1 and not info[keep].any()
    ref = eng.boot_best_run(4, 0, wa[keep], we[keep])
    same((v[keep], masks[keep], found[keep], r2[keep]), ref[:4])
    assert found[keep].all()
    # replicate 2 never sees column j vary: the subsets with j drop out, every size below p still has candidates
    assert found[2, :p].all() and not found[2, p] and np.isnan(v[2, p]) and masks[2, p] == 0
    assert not ((masks[2, :p] >> j) & 1).any()
    cols = [c for c in range(p) if c != j]
    rows = BB.repeated(d, wa[2].astype(int), we[2].astype(int))
    best5 = B.best_truth(B.all_values((rows[0][:, cols], rows[1][:, cols], rows[2], rows[3])), p - 1)[0]
    np.testing.assert_allclose(v[2, :p], best5, **ORACLE_TOL)
    with pytest.warns(RuntimeWarning, match="1 of 5 bootstrap replicates"):
        res = ls_spa_best_subsets_bootstrap(*d, n_boot=5, weights=(wa, we))
    assert res.n_failed == 1 and np.isnan(res.r_squared_replicates[2]).all() and not res.subset_replicates[2].any()
    np.testing.assert_array_equal(res.r_squared_replicates[keep], v[keep])


# ---- 5. nothing else moves -----------------------------------------------------------------------------------------------
def test_a_run_leaves_the_rest_of_the_context_alone():
    d = data(8, n=120, m=90, seed=8)
    e = HipEngine(0)
    try:
        kw = dict(method="argsort", seed=3, batch_size=16, max_samples=32, tolerance=0.0, _engine=e)
        before_run = ls_spa(*d, **kw)
        e.boot_load(*hp_ref.gen(5, 33, 21, 1.0, 1), 0.5)
        before = (e.subsets_shapley()[0], e.subsets_best(), e.boot_run(9, 4), e.stats(), e.info())
        e.boot_best_run(9, 4)
        e.boot_best_run(4, 5, include=0b101, block=3)
        after = (e.subsets_shapley()[0], e.subsets_best(), e.boot_run(9, 4), e.stats(), e.info())
        np.testing.assert_array_equal(before[0], after[0])
        same(before[1], after[1])
        same(before[2], after[2])
        assert before[3][0] == after[3][0] and before[4] == after[4]
        np.testing.assert_array_equal(before[3][1], after[3][1])
        np.testing.assert_array_equal(before[3][2], after[3][2])
        e.boot_free()
        np.testing.assert_array_equal(e.subsets_shapley()[0], before[0])
        after_run = ls_spa(*d, **kw)
        np.testing.assert_array_equal(before_run.attribution, after_run.attribution)
        np.testing.assert_array_equal(before_run.error_history, after_run.error_history)
    finally:
        e.close()


# ---- 6. the public call ----------------------------------------------------------------------------------------------------
def test_public_call():
    p, n_boot = 8, 32
    d = data(p, n=400, m=400, seed=9)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        res = ls_spa_best_subsets_bootstrap(*d, n_boot=n_boot, seed=5)
        point = ls_spa_best_subsets(*d)
    assert isinstance(res, BestSubsetsBootstrapResults) and res.n_failed == 0
    for name in ("sizes", "subsets", "r_squared", "best_subset"):
        np.testing.assert_array_equal(getattr(res, name), getattr(point, name))
    assert res.best_size == point.best_size and res.full_r_squared == point.full_r_squared
    assert res.subset_replicates.shape == (n_boot, p + 1, p) and res.r_squared_replicates.shape == (n_boot, p + 1)
    np.testing.assert_array_equal(res.subset_replicates.sum(axis=2), np.tile(np.arange(p + 1), (n_boot, 1)))
    np.testing.assert_array_equal(res.r_squared_replicates[:, 0], np.zeros(n_boot))
    np.testing.assert_allclose(res.r_squared_replicates[:, p], res.full_r_squared_replicates, rtol=0, atol=1e-12)
    # the frequencies, recomputed from subset_replicates
    np.testing.assert_array_equal(res.inclusion_frequency, res.subset_replicates.mean(axis=0))
    np.testing.assert_array_equal(res.best_size_replicates, np.argmax(res.r_squared_replicates, axis=1))
    chosen = res.subset_replicates[np.arange(n_boot), res.best_size_replicates]
    np.testing.assert_array_equal(res.best_inclusion_frequency, chosen.mean(axis=0))
    np.testing.assert_array_equal(res.best_size_frequency, np.bincount(res.best_size_replicates, minlength=p + 1) / n_boot)
    np.testing.assert_array_equal(res.reselected, (res.subset_replicates == point.subsets[None]).all(axis=2).mean(axis=0))
    assert res.reselected[0] == res.reselected[p] == 1.0
    # the same call twice has the same bits
    again = ls_spa_best_subsets_bootstrap(*d, n_boot=n_boot, seed=5)
    np.testing.assert_array_equal(again.subset_replicates, res.subset_replicates)
    np.testing.assert_array_equal(again.r_squared_replicates, res.r_squared_replicates)
    # one side only: the other side's weight is 1 -- the same as handing in ones
    one = ls_spa_best_subsets_bootstrap(*d, n_boot=8, seed=5, resample="train")
    ones = ls_spa_best_subsets_bootstrap(*d, n_boot=8, seed=5, weights=(None, np.ones((8, 400))))
    np.testing.assert_array_equal(one.subset_replicates, ones.subset_replicates)
    np.testing.assert_array_equal(one.r_squared_replicates, ones.r_squared_replicates)
    inc = ls_spa_best_subsets_bootstrap(*d, n_boot=8, seed=5, include=[6])
    assert inc.sizes.tolist() == list(range(1, p + 1)) and inc.subset_replicates[:, :, 6].all()


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------
def test_refusals_leave_a_working_context():
    e = HipEngine(0)
    try:
        with pytest.raises(LSSPANativeError, match="lsspa_boot_load comes first"):
            e.boot_best_run(3, 0)
        e.boot_load(*data(33, n=40, m=40, seed=1), 0.0, grouped=True)
        with pytest.raises(ValueError, match="at most p = 32"):
            e.boot_best_run(3, 0)
        d = data(4, n=30, m=20, seed=2)
        e.boot_load(*d, 0.0)
        good = e.boot_best_run(3, 1)
        with pytest.raises(ValueError, match="include names a feature beyond p"):
            e.boot_best_run(3, 1, include=1 << 4)
        for bad in (-1.0, np.nan):
            w = np.ones((3, 30))
            w[1, 7] = bad
            with pytest.raises(ValueError, match="finite and >= 0"):
                e.boot_best_run(3, 1, w, None)
        w = np.ones((3, 20))
        w[2] = 0.0
        with pytest.raises(ValueError, match="replicate 2 sum to 0"):
            e.boot_best_run(3, 1, None, w)
        same(good, e.boot_best_run(3, 1))
        e.load_data(*d, 0.0)
        e.full_fit()
        assert e.subsets_best()[2].all()
    finally:
        e.close()
    with pytest.raises(ValueError, match="at most p = 32"):
        ls_spa_best_subsets_bootstrap(*data(33, n=40, m=40, seed=1))
    with pytest.raises(ValueError, match="does not take groups= yet"):
        ls_spa_best_subsets_bootstrap(*data(4, n=30, m=20, seed=2), groups=[0, 0, 1, 1])
    res = ls_spa_best_subsets_bootstrap(*data(4, n=30, m=20, seed=2), n_boot=4)      # the kept engine still works
    assert res.n_failed == 0
