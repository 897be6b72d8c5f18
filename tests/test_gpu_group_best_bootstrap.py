"""ls_spa_best_group_subsets_bootstrap on the MI355X (the REPS instantiation of groups_best_kernel in csrc/k_groups.hip,
lsspa_boot_groups_best_run of include/lsspa.h): every replicate against the brute-force truth on the repeated rows
(tests/group_best_boot_ref.py), against the one-problem grouped selection bit for bit -- exact ties, several launches a
replicate and replicates split over launches included --, independence of block, `first` and the form of the weights, a
failed replicate, isolation, and the public call."""
import warnings

import numpy as np
import pytest

import best_ref as B
import group_best_boot_ref as GB
import group_best_ref as GR
from ls_spa import (BestGroupSubsetsBootstrapResults, ls_spa_best_group_subsets_bootstrap, ls_spa_best_subsets,
                    ls_spa_best_subsets_bootstrap)
from ls_spa._engine import HipEngine, debug_boot_groups_best_plan
from ls_spa._native import LSSPANativeError
from test_gpu_best_subsets import ORACLE_TOL
from test_gpu_best_subsets_bootstrap import launch_edges
from test_gpu_bootstrap import one_hot_case
from test_gpu_group_best import planted
from test_group_best_bootstrap_host import BITS_PLANTED, BITS_SPLIT, INDEPENDENCE, split_R
from test_subsets_host import data

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = HipEngine(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def other():
    """A second context for the one-problem selection on a replicate's reduced problem."""
    e = HipEngine(0)
    yield e
    e.close()


def same(a, b):
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


# ---- 1. truth ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, reg", GB.CASES)
def test_every_replicate_against_brute_force(eng, name, reg):
    d, labels, wa, we, u_all = GB.boot_case(name, reg)
    g = int(labels.max()) + 1
    eng.boot_load(*d, reg, grouped=True)
    u, masks, found, r2, base, info = eng.boot_groups_best_run(labels, GB.R, 0, wa.astype(np.float64),
                                                               we.astype(np.float64))
    assert not info.any() and u.shape == (GB.R, g + 1) and masks.dtype == np.uint32
    for r in range(GB.R):
        best, want_masks, want_found, _ = GB.truth(u_all[r], g)
        print("replicate", r, "max |u - truth|", np.nanmax(np.abs(u[r] - best)), "masks", [hex(int(m)) for m in masks[r]])
        np.testing.assert_array_equal(found[r], want_found)
        np.testing.assert_array_equal(masks[r], want_masks)
        np.testing.assert_allclose(u[r], best, **ORACLE_TOL)
        assert abs(r2[r] - u_all[r][-1]) <= ORACLE_TOL["atol"] and abs(base[r] - u_all[r][0]) <= ORACLE_TOL["atol"]
    assert (masks[:, 0] == 0).all() and (masks[:, g] == (1 << g) - 1).all()
    if not (labels < 0).any():
        assert (u[:, 0] == 0.0).all() and (base == 0.0).all()


# ---- 2. same G, same bits ----------------------------------------------------------------------------------------------
def check_bits(eng, other, d, labels, reg, wa, we, replicates, block=0, clean=True):
    """Replicates of a run against lsspa_groups_best on their own reduced problems, bit for bit."""
    p, R = len(labels), len(wa)
    eng.boot_load(*d, reg, grouped=True)
    Sa, Se, W = eng.boot_debug_grams(R, wa, we)
    u, masks, found, r2, base, info = eng.boot_groups_best_run(labels, R, 0, wa, we, block=block)
    for r in replicates:
        G = Sa[r, :p, :p] / W[r] + reg * np.eye(p)
        gv = Sa[r, :p, p] / W[r]
        other.load_reduced(G, gv, Sa[r, p, p] / W[r] + 1.0, Se[r, p, p], H=Se[r, :p, :p], h=Se[r, :p, p])
        want = other.groups_best(labels)
        assert (want[3] & 1) == (info[r] & 1) and (not clean or info[r] == 0)
        same((u[r], masks[r], found[r]), want[:3])
    return u, masks, found, info


def int_weights(seed, R, n, m):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 4, size=(R, n)).astype(np.float64), rng.integers(0, 4, size=(R, m)).astype(np.float64)


@pytest.mark.parametrize("name", GB.NAMES)
def test_a_replicate_has_the_bits_of_the_one_problem_selection(eng, other, name):
    d, labels, wa, we, _ = GB.boot_case(name, 0.1)
    check_bits(eng, other, d, labels, 0.1, wa.astype(np.float64), we.astype(np.float64), range(GB.R))


@pytest.mark.parametrize("run", list(GR.TIE_RUNS))
def test_exact_ties_survive_the_weights_and_go_to_the_smaller_caller_mask(eng, other, run):
    # g = 0 exactly on the columns of a, b, c under any row weights (their rows have y = 0): u = 0.0 in every replicate
    d, labels, _ = GR.tie_case(run)
    wa, we = int_weights(5, 3, d[0].shape[0], d[1].shape[0])
    wa[:, 0], we[:, 0] = np.maximum(wa[:, 0], 1), np.maximum(we[:, 0], 1)
    u, masks, found, _ = check_bits(eng, other, d, labels, 0.0, wa, we, range(3))
    assert found.all() and (u[:, :4] == 0.0).all()
    for r in range(3):
        assert list(masks[r, 1:4]) == GR.tie_winners(run)


def test_several_launches_a_replicate(eng, other):
    name, R, n = BITS_PLANTED
    labels = GR.PLANTED[name][0]
    plan = debug_boot_groups_best_plan(R, n, n, labels)
    assert plan["per"] == 32 and plan["steps"] < plan["per"] and plan["enum_reps"] == 1
    d, _ = planted(labels, 6000)
    assert d[0].shape[0] == n and d[1].shape[0] == n
    rng = np.random.default_rng(20)
    wa, we = rng.integers(1, 4, size=(R, n)).astype(np.float64), rng.integers(1, 4, size=(R, n)).astype(np.float64)
    u, masks, found, _ = check_bits(eng, other, d, labels, 0.0, wa, we, range(R))
    assert found.all() and len({tuple(m) for m in masks}) == R            # two different selections
    # winners from early and late steps of a unit (the low bits of hi = mask >> gl, test_gpu_group_best.py)
    step = (masks.astype(np.int64) >> GR.PLANTED[name][1]["gl"]) & (plan["per"] - 1)
    assert step.min() < plan["steps"] and step.max() >= plan["per"] - plan["steps"]


def test_replicates_split_over_enumeration_launches(eng, other):
    name, n, m = BITS_SPLIT
    d, labels, _ = GR.brute_case(name, 0.0)
    R = split_R()
    plan = debug_boot_groups_best_plan(R, n, m, labels)
    assert d[0].shape[0] == n and d[1].shape[0] == m and plan["n_blocks"] == 1 and 1 < plan["enum_reps"] < R
    wa, we = int_weights(12, R, n, m)
    check_bits(eng, other, d, labels, 0.0, wa, we, launch_edges(plan, R))


# ---- 3. independence ---------------------------------------------------------------------------------------------------
def test_bits_do_not_depend_on_the_run_the_block_or_the_form_of_the_weights(eng):
    name, R = INDEPENDENCE
    seed = 11
    d, labels, _ = GR.brute_case(name, 0.0)
    eng.boot_load(*d, 0.0, grouped=True)
    base = eng.boot_groups_best_run(labels, R, seed)
    assert not base[5].any()
    same(base, eng.boot_groups_best_run(labels, R, seed))
    for block in (1, 2, 0):
        same(base, eng.boot_groups_best_run(labels, R, seed, block=block))
    head = eng.boot_groups_best_run(labels, 2, seed)                         # a run cut into two calls
    tail = eng.boot_groups_best_run(labels, R - 2, seed, first=2)
    same([np.concatenate([a, b]) for a, b in zip(head, tail)], base)
    wa = np.array([eng.boot_debug_counts(seed, r, 0) for r in range(R)], dtype=np.float64)
    we = np.array([eng.boot_debug_counts(seed, r, 1) for r in range(R)], dtype=np.float64)
    same(eng.boot_groups_best_run(labels, R, 999, wa, we), base)
    phi, r2, r2_base, info = eng.boot_groups_run(labels, R, seed)            # the replicates of lsspa_boot_groups_run
    np.testing.assert_array_equal(base[3], r2)
    np.testing.assert_array_equal(base[4], r2_base)
    np.testing.assert_array_equal(base[5], info)
    assert len({tuple(row) for row in base[0]}) == R                         # the replicates do differ


# ---- 4. a bad replicate stays alone --------------------------------------------------------------------------------------
def test_a_failed_replicate_is_flagged_alone_and_keeps_its_candidates(eng, other):
    d, wa, we = one_hot_case()                      # p = 6; replicate 2 never sees column 4 vary
    labels = np.array([0, 0, 1, -1, 2, 2])          # column 4 lies in group 2, the dead group of replicate 2
    g, dead = 3, 1 << 2
    eng.boot_load(*d, 0.0, grouped=True)
    u, masks, found, r2, base, info = eng.boot_groups_best_run(labels, len(wa), 0, wa, we)
    keep = [0, 1, 3, 4]
    assert info[2] & 1 and not info[keep].any()
    ref = eng.boot_groups_best_run(labels, 4, 0, wa[keep], we[keep])
    same((u[keep], masks[keep], found[keep], r2[keep], base[keep]), ref[:5])
    assert found[keep].all() and np.isfinite(base).all() and np.isnan(r2[2])
    # the sets with the dead group drop out: sizes 0 .. g-1 still have candidates, size g (every group) has none
    assert found[2, :g].all() and not found[2, g] and np.isnan(u[2, g]) and masks[2, g] == 0
    assert not (masks[2, :g] & dead).any()
    # ... with the bits of the one-problem selection on replicate 2's reduced problem, which fails the same way
    check_bits(eng, other, d, labels, 0.0, wa, we, [2], clean=False)
    rows = GB.repeated(d, wa[2].astype(int), we[2].astype(int))
    cols = [c for c in range(6) if labels[c] != 2]
    best2 = B.best_truth(GR.all_group_values(tuple(x[:, cols] if x.ndim == 2 else x for x in rows), labels[cols]), g - 1)[0]
    np.testing.assert_allclose(u[2, :g], best2, **ORACLE_TOL)
    with pytest.warns(RuntimeWarning, match="1 of 5 bootstrap replicates"):
        res = ls_spa_best_group_subsets_bootstrap(*d, labels, n_boot=5, weights=(wa, we))
    assert res.n_failed == 1 and np.isnan(res.r_squared_replicates[2]).all()
    assert not res.group_subset_replicates[2].any() and res.best_size_replicates[2] == -1
    np.testing.assert_array_equal(res.r_squared_replicates[keep], u[keep])


# ---- 5. nothing else moves -----------------------------------------------------------------------------------------------
def test_a_run_leaves_the_rest_of_the_context_alone():
    d, labels, _ = GR.brute_case("mixed", 0.0)
    e = HipEngine(0)
    try:
        e.load_data(*d, 0.0)
        e.full_fit()
        e.boot_load(*data(len(labels), n=70, m=50, seed=5), 0.5, grouped=True)
        before = (e.groups_shapley(labels), e.groups_best(labels), e.boot_groups_run(labels, 9, 4), e.info())
        e.boot_groups_best_run(labels, 9, 4)
        e.boot_groups_best_run(labels, 4, 5, block=3)
        after = (e.groups_shapley(labels), e.groups_best(labels), e.boot_groups_run(labels, 9, 4), e.info())
        same(before[0], after[0])
        same(before[1], after[1])
        same(before[2], after[2])
        assert before[3] == after[3]
        e.boot_free()
        same(e.groups_shapley(labels), before[0])
    finally:
        e.close()


# ---- 6. the public call ----------------------------------------------------------------------------------------------------
def test_public_call(eng):
    n_boot, seed = 32, 5
    labels = np.array([0, 0, 1, -1, 2, 2, 2, 3, 1, -1, 4, 4])
    p, g = len(labels), 5
    d = data(p, n=400, m=400, seed=9)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        res = ls_spa_best_group_subsets_bootstrap(*d, labels, n_boot=n_boot, seed=seed)
        point = ls_spa_best_subsets(*d, groups=labels)
    assert isinstance(res, BestGroupSubsetsBootstrapResults) and res.n_failed == 0
    for name in ("sizes", "group_subsets", "subsets", "r_squared", "best_group_subset", "best_subset"):
        np.testing.assert_array_equal(getattr(res, name), getattr(point, name))
    assert res.best_size == point.best_size and res.full_r_squared == point.full_r_squared
    assert res.baseline_r_squared == point.baseline_r_squared
    # against the C-level rows of the same seed
    eng.boot_load(*d, 0.0, grouped=True)
    u, masks, found, r2, base, info = eng.boot_groups_best_run(labels, n_boot, seed)
    assert found.all() and not info.any()
    np.testing.assert_array_equal(res.r_squared_replicates, u)
    np.testing.assert_array_equal(res.group_subset_replicates, ((masks[:, :, None] >> np.arange(g)) & 1).astype(bool))
    np.testing.assert_array_equal(res.full_r_squared_replicates, r2)
    np.testing.assert_array_equal(res.baseline_r_squared_replicates, base)
    np.testing.assert_array_equal(res.group_subset_replicates.sum(axis=2), np.tile(np.arange(g + 1), (n_boot, 1)))
    np.testing.assert_allclose(res.baseline_r_squared_replicates, res.r_squared_replicates[:, 0], rtol=0, atol=1e-12)
    np.testing.assert_allclose(res.r_squared_replicates[:, g], res.full_r_squared_replicates, rtol=0, atol=1e-12)
    # the frequencies, recomputed from group_subset_replicates
    np.testing.assert_array_equal(res.inclusion_frequency, res.group_subset_replicates.mean(axis=0))
    np.testing.assert_array_equal(res.best_size_replicates, np.argmax(res.r_squared_replicates, axis=1))
    chosen = res.group_subset_replicates[np.arange(n_boot), res.best_size_replicates]
    np.testing.assert_array_equal(res.best_inclusion_frequency, chosen.mean(axis=0))
    np.testing.assert_array_equal(res.best_size_frequency, np.bincount(res.best_size_replicates, minlength=g + 1) / n_boot)
    np.testing.assert_array_equal(res.reselected,
                                  (res.group_subset_replicates == point.group_subsets[None]).all(axis=2).mean(axis=0))
    assert res.reselected[0] == res.reselected[g] == 1.0
    # the same call twice has the same bits
    again = ls_spa_best_group_subsets_bootstrap(*d, labels, n_boot=n_boot, seed=seed)
    np.testing.assert_array_equal(again.group_subset_replicates, res.group_subset_replicates)
    np.testing.assert_array_equal(again.r_squared_replicates, res.r_squared_replicates)
    # one side only: the other side's weight is 1 -- the same as handing in ones
    one = ls_spa_best_group_subsets_bootstrap(*d, labels, n_boot=8, seed=seed, resample="train")
    ones = ls_spa_best_group_subsets_bootstrap(*d, labels, n_boot=8, seed=seed, weights=(None, np.ones((8, 400))))
    np.testing.assert_array_equal(one.group_subset_replicates, ones.group_subset_replicates)
    np.testing.assert_array_equal(one.r_squared_replicates, ones.r_squared_replicates)


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------
def test_refusals_leave_a_working_context():
    labels = np.array([0, 0, 1, -1, 2, 2])
    e = HipEngine(0)
    try:
        with pytest.raises(LSSPANativeError, match="lsspa_boot_load comes first"):
            e.boot_groups_best_run(labels, 3, 0)
        d = data(6, n=30, m=20, seed=2)
        e.boot_load(*d, 0.0)                                 # after the ungrouped load too
        good = e.boot_groups_best_run(labels, 3, 1)
        with pytest.raises(ValueError, match="group labels: a group of 0 .. g-1 has no column"):
            e.boot_groups_best_run([0, 0, 0, 2, 2, 2], 3, 1)
        with pytest.raises(ValueError, match="group labels: a label lies outside -1 .. g-1"):
            e.boot_groups_best_run([0, 0, 0, 1, -2, 1], 3, 1)
        with pytest.raises(ValueError, match="length p = 6"):
            e.boot_groups_best_run([0, 1], 3, 1)
        with pytest.raises(ValueError, match="R must be at least 1"):
            e.boot_groups_best_run(labels, 0, 1)
        for bad in (-1.0, np.nan):
            w = np.ones((3, 30))
            w[1, 7] = bad
            with pytest.raises(ValueError, match="finite and >= 0"):
                e.boot_groups_best_run(labels, 3, 1, w, None)
        w = np.ones((3, 20))
        w[2] = 0.0
        with pytest.raises(ValueError, match="replicate 2 sum to 0"):
            e.boot_groups_best_run(labels, 3, 1, None, w)
        same(good, e.boot_groups_best_run(labels, 3, 1))
        e.load_data(*d, 0.0)
        e.full_fit()
        assert e.groups_best(labels)[2].all()
        e.boot_load(*data(40, n=60, m=50, seed=1), 0.0, grouped=True)
        with pytest.raises(ValueError, match="at most g = 32 groups"):
            e.boot_groups_best_run(np.minimum(np.arange(40), 32), 3, 1)
    finally:
        e.close()
    with pytest.raises(ValueError, match="at most p = 64"):
        ls_spa_best_group_subsets_bootstrap(*data(65, n=140, m=100, seed=1), np.arange(65) % 8)
    with pytest.raises(ValueError, match="does not take groups= yet"):
        ls_spa_best_subsets_bootstrap(*data(4, n=30, m=20, seed=2), groups=[0, 0, 1, 1])
    res = ls_spa_best_group_subsets_bootstrap(*data(4, n=30, m=20, seed=2), [0, 0, 1, 1], n_boot=4)     # the kept engine works
    assert res.n_failed == 0
