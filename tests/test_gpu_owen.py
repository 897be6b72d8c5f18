"""ls_spa_owen on the MI355X: the exact Owen values (csrc/k_groups.hip, the OWEN instantiation of the enumeration
kernel) against the CPU truth of tests/owen_ref.py at every edge of the layout of a refined game -- tests/test_owen_host.py
proves through the library's planner that the shapes reach them --, and by their properties where that truth is too slow."""
import functools

import numpy as np
import pytest

from ls_spa import ls_spa, ls_spa_owen
from owen_ref import BIG_CASE, GPU_CASES, owen_values, owen_values_fast, refined_labels
from test_groups_host import group_shapley, group_values, labels_of, value
from test_subsets_host import data, gram_problem

pytestmark = pytest.mark.gpu

ORACLE_TOL = dict(rtol=0, atol=1e-11)     # tests/test_gpu_groups.py: the same data family, the same subset counts


def problem(p, seed):
    return data(p, n=4 * p + 8, m=3 * p + 5, seed=seed)


@functools.lru_cache(maxsize=None)
def truth(name, reg):
    """(Owen values, group Shapley values) of a case of GPU_CASES, computed once."""
    labels, _ = GPU_CASES[name]
    prob = gram_problem(*problem(len(labels), seed=600 + len(labels)), reg=reg)
    slow = name == "12_groups_of_5_and_4_baseline"       # 12 x 2^16 solves of up to 64 columns: the fast truth
    ow = (owen_values_fast if slow else owen_values)(*prob, labels)
    ow.setflags(write=False)
    return ow, group_shapley(*prob, labels)


@pytest.mark.parametrize("reg", [0.0, 0.1])
@pytest.mark.parametrize("name", list(GPU_CASES))
def test_against_the_cpu_truth(name, reg):
    labels, _ = GPU_CASES[name]
    p, g = len(labels), int(labels.max()) + 1
    d = problem(p, seed=600 + p)
    res = ls_spa_owen(*d, labels, reg=reg)
    want, phi = truth(name, reg)
    print(f"{name} reg={reg}: max |Ow - truth| = {np.abs(res.attribution - want).max():.2e}, "
          f"max |phi - oracle| = {np.abs(res.group_attribution - phi).max():.2e}")
    assert res.attribution.shape == (p,) and res.group_attribution.shape == (g,) and res.theta.shape == (p,)
    np.testing.assert_allclose(res.attribution, want, **ORACLE_TOL)
    np.testing.assert_allclose(res.group_attribution, phi, **ORACLE_TOL)
    assert (res.attribution[labels == -1] == 0.0).all()
    grouped = ls_spa(*d, reg=reg, method="subsets", groups=labels)
    np.testing.assert_array_equal(res.group_attribution, grouped.attribution)
    np.testing.assert_array_equal(res.theta, grouped.theta)
    assert res.r_squared == grouped.r_squared
    prob = gram_problem(*d, reg=reg)
    assert abs(res.baseline_r_squared - value(*prob, np.nonzero(labels == -1)[0])) <= 1e-12
    for k in range(g):
        if (labels == k).sum() == 1:
            assert res.attribution[labels == k][0] == res.group_attribution[k]


@pytest.mark.parametrize("p", [12])
def test_singletons_equal_the_ungrouped_call(p):
    d = problem(p, seed=300 + p)
    np.testing.assert_allclose(ls_spa_owen(*d, np.arange(p)).attribution, ls_spa(*d, method="subsets").attribution,
                               rtol=0, atol=1e-12)


def test_one_group_equals_the_ungrouped_call():
    d = problem(12, seed=312)
    np.testing.assert_allclose(ls_spa_owen(*d, np.zeros(12, dtype=int)).attribution,
                               ls_spa(*d, method="subsets").attribution, **ORACLE_TOL)


@pytest.mark.parametrize("reg", [0.0, 0.1])
def test_14_groups_of_4_and_a_target_of_8_by_properties(engine, reg):
    """p = 64, 22 players for the group of 8 (gh = 16, two launches) and 18 for each of the others: the CPU truth would
    take 2^22 + 14 x 2^18 solves, so the group sums, the total and the enumeration's own subset values on seeded masks."""
    labels = BIG_CASE
    p, g = len(labels), 15
    assert p == 64
    d = problem(p, seed=664)
    res = ls_spa_owen(*d, labels, reg=reg)
    grouped = ls_spa(*d, reg=reg, method="subsets", groups=labels)
    sums = np.array([res.attribution[labels == k].sum() for k in range(g)])
    print(f"reg={reg}: max |group sum - phi| = {np.abs(sums - grouped.attribution).max():.2e}, "
          f"|total - (R^2 - base)| = {abs(res.attribution.sum() - (res.r_squared - res.baseline_r_squared)):.2e}")
    np.testing.assert_allclose(sums, grouped.attribution, **ORACLE_TOL)
    np.testing.assert_array_equal(res.group_attribution, grouped.attribution)
    assert abs(res.attribution.sum() - (res.r_squared - res.baseline_r_squared)) <= 1e-11
    assert res.baseline_r_squared == 0.0 and np.abs(res.attribution).max() > 1e-3
    # the refined game of the group of 8, as the enumeration sees it
    ref, b = refined_labels(labels, 14)
    n = g - 1 + b
    engine.load_data(*d, reg)
    full = (1 << n) - 1
    small = [0] + [1 << i for i in range(n)]
    masks = np.array(small + [full ^ m for m in small] + list(np.random.default_rng(21).integers(0, 1 << n, 2048)),
                     dtype=np.uint64)
    got = engine.debug_group_values(ref, masks)
    want = group_values(*gram_problem(*d, reg=reg), ref, masks)
    print(f"reg={reg}: max |u - oracle| = {np.abs(got - want).max():.2e}")
    np.testing.assert_allclose(got, want, **ORACLE_TOL)
    owen, phi, info = engine.groups_owen(labels)
    kernels, longest, launches = engine.groups_timing()
    print(f"kernels {kernels:.3f} s in {launches} launches, longest {longest * 1e3:.1f} ms")
    # the group game's launch, two for the group of 8, one for each group of 4
    assert info == 0 and launches == 1 + 2 + 14 and 0 < longest <= 0.2
    np.testing.assert_array_equal(owen, res.attribution)
    np.testing.assert_array_equal(phi, res.group_attribution)


def test_renumbering_and_permuting(engine):
    labels = labels_of([3, 1, 6, 2, 4, 1, 5], 2, seed=9)
    p, g = len(labels), 7
    Xa, Xe, ya, ye = problem(p, seed=624)
    engine.load_data(Xa, Xe, ya, ye, 0.0)
    owen, phi, info = engine.groups_owen(labels)
    again, phi2, _ = engine.groups_owen(labels)
    np.testing.assert_array_equal(owen, again)
    np.testing.assert_array_equal(phi, phi2)
    renum = np.random.default_rng(22).permutation(g)        # group k becomes group renum[k]
    relab = np.where(labels < 0, -1, renum[np.maximum(labels, 0)])
    got, got_phi, info_r = engine.groups_owen(relab)
    np.testing.assert_allclose(got, owen, rtol=0, atol=1e-12)
    np.testing.assert_allclose(got_phi[renum], phi, rtol=0, atol=1e-12)
    perm = np.random.default_rng(23).permutation(p)
    engine.load_data(Xa[:, perm], Xe[:, perm], ya, ye, 0.0)
    owen_p, _, info_p = engine.groups_owen(labels[perm])
    assert info == info_r == info_p == 0
    np.testing.assert_allclose(owen_p, owen[perm], rtol=0, atol=1e-12)
    assert np.abs(owen).max() > 1e-3


def test_determinism_through_the_driver():
    labels = labels_of([2, 4, 3, 1, 5, 2, 3, 4, 2, 1], 2, seed=9)
    d = problem(len(labels), seed=29)
    a, b = ls_spa_owen(*d, labels), ls_spa_owen(*d, labels)
    np.testing.assert_array_equal(a.attribution, b.attribution)
    np.testing.assert_array_equal(a.group_attribution, b.group_attribution)


def test_fewer_test_rows_than_columns(golden):
    g = golden("edge")                       # p = 12, M = 8: the test factor itself is kept (rect mode)
    d = [g[k] for k in ("X_train", "X_test", "y_train", "y_test")]
    labels = np.array([0, 0, 1, 1, 1, 2, -1, 2, 3, 3, 3, 3])
    res = ls_spa_owen(*d, labels)
    prob = gram_problem(*d)
    np.testing.assert_allclose(res.attribution, owen_values(*prob, labels), **ORACLE_TOL)
    assert abs(res.baseline_r_squared - value(*prob, [6])) <= 1e-12
    assert abs(res.attribution.sum() - (res.r_squared - res.baseline_r_squared)) <= 1e-11


def test_float32_inputs():
    labels = labels_of([2, 3, 1, 4], 1, seed=3)
    d = [a.astype(np.float32) for a in data(len(labels), seed=9)]
    res = ls_spa_owen(*d, labels)
    np.testing.assert_allclose(res.attribution, owen_values(*gram_problem(*d), labels), **ORACLE_TOL)


def test_kept_engine_float32_then_owen():
    from ls_spa._engine import HipEngine
    labels = labels_of([3, 2, 4, 1, 2], 2, seed=14)
    d = data(len(labels), n=300, m=150, seed=140)
    ls_spa(*d, method="argsort", seed=1, max_samples=256, batch_size=128, tolerance=0.0, precision="float32")
    after = ls_spa_owen(*d, labels)
    fresh_engine = HipEngine(0)
    try:
        fresh = ls_spa_owen(*d, labels, _engine=fresh_engine)
    finally:
        fresh_engine.close()
    np.testing.assert_array_equal(after.theta, fresh.theta)
    assert after.r_squared == fresh.r_squared
    np.testing.assert_array_equal(after.attribution, fresh.attribution)


def test_kept_engine_sampling_unchanged_by_an_owen_call():
    d = data(12, n=200, m=100, seed=12)
    kw = dict(method="argsort", seed=7, max_samples=512, batch_size=128, tolerance=0.0)
    before = ls_spa(*d, **kw)
    ls_spa_owen(*d, np.arange(12) // 3)
    after = ls_spa(*d, **kw)
    np.testing.assert_array_equal(before.attribution, after.attribution)
    np.testing.assert_array_equal(before.error_history, after.error_history)
    np.testing.assert_array_equal(before.attribution_errors, after.attribution_errors)


def test_engine_state_untouched(engine):
    """The running statistics of a sampling batch, the info word, the ungrouped enumeration's timing and result and the
    grouped enumeration's result survive an Owen call."""
    d = data(14, n=200, m=100, seed=14)
    labels = np.arange(14) // 2
    engine.load_data(*d, 0.0)
    engine.full_fit()
    plain, _ = engine.subsets_shapley()
    timing = engine.subsets_timing()
    grouped, _ = engine.groups_shapley(labels)
    perms = np.array([np.random.default_rng(s).permutation(14) for s in range(16)], dtype=np.int32)
    engine.reset_stats()
    engine.run_batch(perms, False, accumulate=2)
    n0, m0, c0 = engine.stats()
    info0 = engine.info()
    _, phi, _ = engine.groups_owen(labels)
    n1, m1, c1 = engine.stats()
    assert n0 == n1 and np.array_equal(m0, m1) and np.array_equal(c0, c1)
    assert engine.info() == info0
    assert engine.subsets_timing() == timing
    np.testing.assert_array_equal(phi, grouped)
    np.testing.assert_array_equal(engine.groups_shapley(labels)[0], grouped)
    np.testing.assert_array_equal(engine.subsets_shapley()[0], plain)


@pytest.mark.parametrize("p, labels, text", [
    (60, np.minimum(np.arange(60), 30), "at most 32 players: group 30 has 30 columns beside 30 other groups"),
    (40, np.minimum(np.arange(40), 32), "at most g = 32"),
    (65, np.arange(65) % 8, "at most p = 64"),
    (6, np.array([0, 0, 2, 2, -1, -1]), "no column"),
    (6, np.array([0, 0, 1, 1, -2, -1]), "outside -1"),
    (6, np.full(6, -1), "at least one group"),
])
def test_refused_by_the_library(engine, p, labels, text):
    engine.load_data(*data(p, n=2 * p + 20, m=p + 20, seed=33), 0.0)
    with pytest.raises(ValueError, match=text):
        engine.groups_owen(labels)


def test_no_problem_loaded():
    from ls_spa._engine import HipEngine
    eng = HipEngine(0)
    try:
        eng.p = 4                            # (the wrapper's own length check passes; the library has nothing loaded)
        with pytest.raises(ValueError, match="no problem loaded"):
            eng.groups_owen(np.array([0, 0, 1, 1]))
    finally:
        eng.close()
