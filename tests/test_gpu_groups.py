"""ls_spa(method='subsets', groups=labels) on the MI355X: the exact attribution over groups of columns
(csrc/k_groups.hip) against the naive CPU oracle of tests/test_groups_host.py and the five facts that pin it: the
ungrouped enumeration (all singletons), the existing lift kernels over all group orderings, efficiency, relabelling and
the baseline eliminated by a Schur complement."""
import numpy as np
import pytest

from ls_spa import ls_spa
from test_groups_host import (group_orderings, group_shapley, group_values, labels_of, schur_problem, value)
from test_subsets_host import data, gram_problem

pytestmark = pytest.mark.gpu

LIFT_TOL = dict(rtol=0, atol=1e-10)       # the stated per-lift tolerance (tests/test_gpu_parity.py)
ORACLE_TOL = dict(rtol=0, atol=1e-11)     # tests/test_gpu_subsets.py, against its oracle at p = 20

MIXED20 = [1, 2, 3, 4, 4, 3, 2, 1, 4, 4, 3, 3, 2, 4, 4, 1, 4, 4, 3, 4]      # 20 groups, 60 columns
SHAPES = {
    "singletons_p12": ([1] * 12, 0),
    "sizes_1_2_3": ([1, 2, 3], 0),
    "8_groups_of_3": ([3] * 8, 0),
    "12_groups_of_5_and_4_baseline": ([5] * 12, 4),
    "16_groups_of_3": ([3] * 16, 0),
}


def problem(p, seed):
    return data(p, n=4 * p + 8, m=3 * p + 5, seed=seed)


@pytest.mark.parametrize("reg", [0.0, 0.1])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_against_the_cpu_oracle(shape, reg):
    sizes, nb = SHAPES[shape]
    labels = labels_of(sizes, nb, seed=len(sizes))
    d = problem(len(labels), seed=200 + len(labels))
    res = ls_spa(*d, reg=reg, method="subsets", groups=labels)
    want = group_shapley(*gram_problem(*d, reg=reg), labels)
    err = np.abs(res.attribution - want).max()
    print(f"{shape} reg={reg}: max |phi - oracle| = {err:.2e}")
    assert res.attribution.shape == (len(sizes),) and res.theta.shape == (len(labels),)
    np.testing.assert_allclose(res.attribution, want, **ORACLE_TOL)


@pytest.mark.parametrize("reg", [0.0, 0.1])
def test_20_mixed_groups_values_and_efficiency(engine, reg):
    """g = 20, p = 60: the naive oracle of all 2^20 group subsets takes minutes, so the enumeration's own device code is
    compared on seeded masks (the small, the nearly full and 4096 random ones), and phi by its sum."""
    labels = labels_of(MIXED20, 4, seed=20)
    p, ng = len(labels), len(MIXED20)
    assert p == 64
    d = problem(p, seed=264)
    prob = gram_problem(*d, reg=reg)
    engine.load_data(*d, reg)
    full = (1 << ng) - 1
    small = [0] + [1 << i for i in range(ng)]
    masks = np.array(small + [full ^ m for m in small] + list(np.random.default_rng(21).integers(0, 1 << ng, 4096)),
                     dtype=np.uint64)
    got = engine.debug_group_values(labels, masks)
    want = group_values(*prob, labels, masks)
    print(f"g=20 reg={reg}: max |u - oracle| = {np.abs(got - want).max():.2e}")
    np.testing.assert_allclose(got, want, **ORACLE_TOL)
    phi, info = engine.groups_shapley(labels)
    assert info == 0
    assert abs(phi.sum() - (want[len(small)] - want[0])) <= 1e-12        # u(all groups) - u(no group)
    assert abs(want[len(small)] - value(*prob, np.arange(p))) <= 1e-13


@pytest.mark.parametrize("p", [12, 24])
def test_fact1_singletons_equal_the_ungrouped_call(p):
    d = problem(p, seed=300 + p)
    grouped = ls_spa(*d, method="subsets", groups=np.arange(p))
    plain = ls_spa(*d, method="subsets")
    np.testing.assert_allclose(grouped.attribution, plain.attribution, rtol=0, atol=1e-12)
    np.testing.assert_array_equal(grouped.theta, plain.theta)
    assert grouped.r_squared == plain.r_squared


@pytest.mark.parametrize("sizes, nb", [([3, 1, 4, 2], 0), ([2, 5, 1, 3, 4], 2)])
def test_fact2_mean_over_all_group_orderings_of_the_lift_kernels(sizes, nb):
    labels = labels_of(sizes, nb, seed=sum(sizes))
    d = problem(len(labels), seed=400 + len(labels))
    orders = group_orderings(labels)
    mean_lift = ls_spa(*d, perms=orders, antithetical=False, batch_size=24, tolerance=0.0).attribution
    per_group = np.array([mean_lift[labels == k].sum() for k in range(len(sizes))])
    phi = ls_spa(*d, method="subsets", groups=labels).attribution
    np.testing.assert_allclose(phi, per_group, **LIFT_TOL)


@pytest.mark.parametrize("nb", [0, 5])
def test_fact3_efficiency(engine, nb):
    labels = labels_of([4] * 13, nb, seed=13)
    p = len(labels)
    d = problem(p, seed=500 + p)
    res = ls_spa(*d, method="subsets", groups=labels)
    base = value(*gram_problem(*d), np.nonzero(labels == -1)[0])
    assert (base == 0.0) == (nb == 0)
    assert abs(res.attribution.sum() - (res.r_squared - base)) <= 1e-12


def test_fact4_relabelling_at_g20_and_launch_bound(engine):
    """Several units and launches in play: permuting the columns with their labels leaves phi unchanged, renumbering the
    groups permutes it, two calls are bitwise equal -- and, this being the largest case of the suite, no launch of it
    takes more than 0.2 s."""
    labels = labels_of(MIXED20, 4, seed=20)
    p, ng = len(labels), len(MIXED20)
    Xa, Xe, ya, ye = problem(p, seed=264)
    engine.load_data(Xa, Xe, ya, ye, 0.0)
    phi, info = engine.groups_shapley(labels)
    kernels, longest, launches = engine.groups_timing()
    print(f"g = 20, p = 64: kernels {kernels:.3f} s in {launches} launches, longest {longest * 1e3:.1f} ms")
    assert launches > 1 and 0 < longest <= 0.2
    again, _ = engine.groups_shapley(labels)
    np.testing.assert_array_equal(phi, again)
    renum = np.random.default_rng(22).permutation(ng)       # group k becomes group renum[k]
    relab = np.where(labels < 0, -1, renum[np.maximum(labels, 0)])
    got, info_r = engine.groups_shapley(relab)
    np.testing.assert_allclose(got[renum], phi, rtol=0, atol=1e-12)
    perm = np.random.default_rng(23).permutation(p)
    engine.load_data(Xa[:, perm], Xe[:, perm], ya, ye, 0.0)
    phi_p, info_p = engine.groups_shapley(labels[perm])
    assert info == info_r == info_p == 0
    np.testing.assert_allclose(phi_p, phi, rtol=0, atol=1e-12)
    assert np.abs(phi).max() > 1e-3


def test_determinism_through_the_driver():
    labels = labels_of([2, 4, 3, 1, 5, 2, 3, 4, 2, 1], 2, seed=9)
    d = problem(len(labels), seed=29)
    a = ls_spa(*d, method="subsets", groups=labels)
    b = ls_spa(*d, method="subsets", groups=labels)
    np.testing.assert_array_equal(a.attribution, b.attribution)


def test_intercept_and_one_hot_groups():
    """A column of ones in the baseline, categorical variables as one-hot columns with one level dropped, one numeric
    variable: phi against the oracle and against the oracle of the Schur-reduced problem (fact 5)."""
    rng = np.random.default_rng(77)
    levels = [4, 3, 6, 5]

    def design(n):
        cats = [rng.integers(0, L, n) for L in levels]
        cols = [np.ones(n)] + [(c == lv).astype(float) for c, L in zip(cats, levels) for lv in range(1, L)]
        return np.column_stack(cols + [rng.standard_normal(n)])

    labels = np.array([-1] + [k for k, L in enumerate(levels) for _ in range(L - 1)] + [len(levels)])
    Xa, Xe = design(400), design(250)
    w = rng.standard_normal(Xa.shape[1])
    ya, ye = Xa @ w + rng.standard_normal(400), Xe @ w + rng.standard_normal(250)
    res = ls_spa(Xa, Xe, ya, ye, method="subsets", groups=labels)
    prob = gram_problem(Xa, Xe, ya, ye)
    np.testing.assert_allclose(res.attribution, group_shapley(*prob, labels), **ORACLE_TOL)
    np.testing.assert_allclose(res.attribution, group_shapley(*schur_problem(*prob, labels)), **ORACLE_TOL)
    base = value(*prob, [0])
    assert abs(res.attribution.sum() - (res.r_squared - base)) <= 1e-12


def test_fewer_test_rows_than_columns(golden):
    g = golden("edge")                       # p = 12, M = 8: the test factor itself is kept (rect mode)
    d = [g[k] for k in ("X_train", "X_test", "y_train", "y_test")]
    labels = np.array([0, 0, 1, 1, 1, 2, -1, 2, 3, 3, 3, 3])
    res = ls_spa(*d, method="subsets", groups=labels)
    np.testing.assert_allclose(res.attribution, group_shapley(*gram_problem(*d), labels), **ORACLE_TOL)


def test_rect_mode_with_more_than_32_columns():
    labels = labels_of([6] * 6 + [2] * 2, 4, seed=44)       # p = 44, 30 test rows
    d = data(len(labels), n=200, m=30, seed=444)
    res = ls_spa(*d, reg=0.05, method="subsets", groups=labels)
    np.testing.assert_allclose(res.attribution, group_shapley(*gram_problem(*d, reg=0.05), labels), **ORACLE_TOL)


def test_float32_inputs():
    labels = labels_of([2, 3, 1, 4], 1, seed=3)
    d = [a.astype(np.float32) for a in data(len(labels), seed=9)]
    res = ls_spa(*d, method="subsets", groups=labels, precision="float32")
    np.testing.assert_allclose(res.attribution, group_shapley(*gram_problem(*d), labels), **ORACLE_TOL)


def test_kept_engine_float32_then_groups():
    from ls_spa._engine import HipEngine
    labels = labels_of([3, 2, 4, 1, 2], 2, seed=14)
    d = data(len(labels), n=300, m=150, seed=140)
    ls_spa(*d, method="argsort", seed=1, max_samples=256, batch_size=128, tolerance=0.0, precision="float32")
    after = ls_spa(*d, method="subsets", groups=labels)
    fresh_engine = HipEngine(0)
    try:
        fresh = ls_spa(*d, method="subsets", groups=labels, _engine=fresh_engine)
    finally:
        fresh_engine.close()
    np.testing.assert_array_equal(after.theta, fresh.theta)
    assert after.r_squared == fresh.r_squared
    np.testing.assert_array_equal(after.attribution, fresh.attribution)


def test_kept_engine_sampling_unchanged_by_a_groups_call():
    d = data(12, n=200, m=100, seed=12)
    kw = dict(method="argsort", seed=7, max_samples=512, batch_size=128, tolerance=0.0)
    before = ls_spa(*d, **kw)
    ls_spa(*d, method="subsets", groups=np.arange(12) // 3)
    after = ls_spa(*d, **kw)
    np.testing.assert_array_equal(before.attribution, after.attribution)
    np.testing.assert_array_equal(before.error_history, after.error_history)
    np.testing.assert_array_equal(before.attribution_errors, after.attribution_errors)


def test_engine_state_untouched(engine):
    """The running statistics of a sampling batch and the ungrouped enumeration's timing survive a grouped call."""
    d = data(14, n=200, m=100, seed=14)
    engine.load_data(*d, 0.0)
    engine.full_fit()
    plain, _ = engine.subsets_shapley()
    timing = engine.subsets_timing()
    perms = np.array([np.random.default_rng(s).permutation(14) for s in range(16)], dtype=np.int32)
    engine.reset_stats()
    engine.run_batch(perms, False, accumulate=2)
    n0, m0, c0 = engine.stats()
    engine.groups_shapley(np.arange(14) // 2)
    n1, m1, c1 = engine.stats()
    assert n0 == n1 and np.array_equal(m0, m1) and np.array_equal(c0, c1)
    assert engine.subsets_timing() == timing
    np.testing.assert_array_equal(engine.subsets_shapley()[0], plain)


@pytest.mark.parametrize("p, labels, text", [
    (40, np.minimum(np.arange(40), 32), "at most g = 32"),
    (65, np.arange(65) % 8, "at most p = 64"),
    (6, np.array([0, 0, 2, 2, -1, -1]), "no column"),
    (6, np.array([0, 0, 1, 1, -2, -1]), "outside -1"),
    (6, np.full(6, -1), "at least one group"),
])
def test_refused_by_the_library(engine, p, labels, text):
    engine.load_data(*data(p, n=2 * p + 20, m=p + 20, seed=33), 0.0)
    with pytest.raises(ValueError, match=text):
        engine.groups_shapley(labels)
