"""ls_spa_groups on the MI355X: sampled Shapley attribution over groups of columns.  The player map of the engine
(lsspa_set_players: host expansion of group orderings, the existing gather / Cholesky / lift kernels, the fold kernel of
csrc/k_players.hip) against the CPU oracle sample by sample, the mean over all group orderings against the grouped
enumeration, efficiency, and the sampling loop -- statistics, estimators, look-ahead, lanes -- in dimension g."""
import numpy as np
import pytest

import lsspa_oracle as O
from ls_spa import ls_spa, ls_spa_groups
from test_group_sampling_host import expand
from test_groups_host import labels_of, value
from test_subsets_host import data, gram_problem

pytestmark = pytest.mark.gpu

LIFT_TOL = 1e-10        # the stated per-lift tolerance (README, tests/test_gpu_parity.py)
LIFT_TOL_F32 = 1e-4     # fp32 per-ordering work against fp64 (tests/test_gpu_parity.py)


def even_sizes(cols, g):
    """g group sizes that add up to `cols`, as equal as they can be."""
    return [cols // g + (1 if k < cols % g else 0) for k in range(g)]


def oracle_group_lifts(d, reg, labels, group_perms, antithetical):
    """Per sample: the oracle's lifts of the expanded ordering(s), summed by label, averaged over the pair."""
    labels = np.asarray(labels)
    g = int(labels.max()) + 1
    red = O.reduce(*d, reg)
    yy = float(np.asarray(d[3]) @ np.asarray(d[3]))
    out = np.empty((len(group_perms), g))
    for s, o in enumerate(group_perms):
        rows = [expand(labels, o)] + ([expand(labels, o[::-1])] if antithetical else [])
        lifts = [O.ordering_lift(*red, yy, r) for r in rows]
        out[s] = np.mean([[l[labels == k].sum() for k in range(g)] for l in lifts], axis=0)
    return out


# p, rows (n, m), g, baseline, flags, name.  With a baseline an antithetical pair runs as two unpaired orderings, without
# one as the kernels' pair: every kernel path is met both ways.
PARITY = [
    (44, (200, 150), 9, 4, 0, "small_p_registers_baseline"),
    (44, (200, 150), 9, 0, 0, "small_p_registers"),
    (44, (200, 150), 9, 4, 16384, "small_p_lds_baseline"),
    (44, (200, 150), 9, 0, 16384, "small_p_lds"),
    (44, (200, 150), 44, 0, 0, "small_p_singletons"),
    (300, (900, 700), 37, 5, 0, "general_tri_baseline"),
    (300, (900, 700), 37, 0, 0, "general_tri"),
    (150, (500, 100), 12, 6, 0, "general_rect_baseline"),
    (150, (500, 100), 12, 0, 0, "general_rect"),
]


# ---- 4. per-sample parity --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("antithetical", [False, True])
@pytest.mark.parametrize("case", PARITY, ids=[c[-1] for c in PARITY])
def test_group_lifts_against_the_oracle(engine, case, antithetical):
    p, (n, m), g, nb, flags, name = case
    sizes = even_sizes(p - nb, g)
    labels = labels_of(sizes, nb, seed=p + g)
    d = data(p, n=n, m=m, seed=300 + p)
    rng = np.random.default_rng(g)
    perms = np.array([rng.permutation(g) for _ in range(10)], dtype=np.int32)
    want = oracle_group_lifts(d, 0.05, labels, perms, antithetical)
    engine.load_data(*d, 0.05)
    assert engine.tri == (m >= p)
    engine.full_fit()                 # from here on every batch's un-folded lifts are checked against the full R^2
    try:
        engine.set_flags(flags)
        engine.set_players(labels)
        got = engine.run_batch(perms, antithetical, want_lifts=True, accumulate=False)
        again = engine.run_batch(perms, antithetical, want_lifts=True, accumulate=False)
        assert got.shape == (10, g)
        err = np.abs(got - want).max()
        print(f"{name} anti={antithetical} baseline={nb}: max |group lift - oracle| = {err:.2e}")
        assert engine.info() & 12 == 0
        np.testing.assert_allclose(got, want, rtol=0, atol=LIFT_TOL * max(sizes))
        np.testing.assert_array_equal(got, again)
        with pytest.raises(ValueError):
            engine.run_batch(np.zeros((2, g), dtype=np.int32) if g > 1 else np.ones((2, 1), dtype=np.int32), antithetical)
        if flags == 0 and p > 127:
            engine.set_precision("float32")
            try:
                got32 = engine.run_batch(perms, antithetical, want_lifts=True, accumulate=False)
            finally:
                engine.set_precision("float64")
            print(f"{name} fp32: max |fp32 - fp64| = {np.abs(got32 - got).max():.2e}")
            np.testing.assert_allclose(got32, got, rtol=0, atol=LIFT_TOL_F32 * max(sizes))
    finally:
        engine.set_flags(0)
        engine.clear_players()
    # the map is gone: column orderings again, lift vectors of length p
    col = engine.run_batch(np.arange(p, dtype=np.int32)[None, :], False, want_lifts=True, accumulate=False)
    assert col.shape == (1, p)


# ---- 5. all group orderings against the enumeration ----------------------------------------------------------------
@pytest.mark.parametrize("nb", [0, 6])
def test_exact_method_equals_the_enumeration(nb):
    labels = labels_of([4] * 6 if nb else [5] * 6, nb, seed=6)
    assert len(labels) == 30
    d = data(30, n=200, m=150, seed=56)
    got = ls_spa_groups(*d, labels, method="exact")
    ref = ls_spa(*d, method="subsets", groups=labels)
    err = np.abs(got.attribution - ref.attribution).max()
    print(f"g = 6, p = 30, baseline {nb}: max |mean of 720 samples - enumeration| = {err:.2e}")
    np.testing.assert_allclose(got.attribution, ref.attribution, rtol=0, atol=6 * LIFT_TOL)
    assert got.attribution.shape == (6,) and got.theta.shape == (30,)
    np.testing.assert_array_equal(got.theta, ref.theta)
    assert got.r_squared == ref.r_squared


# ---- 6. efficiency ---------------------------------------------------------------------------------------------------
def test_efficiency_g60_p500():
    labels = labels_of([8] * 60, 20, seed=60)
    assert len(labels) == 500
    d = data(500, n=1500, m=1000, seed=65)
    res = ls_spa_groups(*d, labels, method="argsort", max_samples=512, batch_size=128, tolerance=0.0, seed=3)
    base = value(*gram_problem(*d), np.nonzero(labels == -1)[0])
    dev = abs(res.attribution.sum() - (res.r_squared - base))
    print(f"g = 60, p = 500: |sum phi - (R^2 - R^2(B))| = {dev:.2e}")
    assert res.attribution.shape == (60,) and res.attribution_errors.shape == (60,)
    assert dev <= 1e-9


# ---- 7. same orderings, same numbers -------------------------------------------------------------------------------
def test_lookahead_lanes_and_estimators_agree():
    labels = labels_of([5] * 30 + [4] * 10, 10, seed=40)
    assert len(labels) == 200
    d = data(200, n=700, m=500, seed=47)
    kw = dict(method="argsort", seed=7, max_samples=512, batch_size=64, tolerance=0.0)
    one = ls_spa_groups(*d, labels, lookahead=1, lanes=1, **kw)
    same = ls_spa_groups(*d, labels, lookahead=1, lanes=1, **kw)
    np.testing.assert_array_equal(one.attribution, same.attribution)
    np.testing.assert_array_equal(one.error_history, same.error_history)
    np.testing.assert_array_equal(one.attribution_errors, same.attribution_errors)
    for other in (dict(lookahead=4, lanes=1), dict(lookahead=1, lanes=2), dict(lookahead=4, lanes=2)):
        res = ls_spa_groups(*d, labels, **other, **kw)
        print(other, "max |diff| =", np.abs(res.attribution - one.attribution).max())
        np.testing.assert_allclose(res.attribution, one.attribution, rtol=0, atol=1e-13)
        assert len(res.error_history) == len(one.error_history)
    low = ls_spa_groups(*d, labels, error_estimator="lowrank", **kw)
    dev = ls_spa_groups(*d, labels, error_estimator="device", **kw)
    assert len(dev.error_history) == len(low.error_history) == 9       # 64 .. 512, and 511
    np.testing.assert_allclose(dev.attribution, low.attribution, rtol=0, atol=1e-14)
    np.testing.assert_allclose(dev.error_history, low.error_history, rtol=0.15)
    ref = ls_spa_groups(*d, labels, error_estimator="reference", **kw)
    np.testing.assert_allclose(ref.attribution, low.attribution, rtol=0, atol=1e-14)
    assert ref.attribution_errors.shape == (40,) and len(ref.error_history) == 9


# ---- 8. statistics and history in dimension g ------------------------------------------------------------------------
def test_statistics_and_history_have_dimension_g(engine):
    labels = labels_of(even_sizes(190, 23), 10, seed=23)
    d = data(200, n=700, m=500, seed=48)
    engine.load_data(*d, 0.0)
    engine.full_fit()
    try:
        engine.set_players(labels)
        engine.history_enable(64)
        rng = np.random.default_rng(8)
        parts = []
        for B, mode in ((32, 2), (48, 2), (16, True)):
            perms = np.array([rng.permutation(23) for _ in range(B)], dtype=np.int32)
            parts.append(engine.run_batch(perms, True, want_lifts=True, accumulate=mode))
            if mode is True:
                engine.merge()
        lifts = np.concatenate(parts)
        n, mean, cov = engine.stats()
        assert n == 96 and mean.shape == (23,) and cov.shape == (23, 23)
        np.testing.assert_allclose(mean, lifts.mean(axis=0), rtol=0, atol=1e-12)
        np.testing.assert_allclose(cov, np.cov(lifts.T, bias=True), rtol=0, atol=1e-12)
        np.testing.assert_array_equal(engine.history(), lifts)
        assert engine.info() & 12 == 0
    finally:
        engine.history_enable(0)
        engine.clear_players()
    n, mean, _ = engine.stats()
    assert n == 0 and mean.shape == (200,)


# ---- 9. a kept engine is clean ---------------------------------------------------------------------------------------
def test_kept_engine_sampling_unchanged_by_a_grouped_sampling_call():
    d = data(150, n=600, m=400, seed=15)
    kw = dict(method="argsort", seed=7, max_samples=512, batch_size=128, tolerance=0.0)
    before = ls_spa(*d, **kw)
    grouped = ls_spa_groups(*d, labels_of(even_sizes(140, 30), 10, seed=1), **kw)
    assert grouped.attribution.shape == (30,)
    after = ls_spa(*d, **kw)
    np.testing.assert_array_equal(before.attribution, after.attribution)
    np.testing.assert_array_equal(before.error_history, after.error_history)
    np.testing.assert_array_equal(before.attribution_errors, after.attribution_errors)
