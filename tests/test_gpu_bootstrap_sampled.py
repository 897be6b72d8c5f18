"""ls_spa_bootstrap_sampled on the MI355X (the wide weighted Gram pass, boot_lift_finalize_kernel and
boot_lift_stats_kernel of csrc/k_boot.hip, launch_small_problems of csrc/k_small.hip, lsspa_boot_lift_* of
include/lsspa.h): the Gram pass bit for bit on integer data at every column-block count, the replicate problems against
long-double weighted Grams, every sample's lifts against the long-double truth of tests/boot_sampled_ref.py at the
edges of the ordering kernels' layout, the per-replicate statistics, the bitwise contracts of the header, the exact
bootstrap at small p, efficiency, a failed replicate, isolation, memory and the public call.

Tolerance of the lifts: the project's rule, tol = max(1e-10, 8 e_plain) with e_plain the error of NumPy / LAPACK on the
same case (tests/test_gpu_multi_sampled.py).  No truth case may be flagged NOT_PD: for exactly these data (hp_ref.gen(p,
4 p + 3, 4 p + 1, kappa, 9000 + p), boot_seed 42, replicates 0, 1, 2 and the point problem, the three orderings of
hp_ref.orderings(p, 9000 + p, count=1) and their reverses) the smallest relative pivot of any G or H is, computed in
long double on the CPU, at least 1.9e6 x the threshold 16 p eps: p = 9: 1.2e12 / 1.9e6 (kappa 1e1 / 1e4), 15: 9.0e11 /
5.8e6, 16: 8.7e11 / 7.2e6, 40: 4.0e11 / 3.0e6, 111: 2.0e11 / 2.1e6, 112: 2.0e11 / 2.7e6, 127: 1.9e11 / 2.3e6."""
import functools
import itertools
import warnings

import numpy as np
import pytest

import boot_ref
import boot_sampled_ref as ref
import hp_ref
from ls_spa import ls_spa, ls_spa_bootstrap, ls_spa_bootstrap_sampled
from ls_spa._engine import debug_boot_lift_plan

pytestmark = pytest.mark.gpu

T0, MG = 1e-10, 8
EPS = 2.0 ** -52
SEED = 42                      # boot_seed of the truth cases


# ---- 1. the Gram pass, bit for bit -----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def int_case(c):
    """Small-integer rows: every product and every partial sum is an integer far below 2^53, so any order of addition
    gives the same fp64.  549 = 2 x 256 + 37 training rows, 301 = 256 + 45 test rows: two and three slices with a ragged
    last one, neither a multiple of 4."""
    rng = np.random.default_rng(100 + c)
    p = c - 1
    Xa, Xe = rng.integers(-3, 4, (549, p)).astype(np.float64), rng.integers(-3, 4, (301, p)).astype(np.float64)
    ya, ye = rng.integers(-3, 4, 549).astype(np.float64), rng.integers(1, 4, 301).astype(np.float64)
    return Xa, Xe, ya, ye


def int_truth(X, y, w):
    Z = np.concatenate([X, y[:, None]], axis=1)
    return np.einsum("ri,ij,ik->rjk", w, Z, Z)


@pytest.mark.parametrize("R", [1, 5])
@pytest.mark.parametrize("c", [10, 71, 81, 96, 97, 112, 113, 128])
def test_weighted_grams_are_exact_on_integer_rows(engine, c, R):
    Xa, Xe, ya, ye = int_case(c)
    plan = debug_boot_lift_plan(R, len(Xa), len(Xe), c - 1, c - 1, 2, False)
    assert plan["cb"] == (c + 15) // 16 and plan["gram_form"] == int(plan["cb"] >= 6)
    assert plan["slices_train"] == 3 and plan["slices_test"] == 2
    rng = np.random.default_rng(c + R)
    # counts as the device draws them are small integers; fp64 weights: halves, still exact
    wa = rng.integers(0, 5, (R, len(Xa))).astype(np.float64)
    we = rng.integers(0, 9, (R, len(Xe))).astype(np.float64) / 2
    try:
        engine.boot_lift_load(Xa, Xe, ya, ye, 0.0)
        Sa, Se, ws = engine.boot_lift_debug_grams(R, wa, we)
        Sa1, Se1, ws1 = engine.boot_lift_debug_grams(R)          # a side without weights: ones
    finally:
        engine.boot_lift_free()
    assert np.array_equal(Sa, int_truth(Xa, ya, wa)), f"c={c}: S_train differs from the integer truth"
    assert np.array_equal(Se, int_truth(Xe, ye, we)), f"c={c}: S_test differs from the integer truth"
    assert np.array_equal(ws, wa.sum(axis=1))
    assert np.array_equal(Sa1, int_truth(Xa, ya, np.ones_like(wa))) and np.array_equal(ws1, np.full(R, float(len(Xa))))
    assert np.array_equal(Se1, int_truth(Xe, ye, np.ones_like(we)))
    for S in (Sa, Se):
        assert np.array_equal(S, S.transpose(0, 2, 1)), "S is not exactly symmetric"


@pytest.mark.parametrize("c", [10, 81, 128])
def test_counts_are_the_exact_bootstraps_and_enter_as_the_same_weights(engine, c):
    Xa, Xe, ya, ye = int_case(c)
    try:
        engine.boot_lift_load(Xa, Xe, ya, ye, 0.0)
        for r in (0, 3):
            ca = boot_ref.counts(SEED, r, 0, len(Xa)).astype(np.float64)
            ce = boot_ref.counts(SEED, r, 1, len(Xe)).astype(np.float64)
            by_counts = engine.boot_lift_problem(r, SEED)
            by_weights = engine.boot_lift_problem(r, 0, ca, ce)
            for a, b in zip(by_counts, by_weights):
                assert np.array_equal(a, b), f"c={c} r={r}: the uint32 counts and the same fp64 weights differ"
            # H = S_test[:p, :p] is an integer matrix: exact
            assert np.array_equal(by_counts[2], int_truth(Xe, ye, ce[None])[0][:c - 1, :c - 1])
    finally:
        engine.boot_lift_free()


# ---- 2. the replicate problems ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(p, kappa):
    """(data, orderings); computed once and left unchanged."""
    n = 4 * p + 3
    data = hp_ref.gen(p, n, n - 2, kappa, 9000 + p)
    orders = hp_ref.orderings(p, 9000 + p, count=1)            # identity, reversed, one seeded
    for a in data + (orders,):
        a.setflags(write=False)
    return data, orders


@pytest.mark.parametrize("p", [9, 40, 100, 127])
def test_replicate_problems_against_long_double_weighted_grams(engine, p):
    data, _ = case(p, 1e1)
    n, m = len(data[0]), len(data[1])
    try:
        engine.boot_lift_load(*data, 0.25)
        for r in (-1, 0, 2):
            wa = np.ones(n) if r < 0 else boot_ref.counts(SEED, r, 0, n).astype(np.float64)
            we = np.ones(m) if r < 0 else boot_ref.counts(SEED, r, 1, m).astype(np.float64)
            got = engine.boot_lift_problem(r, SEED)
            want = ref.weighted_problem(data, wa, we, 0.25)
            # a sum of n terms carries at most n + 1 roundings on any path (products, additions in any tree, the
            # division by W, reg), and sum_i w |z_a z_b| <= the largest diagonal entry (Cauchy-Schwarz)
            for name, a, b, rows in zip("GgHh", got[:4], want[:4], (n, n, m, m)):
                scale = max(np.abs(np.diag(want[0 if name in "Gg" else 2])).max(), np.abs(b).max())
                err, tol = np.abs(a - b).max(), 2 * (rows + 4) * EPS * scale
                print(f"BOOTLIFT problem p={p} r={r} {name}: err {err:.3e} tol {tol:.3e}")
                assert err <= tol, f"p={p} r={r} {name}: {err:.3e} > {tol:.3e}"
            assert abs(got[4] - want[4]) <= 2 * (m + 4) * EPS * want[4]
    finally:
        engine.boot_lift_free()


# ---- 3. lifts against the truth --------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def truth(p, kappa, anti):
    """(lifts [4][3][p] of replicates 0, 1, 2 and the point problem, e_plain)"""
    data, orders = case(p, kappa)
    want, plain = [], []
    for r in (0, 1, 2, -1):
        want.append(ref.truth_lifts(ref.problem(data, SEED, r), orders, anti))
        plain.append(ref.plain_lifts(data, SEED, r, 0.0, orders, anti))
    want, plain = np.array(want), np.array(plain)
    e_plain = float(np.nanmax(np.abs(plain - want)))
    want.setflags(write=False)
    return want, (e_plain if np.isfinite(e_plain) else 0.0)


def judge(name, got, want, e_plain):
    assert np.all(np.isfinite(got)), f"{name}: non-finite result"
    err, tol = float(np.abs(got - want).max()), max(T0, MG * e_plain)
    print(f"BOOTLIFT {name}: err {err:.3e} e_plain {e_plain:.3e} tol {tol:.3e}")
    assert err <= tol, f"{name}: |got - truth| = {err:.3e} > {tol:.3e} (e_plain {e_plain:.3e})"


# 15: p + 1 fills one block; 16: the augmented row opens a block; 111: the last register-resident shape; 112: the first
# LDS shape; 127: the limit (tests/test_gpu_cv_sampled.py)
@pytest.mark.parametrize("kappa", [1e1, 1e4])
@pytest.mark.parametrize("p", [9, 15, 16, 40, 111, 112, 127])
def test_every_samples_lifts_against_the_long_double_truth(engine, p, kappa):
    data, orders = case(p, kappa)
    try:
        engine.boot_lift_load(*data, 0.0)
        for anti in (False, True):
            engine.boot_lift_set_orderings(orders, anti)
            mean, m2, r2, base, info, samples = engine.boot_lift_run(3, SEED, want_samples=True)
            pm, pm2, pr2, pbase, pinfo, psamples = engine.boot_lift_point(want_samples=True)
            assert samples.shape == (3, len(orders), p) and psamples.shape == (len(orders), p)
            assert not info.any() and not pinfo, f"p={p} kappa={kappa:g}: flagged {info} {pinfo} (no case here may be)"
            want, e_plain = truth(p, kappa, anti)
            judge(f"replicates p={p} kappa={kappa:g} anti={int(anti)}", samples, want[:3], e_plain)
            judge(f"point p={p} kappa={kappa:g} anti={int(anti)}", psamples, want[3], e_plain)
            assert np.all(base == 0.0) and pbase == 0.0
            # the mean of three samples is within round-off of theirs
            assert np.abs(mean - samples.mean(axis=1)).max() <= 8 * EPS * np.abs(samples).max()
    finally:
        engine.boot_lift_free()


# ---- 4. statistics ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("anti, n_samples", [(False, 2 * 256 + 5), (True, 128 + 37)])
def test_per_replicate_statistics_against_numpy(engine, anti, n_samples):
    """mean and M2 of every replicate against the long-double two-pass values of the device's own samples.  Bound, in the
    manner of tests/hp_stats.py (u = 2^-53 times the roundings on the path times the magnitudes summed): a Welford step
    has three roundings and the Chan merge five, so the mean is within 3 (n + merges) u max|x|, and M2 = sum d^2 within
    (3 n + 8 merges) u sum d^2 + 2 E_mean sum |d| (the shift of the mean the deviations are taken about)."""
    p, R = 9, 4
    data, _ = case(p, 1e1)
    rng = np.random.default_rng(5)
    perms = np.array([rng.permutation(p) for _ in range(n_samples)], dtype=np.int32)
    plan = debug_boot_lift_plan(R, len(data[0]), len(data[1]), p, p, n_samples, anti)
    cut = plan["samples_per_launch"]
    assert n_samples % cut != 0 and plan["sample_cuts"] == -(-n_samples // cut)
    if not anti:
        assert plan["sample_cuts"] >= 3
    try:
        engine.boot_lift_load(*data, 0.0)
        engine.boot_lift_set_orderings(perms, anti)
        mean, m2, r2, base, info, samples = engine.boot_lift_run(R, SEED, want_samples=True)
    finally:
        engine.boot_lift_free()
    assert not info.any()
    u, merges = 2.0 ** -53, plan["sample_cuts"]
    for r in range(R):
        x = samples[r].astype(np.longdouble)
        mu = x.mean(axis=0)
        dev = x - mu
        e_mean = 3 * (n_samples + merges) * u * np.abs(samples[r]).max() * (1 + 2.0 ** -10)
        e_m2 = ((3 * n_samples + 8 * merges) * u * (dev * dev).sum(axis=0) + 2 * e_mean * np.abs(dev).sum(axis=0)) \
            * (1 + 2.0 ** -10)
        assert np.all(np.abs(mean[r] - mu) <= e_mean), f"replicate {r}: mean off by {np.abs(mean[r] - mu).max():.3e}"
        got = np.abs(m2[r] - (dev * dev).sum(axis=0))
        assert np.all(got <= e_m2), f"replicate {r}: M2 off by {float((got / e_m2).max()):.3g} x the bound"
        # and the documented merge order in fp64 (the device may fuse a product and an addition)
        wm, wq = ref.welford(samples[r], cut)
        assert np.abs(mean[r] - wm).max() <= e_mean and np.all(np.abs(m2[r] - wq) <= e_m2)


# ---- 5. bitwise ------------------------------------------------------------------------------------------------------------
def test_bitwise_contracts(engine):
    p = 112                      # the LDS-resident form: the fewest replicates a lift launch
    data, _ = case(p, 1e1)
    n, m = len(data[0]), len(data[1])
    R = 37
    rng = np.random.default_rng(11)
    orders = np.array([rng.permutation(p) for _ in range(128 + 3)], dtype=np.int32)     # two sample cuts, the last ragged
    plan = debug_boot_lift_plan(R, n, m, p, p, len(orders), True)
    assert plan["sample_cuts"] == 2
    assert plan["reps_per_launch"] < R <= plan["block"], "the run must cross the replicates-per-launch boundary"
    try:
        engine.boot_lift_load(*data, 0.0)
        engine.boot_lift_set_orderings(orders, True)
        a = engine.boot_lift_run(R, SEED, want_samples=True)
        b = engine.boot_lift_run(R, SEED, want_samples=True)
        for x, y in zip(a, b):
            assert np.array_equal(x, y), "two calls differ"
        alone = engine.boot_lift_run(1, SEED, first=5, want_samples=True)
        by_one = engine.boot_lift_run(R, SEED, block=1, want_samples=True)
        tail = engine.boot_lift_run(R - plan["reps_per_launch"] + 1, SEED, first=plan["reps_per_launch"] - 1)
        for k, (x, y, z) in enumerate(zip(a, alone, by_one)):
            assert np.array_equal(x[5], y[0]), f"output {k}: replicate 5 alone differs from its row in a run of {R}"
            assert np.array_equal(x, z), f"output {k}: block=1 differs"
        for x, y in zip(a[:5], tail):
            assert np.array_equal(x[plan["reps_per_launch"] - 1:], y), "a run starting elsewhere differs"
        assert not a[4].any()
    finally:
        engine.boot_lift_free()


# ---- 6. against the exact bootstrap ----------------------------------------------------------------------------------------
def test_all_orderings_give_the_exact_bootstrap_and_the_exact_point_estimate():
    p = 5
    data = hp_ref.gen(p, 60, 50, 1e1, 5)
    perms = np.array(list(itertools.permutations(range(p))), dtype=np.int32)
    res = ls_spa_bootstrap_sampled(*data, n_boot=20, perms=perms, antithetical=False, boot_seed=7)
    exact = ls_spa_bootstrap(*data, n_boot=20, seed=7)
    point = ls_spa(*data, method="subsets")
    assert res.n_samples == 120 and res.n_failed == 0
    assert np.abs(res.replicates - exact.replicates).max() <= 1e-11
    assert np.abs(res.r_squared_replicates - exact.r_squared_replicates).max() <= 1e-11
    assert np.abs(res.attribution - point.attribution).max() <= 1e-11
    assert abs(res.r_squared - point.r_squared) <= 1e-11 and np.abs(res.theta - point.theta).max() <= 1e-9
    assert np.abs(res.std_error - exact.std_error).max() <= 1e-11 and np.abs(res.lower - exact.lower).max() <= 1e-11


def test_all_group_orderings_give_the_exact_bootstrap_over_groups():
    p, g = 12, 4
    data = hp_ref.gen(p, 90, 70, 1e1, 12)
    labels = np.array([-1, 0, 1, 2, 3, 0, 1, 2, 3, -1, 0, 1])
    perms = np.array(list(itertools.permutations(range(g))), dtype=np.int32)
    res = ls_spa_bootstrap_sampled(*data, n_boot=20, perms=perms, antithetical=False, boot_seed=7, groups=labels)
    exact = ls_spa_bootstrap(*data, n_boot=20, seed=7, groups=labels)
    assert res.replicates.shape == (20, g) and res.n_samples == 24
    assert np.abs(res.replicates - exact.replicates).max() <= 1e-11
    assert np.abs(res.baseline_r_squared_replicates - exact.baseline_r_squared_replicates).max() <= 1e-11
    assert np.abs(res.attribution - exact.attribution).max() <= 1e-11


# ---- 7. efficiency ---------------------------------------------------------------------------------------------------------
def test_every_sample_and_every_replicate_sums_to_its_r_squared_over_groups(engine):
    p, g = 100, 12
    data, _ = case(p, 1e1)
    labels = (np.arange(p) % (g + 1) - 1).astype(np.int32)      # -1: a baseline of eight columns
    rng = np.random.default_rng(3)
    perms = np.array([rng.permutation(g) for _ in range(4)], dtype=np.int32)
    try:
        engine.boot_lift_load(*data, 0.0)
        engine.boot_lift_set_players(labels)
        engine.boot_lift_set_orderings(perms, True)
        mean, m2, r2, base, info, samples = engine.boot_lift_run(3, SEED, want_samples=True)
    finally:
        engine.boot_lift_free()
    assert not info.any() and samples.shape == (3, 4, g) and np.all(base > 0)
    assert np.abs(samples.sum(axis=2) - (r2 - base)[:, None]).max() <= 1e-9
    assert np.abs(mean.sum(axis=1) - (r2 - base)).max() <= 1e-9


# ---- 8. a failed replicate -------------------------------------------------------------------------------------------------
def test_a_replicate_without_enough_rows_is_nan_counted_and_warned_about(engine):
    p, R = 9, 6
    data, orders = case(p, 1e1)
    n = len(data[0])
    good = np.array([boot_ref.counts(SEED, r, 0, n) for r in range(R)], dtype=np.float64)
    bad = good.copy()
    bad[2] = 0.0
    bad[2, :p - 1] = 1.0         # p - 1 rows: a Gram matrix of rank p - 1
    try:
        engine.boot_lift_load(*data, 0.0)
        engine.boot_lift_set_orderings(orders, True)
        info = engine.boot_lift_run(R, SEED, bad)[4]
    finally:
        engine.boot_lift_free()
    assert list(info & 1) == [0, 0, 1, 0, 0, 0]
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        res = ls_spa_bootstrap_sampled(*data, n_boot=R, perms=orders, weights=(bad, None), boot_seed=SEED)
    assert [w.category for w in caught] == [RuntimeWarning], [str(w.message) for w in caught]
    ok = ls_spa_bootstrap_sampled(*data, n_boot=R, perms=orders, weights=(good, None), boot_seed=SEED)
    assert res.n_failed == 1 and ok.n_failed == 0
    assert np.isnan(res.replicates[2]).all() and np.isnan(res.r_squared_replicates[2])
    keep = [0, 1, 3, 4, 5]
    assert np.array_equal(res.replicates[keep], ok.replicates[keep])
    assert np.array_equal(res.replicate_errors[keep], ok.replicate_errors[keep])


# ---- 9. isolation and memory -----------------------------------------------------------------------------------------------
def test_the_other_stores_are_left_alone(engine):
    p = 12
    one = hp_ref.gen(p, 60, 40, 1e1, 12)
    o1 = hp_ref.orderings(p, 12)
    engine.load_data(*one, 0.0)
    engine.full_fit()
    before = engine.run_batch(o1, True, want_lifts=True, accumulate=True)
    stats_before, info_before, gram_before = engine.stats(), engine.info(), engine.gram()
    engine.boot_load(*one, 0.0)
    boot_before = engine.boot_run(4, 3)
    Xc, _, yc, _ = hp_ref.gen(16, 61, 1, 1e1, 6)
    idc = (np.arange(61) % 3).astype(np.int32)
    engine.cv_lift_load(Xc, yc, idc, 3, 0.0)
    cvo = hp_ref.orderings(16, 6)
    cv_before = engine.cv_lift_batch(cvo, True, want_lifts=True, accumulate=True)
    cv_state = engine.cv_lift_get()
    data, orders = case(16, 1e1)
    try:
        engine.boot_lift_load(*data, 0.0)
        engine.boot_lift_set_orderings(orders, True)
        out = engine.boot_lift_run(5, SEED)
        assert not out[4].any()
    finally:
        engine.boot_lift_free()
    assert engine.info() == info_before
    for a, b in zip(engine.stats(), stats_before):
        np.testing.assert_array_equal(a, b)
    for a, b in zip(engine.gram(), gram_before):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(engine.run_batch(o1, True, want_lifts=True, accumulate=False), before)
    for a, b in zip(engine.boot_run(4, 3), boot_before):
        np.testing.assert_array_equal(a, b)
    engine.boot_free()
    for a, b in zip(engine.cv_lift_get(), cv_state):
        np.testing.assert_array_equal(a, b)
    for a, b in zip(engine.cv_lift_batch(cvo, True, want_lifts=True, accumulate=False), cv_before):
        np.testing.assert_array_equal(a, b)
    engine.cv_lift_free()


def test_repeated_load_and_free_leaves_free_memory_where_it_was(engine):
    import torch
    data, orders = case(16, 1e1)

    def cycle():
        engine.boot_lift_load(*data, 0.0)
        engine.boot_lift_set_players((np.arange(16) % 4).astype(np.int32))
        engine.boot_lift_set_orderings(np.array([[0, 1, 2, 3], [3, 1, 0, 2]], dtype=np.int32), True)
        engine.boot_lift_run(3, SEED, want_samples=True)
        engine.boot_lift_point()
        engine.boot_lift_free()

    cycle()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(3):
        cycle()
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    assert free1 == free0, (free0, free1)
    assert getattr(engine, "_boot_lift_dims", None) is None


def test_errors_of_the_engine(engine):
    from ls_spa._native import LSSPANativeError
    data, orders = case(9, 1e1)
    with pytest.raises(LSSPANativeError, match="lsspa_boot_lift_load comes first"):
        engine.boot_lift_set_orderings(orders, True)
    try:
        engine.boot_lift_load(*data, 0.0)
        with pytest.raises(LSSPANativeError, match="lsspa_boot_lift_set_orderings comes first"):
            engine.boot_lift_run(2, SEED)
        bad = orders.copy()
        bad[1, 0] = bad[1, 1]
        with pytest.raises(ValueError, match="not a permutation"):
            engine.boot_lift_set_orderings(bad, True)
        engine.boot_lift_set_orderings(orders, True)
        engine.boot_lift_set_players((np.arange(9) % 3).astype(np.int32))
        with pytest.raises(LSSPANativeError, match="lsspa_boot_lift_set_orderings comes first"):
            engine.boot_lift_point()          # the orderings were the columns'
    finally:
        engine.boot_lift_free()
    wide = hp_ref.gen(128, 140, 140, 1e1, 1)
    with pytest.raises(ValueError, match="at most p = 127"):
        engine.boot_lift_load(*wide, 0.0)


# ---- 10. the public call ---------------------------------------------------------------------------------------------------
def test_public_call_end_to_end():
    p = 40
    data, _ = case(p, 1e1)
    res = ls_spa_bootstrap_sampled(*data, n_boot=16, n_samples=64, confidence=0.8)
    again = ls_spa_bootstrap_sampled(*data, n_boot=16, n_samples=64, confidence=0.8)
    assert res.replicates.shape == (16, p) and res.replicate_errors.shape == (16, p)
    assert res.attribution.shape == (p,) and res.attribution_errors.shape == (p,) and res.theta.shape == (p,)
    assert res.n_samples == 64 and res.n_failed == 0 and res.confidence == 0.8
    assert np.all(res.lower <= res.upper) and np.all(res.std_error > 0) and np.all(res.attribution_errors > 0)
    assert np.all(res.lower <= np.median(res.replicates, axis=0)) and np.all(np.median(res.replicates, axis=0) <= res.upper)
    alpha = (1.0 - 0.8) / 2.0
    assert np.array_equal(res.lower, np.quantile(res.replicates, alpha, axis=0))
    assert np.array_equal(res.upper, np.quantile(res.replicates, 1.0 - alpha, axis=0))
    assert res.prob_greater.shape == (p, p) and np.all(np.diag(res.prob_greater) == 0.0)
    assert res.r_squared_interval[0] <= res.r_squared_interval[1]
    assert abs(res.attribution.sum() - res.r_squared) <= 1e-9
    assert np.abs(res.replicates.sum(axis=1) - res.r_squared_replicates).max() <= 1e-9
    assert np.array_equal(res.replicates, again.replicates) and np.array_equal(res.attribution, again.attribution)
    # the orderings are shared: a replicate's Monte-Carlo error is of the size of the point estimate's
    assert np.nanmax(res.replicate_errors) <= 10 * res.attribution_errors.max()
    fixed = ls_spa_bootstrap_sampled(*data, n_boot=4, n_samples=8, resample="train")
    assert np.ptp(fixed.r_squared_replicates) > 0 and fixed.replicates.shape == (4, p)
