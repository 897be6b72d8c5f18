"""ls_spa_bootstrap(groups=) on the MI355X (the cb = 4, 5 instantiations of csrc/k_boot.hip, the replicate dimension of
csrc/k_groups.hip, lsspa_boot_groups_* of include/lsspa.h): the weighted Gram sums of up to 65 columns against an integer
truth bit for bit, a replicate against the one-problem grouped enumeration bit for bit and against the long-double
truth of tests/hp_ref.py on the repeated rows, reproducibility, isolation of a failed replicate, refusals, and the
public call."""
import numpy as np
import pytest

import gram_cases
import hp_ref
from ls_spa import ls_spa, ls_spa_bootstrap
from ls_spa._engine import HipEngine, debug_boot_groups_plan
from ls_spa._native import LSSPANativeError
from test_gpu_accuracy import judge, threshold
from test_groups_host import group_shapley, labels_of
from test_subsets_host import data, gram_problem

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = HipEngine(0)
    yield e
    e.close()


# ---- 1. exact sums ---------------------------------------------------------------------------------------------------
RPW = {33: 2, 47: 2, 48: 1, 63: 1, 64: 1}       # replicates a wave: c = p + 1 <= 48 is three column blocks, then 4 and 5
CB = {33: 3, 47: 3, 48: 4, 63: 4, 64: 5}
N_AXIS = (3, 4, 5, 65, 513)                      # four-row steps and their tails; 513: three slices, the last of one row


def r_axis(p):
    """A workgroup carries 4 rpw replicates: one short of it, full, one into the next, and one more workgroup."""
    w = 4 * RPW[p]
    return (w - 1, w, w + 1, 2 * w + 1)


def _sum_cases():
    out = [(p, R, 65) for p in RPW for R in r_axis(p)]
    out += [(p, 4 * RPW[p] + 1, n) for p in RPW for n in N_AXIS]
    out += [(p, 2 * 4 * RPW[p] + 1, 513) for p in RPW]
    return sorted(set(out))


def one_group(p):
    return np.zeros(p, dtype=np.int32)


def test_the_plan_is_what_the_cases_were_chosen_for():
    for p in RPW:
        plan = debug_boot_groups_plan(9, 513, 5, one_group(p))
        assert (plan["cb"], plan["rpw"], plan["pairs"]) == (CB[p], RPW[p], CB[p] * (CB[p] + 1) // 2)
        assert (plan["slices_train"], plan["rps_train"], plan["slices_test"]) == (3, 256, 1)
        assert debug_boot_groups_plan(9, 65, 5, one_group(p))["slices_train"] == 1


def int_weights(rng, R, n):
    """Integers 0 .. 7, about a sixth of the rows zero in every replicate, row 0 never (a positive sum at n = 1)."""
    w = rng.integers(0, 8, size=(R, n))
    w[:, rng.random(n) < 1 / 6] = 0
    w[:, 0] = np.maximum(w[:, 0], 1)
    return w


@pytest.mark.parametrize("p,R,n", _sum_cases())
def test_weighted_sums_are_exact(eng, p, R, n):
    """|z| <= 2^15, w <= 7, n <= 513: every partial sum is an integer below 2^46 < 2^53, so any correct fp64 evaluation
    has the int64 truth's bits."""
    m = max(1, (n * 3) // 4)
    rng = np.random.default_rng(1000 * p + 10 * R + n)
    Xa, ya = gram_cases.integer_data(gram_cases.seed_of(f"gboot_tr_{p}_{n}"), n, p, "float64")
    Xe, ye = gram_cases.integer_data(gram_cases.seed_of(f"gboot_te_{p}_{m}"), m, p, "float64")
    wa, we = int_weights(rng, R, n), int_weights(rng, R, m)
    eng.boot_load(Xa, Xe, ya, ye, 0.0, grouped=True)
    Sa, Se, ws = eng.boot_debug_grams(R, wa.astype(np.float64), we.astype(np.float64))
    for S, X, y, w in ((Sa, Xa, ya, wa), (Se, Xe, ye, we)):
        Z = np.concatenate([X, y[:, None]], axis=1).astype(np.int64)
        want = np.einsum("ri,ia,ib->rab", w.astype(np.int64), Z, Z)
        assert np.abs(want).max() < 2 ** 53
        np.testing.assert_array_equal(S, want.astype(np.float64))
    np.testing.assert_array_equal(ws, wa.sum(axis=1).astype(np.float64))


# ---- 2. same G, same bits --------------------------------------------------------------------------------------------
LAYOUTS = {
    "all_low_p6_g3": labels_of([2, 2, 2]),
    "mixed_baseline_p12_g5": labels_of([1, 2, 2, 3, 2], 2, seed=5),
    "p40_g8": labels_of([5] * 8, 0, seed=8),
    "p64_g6_wide_group": labels_of([20, 12, 10, 10, 8, 4], 0, seed=6),
    # more than 8192 high subsets, so a unit owns several: 2^14 in one launch a unit (two steps), and 2^18 in six launches
    # of six steps -- the one-problem call's own cut (tests/test_group_bootstrap_host.py pins both plans)
    "p20_g20_two_steps": labels_of([1] * 20),
    "p64_g20_six_launches": labels_of([4] * 4 + [3] * 16, 0, seed=20),
}


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_a_replicate_has_the_bits_of_the_one_problem_enumeration(eng, name):
    labels = LAYOUTS[name]
    p, n, m, R, reg = len(labels), 80, 70, 3, 0.25
    d = data(p, n=n, m=m, seed=40 + p)
    rng = np.random.default_rng(p)
    wa, we = rng.integers(0, 4, size=(R, n)).astype(np.float64), rng.integers(0, 4, size=(R, m)).astype(np.float64)
    eng.boot_load(*d, reg, grouped=True)
    Sa, Se, W = eng.boot_debug_grams(R, wa, we)
    phi, r2, base, info = eng.boot_groups_run(labels, R, 0, wa, we)
    other = HipEngine(0)
    try:
        for r in range(R):
            G = Sa[r, :p, :p] / W[r] + reg * np.eye(p)
            g = Sa[r, :p, p] / W[r]
            other.load_reduced(G, g, float(g @ np.linalg.solve(G, g)) * 1.01 + 1.0, Se[r, p, p], H=Se[r, :p, :p],
                               h=Se[r, :p, p])
            want, bits = other.groups_shapley(labels)
            assert bits == 0 and info[r] == 0
            np.testing.assert_array_equal(phi[r], want)
    finally:
        other.close()


# ---- 3. truth --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("labels,checked", [(labels_of([2, 3, 1, 4, 2], 2, seed=3), (0, 1, 2)),
                                            (labels_of([5] * 8, 0, seed=8), (1,)),
                                            (labels_of([7, 7, 8, 8, 6, 6, 4], 4, seed=7), (1,))])
def test_a_replicate_is_the_grouped_attribution_of_the_repeated_rows(eng, labels, checked):
    """Judged as the one-problem grouped enumeration is in tests/test_gpu_accuracy.py: against the long-double group
    Shapley values, with the error of NumPy / LAPACK on the same route as the yardstick (judge)."""
    p = len(labels)
    n, m, R = 3 * p + 20, 2 * p + 15, 3
    d = hp_ref.gen(p, n, m, 10.0, 8100 + p)
    rng = np.random.default_rng(p)
    wa, we = rng.integers(0, 4, size=(R, n)), rng.integers(0, 4, size=(R, m))
    eng.boot_load(*d, 0.0, grouped=True)
    phi, r2, base, info = eng.boot_groups_run(labels, R, 0, wa.astype(np.float64), we.astype(np.float64))
    assert not info.any()
    dev = np.abs(phi.sum(axis=1) - (r2 - base))
    print(f"GBOOT p={p} |sum phi - (r2 - r2_base)| = {dev.max():.3e}")
    assert dev.max() <= 1e-12
    if not (labels == -1).any():
        assert not base.any()
    for r in checked:
        rows = (np.repeat(d[0], wa[r], axis=0), np.repeat(d[1], we[r], axis=0), np.repeat(d[2], wa[r]),
                np.repeat(d[3], we[r]))
        truth = hp_ref.Problem(*rows)
        want = truth.shapley(labels)
        plain = group_shapley(*gram_problem(*rows), labels)
        e_plain = float(np.abs(plain - want).max())
        judge(f"grouped bootstrap replicate p={p} r={r}", phi[r], want, e_plain, 0, truth.min_pivot / threshold(p))


# ---- 4. reproducible, block-independent, counts = weights ------------------------------------------------------------
# g = 8: one high subset a unit.  20 singletons (2^14 high subsets, two a unit) with R = 22: the replicates a launch takes
# change with the block (20, 1, 3) and with the cut by `first`.  p = 64 in 20 groups (2^18, 32 a unit): six launches a
# replicate, whose cut must not move with the block either.
@pytest.mark.parametrize("sizes,R", [([5] * 8, 7), ([1] * 20, 22), ([4] * 4 + [3] * 16, 4)])
def test_bits_do_not_depend_on_the_run_the_block_or_the_form_of_the_weights(eng, sizes, R):
    labels = labels_of(sizes, 0, seed=8)
    p, n, m, seed = len(labels), 300, 270, 11
    eng.boot_load(*data(p, n=n, m=m, seed=3), 0.0, grouped=True)
    base = eng.boot_groups_run(labels, R, seed)
    assert not base[3].any()
    for block in (0, 1, 3):
        again = eng.boot_groups_run(labels, R, seed, block=block)
        for a, b in zip(base, again):
            np.testing.assert_array_equal(a, b)
    tail = eng.boot_groups_run(labels, R - 2, seed, first=2)                # a run cut into calls
    for a, b in zip(base, tail):
        np.testing.assert_array_equal(a[2:], b)
    wa = np.array([eng.boot_debug_counts(seed, r, 0) for r in range(R)], dtype=np.float64)
    we = np.array([eng.boot_debug_counts(seed, r, 1) for r in range(R)], dtype=np.float64)
    explicit = eng.boot_groups_run(labels, R, 999, wa, we)
    for a, b in zip(base, explicit):
        np.testing.assert_array_equal(a, b)
    assert np.abs(base[0] - base[0][0]).max() > 0                           # the replicates do differ


def test_a_seed_draws_the_same_rows_with_and_without_groups(eng):
    d = data(9, n=100, m=90, seed=4)
    eng.boot_load(*d, 0.0)
    plain = [eng.boot_debug_counts(7, r, s) for r in range(3) for s in (0, 1)]
    single = eng.boot_run(3, 7)
    grouped = eng.boot_groups_run(np.arange(9), 3, 7)                       # after the ungrouped load too
    eng.boot_load(*d, 0.0, grouped=True)
    again = [eng.boot_debug_counts(7, r, s) for r in range(3) for s in (0, 1)]
    for a, b in zip(plain, again):
        np.testing.assert_array_equal(a, b)
    # the same reduced problems: the same R^2, up to the rounding of two host Cholesky solves of a 9 x 9 system
    np.testing.assert_allclose(grouped[1], single[1], rtol=0, atol=1e-12)
    np.testing.assert_allclose(grouped[0], single[0], rtol=0, atol=1e-12)   # one column a group: the features' game


# ---- 5. a bad replicate stays alone ----------------------------------------------------------------------------------
def one_hot_case():
    labels = labels_of([6] * 6)
    p, n, m, R, j = 36, 120, 90, 5, 10                                      # column 10: in a high group
    rng = np.random.default_rng(70)
    Xa, Xe, ya, ye = data(p, n=n, m=m, seed=70)
    Xa = Xa.copy()
    Xa[:, j] = (np.arange(n) % 5 == 0).astype(np.float64)
    wa = rng.integers(1, 4, size=(R, n)).astype(np.float64)
    we = rng.integers(1, 4, size=(R, m)).astype(np.float64)
    wa[2, Xa[:, j] == 1] = 0.0                                       # replicate 2 never sees a row where column j is 1
    return labels, (Xa, Xe, ya, ye), wa, we


def test_a_failed_replicate_is_flagged_alone(eng):
    labels, d, wa, we = one_hot_case()
    eng.boot_load(*d, 0.0, grouped=True)
    phi, r2, base, info = eng.boot_groups_run(labels, len(wa), 0, wa, we)
    keep = [0, 1, 3, 4]
    assert info[2] & 1 and not info[keep].any()
    ref = eng.boot_groups_run(labels, 4, 0, wa[keep], we[keep])
    np.testing.assert_array_equal(phi[keep], ref[0])
    np.testing.assert_array_equal(r2[keep], ref[1])
    with pytest.warns(RuntimeWarning, match="1 of 5 bootstrap replicates"):
        res = ls_spa_bootstrap(*d, n_boot=5, weights=(wa, we), groups=labels)
    assert res.n_failed == 1 and np.isnan(res.replicates[2]).all() and np.isfinite(res.replicates[keep]).all()
    np.testing.assert_array_equal(res.replicates[keep], phi[keep])


# ---- 6. isolation and refusals ---------------------------------------------------------------------------------------
def test_a_grouped_run_leaves_the_loaded_problem_alone():
    d = data(8, n=120, m=90, seed=8)
    labels8 = labels_of([3, 3, 2])
    e = HipEngine(0)
    try:
        e.load_data(*d, 0.0)
        e.full_fit()
        before = (e.subsets_shapley()[0], e.groups_shapley(labels8)[0])
        e.boot_load(*data(40, n=70, m=60, seed=1), 0.5, grouped=True)
        e.boot_groups_run(labels_of([5] * 8), 9, 4)
        after = (e.subsets_shapley()[0], e.groups_shapley(labels8)[0])
        for a, b in zip(before, after):
            np.testing.assert_array_equal(a, b)
        e.boot_free()
        np.testing.assert_array_equal(e.groups_shapley(labels8)[0], before[1])
    finally:
        e.close()


def test_refusals_leave_a_working_context():
    e = HipEngine(0)
    try:
        with pytest.raises(LSSPANativeError, match="lsspa_boot_load comes first"):
            e.boot_groups_run(np.arange(4), 3, 0)
        with pytest.raises(ValueError, match="at most p = 64 columns"):
            e.boot_load(*data(65, n=80, m=80, seed=1), 0.0, grouped=True)
        with pytest.raises(LSSPANativeError, match="lsspa_boot_load comes first"):
            e.boot_groups_run(np.arange(4), 3, 0)
        labels = labels_of([5] * 8)
        e.boot_load(*data(40, n=70, m=60, seed=2), 0.0, grouped=True)
        good = e.boot_groups_run(labels, 3, 1)
        with pytest.raises(ValueError, match="at most p = 32 features"):
            e.boot_run(3, 1)
        bad = labels.copy()
        bad[0] = -2
        gap = labels.copy()
        gap[gap == 2] = 3
        for lab, what in ((bad, "outside -1"), (gap, "no column"), (labels[:-1], "length p = 40"),
                          (np.arange(40), "at most g = 32"), (np.full(40, -1), "at least one group")):
            with pytest.raises(ValueError, match=what):
                e.boot_groups_run(lab, 3, 1)
        w = np.ones((3, 70))
        w[1, 7] = -1.0
        with pytest.raises(ValueError, match="finite and >= 0"):
            e.boot_groups_run(labels, 3, 1, w, None)
        for a, b in zip(good, e.boot_groups_run(labels, 3, 1)):
            np.testing.assert_array_equal(a, b)
        assert e.boot_debug_grams(2)[0].shape == (2, 41, 41) and e.boot_timing()["enumeration"] > 0
    finally:
        e.close()


# ---- 7. public call --------------------------------------------------------------------------------------------------
def test_public_call():
    labels = labels_of([8, 8, 6, 6, 5, 4], 3, seed=2)
    p, g, n_boot = 40, 6, 40
    d = data(p, n=400, m=400, seed=9)
    res = ls_spa_bootstrap(*d, n_boot=n_boot, seed=5, groups=labels)
    point = ls_spa(*d, method="subsets", groups=labels)
    np.testing.assert_array_equal(res.attribution, point.attribution)
    np.testing.assert_array_equal(res.theta, point.theta)
    assert res.r_squared == point.r_squared and res.n_failed == 0
    assert res.attribution.shape == (g,) and res.theta.shape == (p,) and res.replicates.shape == (n_boot, g)
    assert res.std_error.shape == res.lower.shape == res.upper.shape == (g,) and res.prob_greater.shape == (g, g)
    assert res.r_squared_replicates.shape == res.baseline_r_squared_replicates.shape == (n_boot,)
    assert np.all(res.lower <= res.upper)
    np.testing.assert_allclose(res.replicates.sum(axis=1), res.r_squared_replicates - res.baseline_r_squared_replicates,
                               rtol=0, atol=1e-12)
    assert np.isfinite(res.baseline_r_squared_replicates).all() and res.baseline_r_squared_replicates.all()
    again = ls_spa_bootstrap(*d, n_boot=n_boot, seed=5, groups=labels)
    np.testing.assert_array_equal(again.replicates, res.replicates)
    np.testing.assert_array_equal(again.baseline_r_squared_replicates, res.baseline_r_squared_replicates)
    # one side only: the other side's weight is 1 -- the same as handing in ones; caller weights run
    one = ls_spa_bootstrap(*d, n_boot=8, seed=5, resample="train", groups=labels)
    ones = ls_spa_bootstrap(*d, n_boot=8, seed=5, weights=(None, np.ones((8, 400))), groups=labels)
    np.testing.assert_array_equal(one.replicates, ones.replicates)
    assert one.replicates.shape == (8, g) and np.isfinite(one.replicates).all()
