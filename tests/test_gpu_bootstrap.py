"""ls_spa_bootstrap on the MI355X (csrc/k_boot.hip, the replicate dimension of csrc/k_subsets.hip, lsspa_boot_* of
include/lsspa.h): the weighted Gram sums against an integer truth bit for bit, the counts against tests/boot_ref.py, a
replicate against the long-double truth of tests/hp_ref.py on the repeated rows and against the one-problem enumeration
bit for bit, reproducibility, isolation of a failed replicate, and the public call."""
import itertools

import numpy as np
import pytest

import boot_ref
import gram_cases
import hp_ref
from ls_spa import ls_spa, ls_spa_bootstrap
from ls_spa._engine import HipEngine, debug_boot_plan
from ls_spa._native import LSSPANativeError
from test_gpu_accuracy import MG, T0, judge, threshold
from test_subsets_host import data, exact_shapley, gram_problem

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = HipEngine(0)
    yield e
    e.close()


# ---- 1. exact sums ---------------------------------------------------------------------------------------------------
P_AXIS = (1, 2, 6, 7, 15, 16, 17, 31, 32)      # c = p + 1 = 16 | 17 and 32 | 33: the edges of the 16-column blocks
R_AXIS = (1, 15, 16, 17, 33)                   # a workgroup carries 16 replicates (8 with three column blocks)
# The smallest n with several row slices and a ragged last one: a slice is max(256, ceil(n / 128) rounded up to 4) rows
# (boot_plan), so up to n = 512 there are at most two slices, both full at 512; n = 513 is three slices, the last of ONE
# row -- also a last step of the four-row loop with three dead rows.
N_SLICES = 513
N_AXIS = (1, 3, 4, 5, 63, 64, 65, N_SLICES)    # 4-row steps; 64: a multiple of the step; slices


def _sum_cases():
    out = [(p, 17, 65) for p in P_AXIS] + [(16, R, 5) for R in R_AXIS] + [(15, 16, n) for n in N_AXIS]
    out += list(itertools.product((15, 16, 31, 32), (15, 16, 17), (3, 4, 5, 64, 65)))     # two tile edges at once
    out += [(p, R, N_SLICES) for p in (16, 32) for R in (17, 33)]
    return sorted(set(out))


def test_the_slice_plan_is_what_the_cases_were_chosen_for():
    assert debug_boot_plan(1, 512, 512, 16)["slices_train"] == 2 and debug_boot_plan(1, 512, 512, 16)["rps_train"] == 256
    plan = debug_boot_plan(1, N_SLICES, 5, 16)
    assert (plan["slices_train"], plan["rps_train"], plan["slices_test"]) == (3, 256, 1)
    assert [debug_boot_plan(1, 9, 9, p)["cb"] for p in (15, 16, 31, 32)] == [1, 2, 2, 3]


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
    Xa, ya = gram_cases.integer_data(gram_cases.seed_of(f"boot_tr_{p}_{n}"), n, p, "float64")
    Xe, ye = gram_cases.integer_data(gram_cases.seed_of(f"boot_te_{p}_{m}"), m, p, "float64")
    wa, we = int_weights(rng, R, n), int_weights(rng, R, m)
    eng.boot_load(Xa, Xe, ya, ye, 0.0)
    Sa, Se, ws = eng.boot_debug_grams(R, wa.astype(np.float64), we.astype(np.float64))
    for S, X, y, w in ((Sa, Xa, ya, wa), (Se, Xe, ye, we)):
        Z = np.concatenate([X, y[:, None]], axis=1).astype(np.int64)
        want = np.einsum("ri,ia,ib->rab", w.astype(np.int64), Z, Z)
        assert np.abs(want).max() < 2 ** 53
        np.testing.assert_array_equal(S, want.astype(np.float64))
    np.testing.assert_array_equal(ws, wa.sum(axis=1).astype(np.float64))


# ---- 2. counts -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1000])
def test_counts_match_the_numpy_restatement(eng, n):
    d = data(3, n=n, m=n, seed=n)
    eng.boot_load(*d, 0.0)
    for seed in (42, 2 ** 63 + 12345):
        for r in (0, 1, 2 ** 31):
            got = [eng.boot_debug_counts(seed, r, side) for side in (0, 1)]
            for side in (0, 1):
                np.testing.assert_array_equal(got[side], boot_ref.counts(seed, r, side, n))
                assert got[side].sum() == n
            if n == 1000:
                assert not np.array_equal(got[0], got[1])


# ---- 3. one replicate is the existing attribution ----------------------------------------------------------------------
def ld_shapley(ref):
    """Problem.shapley without its p <= 12 limit (p = 13: 8192 subsets)."""
    p = ref.p
    tab = [ref.mask_value(k) for k in range(1 << p)]
    size = [bin(k).count("1") for k in range(1 << p)]
    from math import comb
    phi = ref.ar.zeros(p)
    for j in range(p):
        for k in range(1 << p):
            if not (k >> j) & 1:
                phi[j] = phi[j] + (tab[k | 1 << j] - tab[k]) / ref.ar.conv(np.float64(p * comb(p - 1, size[k])))
    return ref.ar.to_float(phi), float(tab[-1])


@pytest.mark.parametrize("p,checked", [(6, (0, 1, 2)), (7, (0, 1, 2)), (13, (1,))])
def test_a_replicate_is_the_attribution_of_the_repeated_rows(eng, p, checked):
    n, m, R = 3 * p + 20, 2 * p + 15, 3
    d = hp_ref.gen(p, n, m, 10.0, 8000 + p)
    rng = np.random.default_rng(p)
    wa, we = rng.integers(0, 4, size=(R, n)), rng.integers(0, 4, size=(R, m))
    eng.boot_load(*d, 0.0)
    phi, r2, info = eng.boot_run(R, 0, wa.astype(np.float64), we.astype(np.float64))
    assert not info.any()
    np.testing.assert_allclose(phi.sum(axis=1), r2, rtol=0, atol=1e-12)
    for r in checked:
        rows = (np.repeat(d[0], wa[r], axis=0), np.repeat(d[1], we[r], axis=0), np.repeat(d[2], wa[r]),
                np.repeat(d[3], we[r]))
        truth = hp_ref.Problem(*rows)
        want, want_r2 = ld_shapley(truth)
        plain = exact_shapley(*gram_problem(*rows))
        e_plain = float(np.abs(plain - want).max())
        judge(f"bootstrap replicate p={p} r={r}", phi[r], want, e_plain, 0, truth.min_pivot / threshold(p))
        assert abs(r2[r] - want_r2) <= max(T0["float64"], MG * abs(plain.sum() - want_r2))


# ---- 4. same G, same bits ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [5, 6, 7, 12])
def test_a_replicate_has_the_bits_of_the_one_problem_enumeration(eng, p):
    n, m, R, reg = 50, 40, 3, 0.25
    d = data(p, n=n, m=m, seed=40 + p)
    rng = np.random.default_rng(p)
    wa, we = rng.integers(0, 4, size=(R, n)).astype(np.float64), rng.integers(0, 4, size=(R, m)).astype(np.float64)
    eng.boot_load(*d, reg)
    Sa, Se, W = eng.boot_debug_grams(R, wa, we)
    phi, r2, info = eng.boot_run(R, 0, wa, we)
    other = HipEngine(0)
    try:
        for r in range(R):
            G = Sa[r, :p, :p] / W[r] + reg * np.eye(p)
            g = Sa[r, :p, p] / W[r]
            other.load_reduced(G, g, float(g @ np.linalg.solve(G, g)) * 1.01 + 1.0, Se[r, p, p], H=Se[r, :p, :p],
                               h=Se[r, :p, p])
            want, bits = other.subsets_shapley()
            assert bits == 0 and info[r] == 0
            np.testing.assert_array_equal(phi[r], want)
    finally:
        other.close()


# ---- 5. / 6. reproducible, block-independent, counts = weights -------------------------------------------------------
def test_bits_do_not_depend_on_the_run_the_block_or_the_form_of_the_weights(eng):
    p, n, m, R, seed = 9, 300, 270, 7, 11
    eng.boot_load(*data(p, n=n, m=m, seed=3), 0.0)
    base = eng.boot_run(R, seed)
    assert not base[2].any()
    for block in (0, 1, 3):
        again = eng.boot_run(R, seed, block=block)
        for a, b in zip(base, again):
            np.testing.assert_array_equal(a, b)
    tail = eng.boot_run(R - 2, seed, first=2)                       # a run cut into calls
    np.testing.assert_array_equal(tail[0], base[0][2:])
    wa = np.array([eng.boot_debug_counts(seed, r, 0) for r in range(R)], dtype=np.float64)
    we = np.array([eng.boot_debug_counts(seed, r, 1) for r in range(R)], dtype=np.float64)
    explicit = eng.boot_run(R, 999, wa, we)
    np.testing.assert_array_equal(explicit[0], base[0])
    np.testing.assert_array_equal(explicit[1], base[1])
    assert np.abs(base[0] - base[0][0]).max() > 0                   # the replicates do differ


# ---- 7. a bad replicate stays alone ----------------------------------------------------------------------------------
def one_hot_case():
    p, n, m, R, j = 6, 80, 60, 5, 4
    rng = np.random.default_rng(70)
    Xa, Xe, ya, ye = data(p, n=n, m=m, seed=70)
    Xa = Xa.copy()
    Xa[:, j] = (np.arange(n) % 5 == 0).astype(np.float64)
    wa = rng.integers(1, 4, size=(R, n)).astype(np.float64)
    we = rng.integers(1, 4, size=(R, m)).astype(np.float64)
    wa[2, Xa[:, j] == 1] = 0.0                                       # replicate 2 never sees a row where column j is 1
    return (Xa, Xe, ya, ye), wa, we


def test_a_failed_replicate_is_flagged_alone(eng):
    d, wa, we = one_hot_case()
    eng.boot_load(*d, 0.0)
    phi, r2, info = eng.boot_run(len(wa), 0, wa, we)
    keep = [0, 1, 3, 4]
    assert info[2] & 1 and not info[keep].any()
    ref = eng.boot_run(4, 0, wa[keep], we[keep])
    np.testing.assert_array_equal(phi[keep], ref[0])
    np.testing.assert_array_equal(r2[keep], ref[1])
    with pytest.warns(RuntimeWarning, match="1 of 5 bootstrap replicates"):
        res = ls_spa_bootstrap(*d, n_boot=5, weights=(wa, we))
    assert res.n_failed == 1 and np.isnan(res.replicates[2]).all() and np.isfinite(res.replicates[keep]).all()
    np.testing.assert_array_equal(res.replicates[keep], phi[keep])


# ---- 8. nothing else moves -------------------------------------------------------------------------------------------
def test_a_bootstrap_run_leaves_the_rest_of_the_context_alone():
    p = 8
    d = data(p, n=120, m=90, seed=8)
    e = HipEngine(0)
    try:
        kw = dict(method="argsort", seed=3, batch_size=16, max_samples=32, tolerance=0.0, _engine=e)
        before_run = ls_spa(*d, **kw)
        before = (e.subsets_shapley()[0], e.stats(), e.info())
        e.boot_load(*hp_ref.gen(5, 33, 21, 1.0, 1), 0.5)
        e.boot_run(9, 4)
        after = (e.subsets_shapley()[0], e.stats(), e.info())
        np.testing.assert_array_equal(before[0], after[0])
        assert before[1][0] == after[1][0] and before[2] == after[2]
        np.testing.assert_array_equal(before[1][1], after[1][1])
        np.testing.assert_array_equal(before[1][2], after[1][2])
        e.boot_free()
        np.testing.assert_array_equal(e.subsets_shapley()[0], before[0])
        after_run = ls_spa(*d, **kw)
        np.testing.assert_array_equal(before_run.attribution, after_run.attribution)
        np.testing.assert_array_equal(before_run.error_history, after_run.error_history)
    finally:
        e.close()


# ---- 9. public call ----------------------------------------------------------------------------------------------------
def test_public_call():
    d = data(8, n=400, m=400, seed=9)
    res = ls_spa_bootstrap(*d, n_boot=64, seed=5)
    point = ls_spa(*d, method="subsets")
    np.testing.assert_array_equal(res.attribution, point.attribution)
    np.testing.assert_array_equal(res.theta, point.theta)
    assert res.r_squared == point.r_squared and res.n_failed == 0 and res.replicates.shape == (64, 8)
    assert np.all(res.lower <= res.upper)
    alpha = (1.0 - 0.95) / 2.0               # the interval's levels as BootstrapResults states them: alpha, 1 - alpha
    np.testing.assert_array_equal(res.lower, np.quantile(res.replicates, alpha, axis=0))
    np.testing.assert_array_equal(res.upper, np.quantile(res.replicates, 1.0 - alpha, axis=0))
    assert res.r_squared_interval == (np.quantile(res.r_squared_replicates, alpha),
                                      np.quantile(res.r_squared_replicates, 1.0 - alpha))
    np.testing.assert_allclose(res.replicates.sum(axis=1), res.r_squared_replicates, rtol=0, atol=1e-12)
    ties = (res.replicates[:, :, None] == res.replicates[:, None, :]).any(axis=0)
    both = res.prob_greater + res.prob_greater.T
    assert np.all(both[~ties] == 1.0) and np.all(np.diag(res.prob_greater) == 0.0)
    # the point estimate lies inside the spread of its replicates; the same call twice has the same bits
    assert np.all(res.attribution > res.replicates.min(axis=0)) and np.all(res.attribution < res.replicates.max(axis=0))
    np.testing.assert_array_equal(ls_spa_bootstrap(*d, n_boot=64, seed=5).replicates, res.replicates)
    # one side only: the other side's weight is 1 -- the same as handing in ones
    one = ls_spa_bootstrap(*d, n_boot=8, seed=5, resample="train")
    ones = ls_spa_bootstrap(*d, n_boot=8, seed=5, weights=(None, np.ones((8, 400))))
    np.testing.assert_array_equal(one.replicates, ones.replicates)
    np.testing.assert_array_equal(one.replicates, ls_spa_bootstrap(*d, n_boot=64, seed=5, resample="train").replicates[:8])


# ---- 10. refusals ------------------------------------------------------------------------------------------------------
def test_refusals_leave_a_working_context():
    e = HipEngine(0)
    try:
        with pytest.raises(LSSPANativeError, match="lsspa_boot_load comes first"):
            e.boot_run(3, 0)
        with pytest.raises(ValueError, match="at most p = 32"):
            e.boot_load(*data(33, n=40, m=40, seed=1), 0.0)
        with pytest.raises(LSSPANativeError, match="lsspa_boot_load comes first"):
            e.boot_run(3, 0)
        d = data(4, n=30, m=20, seed=2)
        e.boot_load(*d, 0.0)
        good = e.boot_run(3, 1)
        for bad, what in ((-1.0, "finite and >= 0"), (np.nan, "finite and >= 0")):
            w = np.ones((3, 30))
            w[1, 7] = bad
            with pytest.raises(ValueError, match=what):
                e.boot_run(3, 1, w, None)
        w = np.ones((3, 20))
        w[2] = 0.0
        with pytest.raises(ValueError, match="replicate 2 sum to 0"):
            e.boot_run(3, 1, None, w)
        for a, b in zip(good, e.boot_run(3, 1)):
            np.testing.assert_array_equal(a, b)
        e.load_data(*d, 0.0)
        e.full_fit()
        assert np.isfinite(e.subsets_shapley()[0]).all()
    finally:
        e.close()
    with pytest.raises(ValueError, match="group the columns"):
        ls_spa_bootstrap(*data(33, n=40, m=40, seed=1))
