"""ls_spa_interactions_bootstrap on the MI355X (the INTER && REPS instantiation of csrc/k_subsets.hip,
lsspa_boot_interactions_run of include/lsspa.h): a replicate against the one-problem interaction enumeration bit for bit,
independence of how a run is cut, agreement with the phi bootstrap, a replicate against the long-double truth of
tests/hp_ref.py on the repeated rows, isolation of a failed replicate, context hygiene and the public call."""
import numpy as np
import pytest

import hp_ref
from ls_spa import ls_spa, ls_spa_bootstrap, ls_spa_interactions, ls_spa_interactions_bootstrap
from ls_spa._engine import HipEngine, debug_boot_plan
from ls_spa._native import LSSPANativeError
from test_gpu_accuracy import judge, threshold
from test_gpu_bootstrap import one_hot_case
from test_gpu_interactions import truth_interactions
from test_interactions_host import exact_interactions, shap_matrix
from test_subsets_host import data, gram_problem

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = HipEngine(0)
    yield e
    e.close()


def reduced_of(Sa, Se, W, r, p, reg):
    """Replicate r's reduced problem as finalise forms it, in load_reduced's arguments."""
    G = Sa[r, :p, :p] / W[r] + reg * np.eye(p)
    g = Sa[r, :p, p] / W[r]
    return (G, g, float(g @ np.linalg.solve(G, g)) * 1.01 + 1.0, Se[r, p, p]), dict(H=Se[r, :p, :p], h=Se[r, :p, p])


# ---- 1. same problem, same bits ----------------------------------------------------------------------------------------
# p = 5: no high feature, 32 live lanes; 6: nh = 0; 7: nh = 1, the high-high branch off; 8: the first high-high pair;
# 12: 15 pairs, one slot a lane; 18: 66 high-high pairs, a second slot on two lanes; 20: per = 2, the in-kernel step loop;
# 27: per = 256 against 128 steps, two launches add into one row.
@pytest.mark.parametrize("p,R", [(5, 3), (6, 3), (7, 3), (8, 3), (12, 3), (18, 3), (20, 3), (27, 2)])
def test_a_replicate_has_the_bits_of_the_one_problem_interactions(eng, p, R):
    n, m, reg = 50, 40, 0.25
    d = data(p, n=n, m=m, seed=40 + p)
    rng = np.random.default_rng(p)
    wa, we = rng.integers(0, 4, size=(R, n)).astype(np.float64), rng.integers(0, 4, size=(R, m)).astype(np.float64)
    plan = debug_boot_plan(R, n, m, p, inter=True)
    if p == 20:
        assert plan["per"] == 2 and plan["steps"] == 2
    if p == 27:
        assert plan["per"] == 256 and plan["steps"] == 128 and plan["enum_reps"] == 1
    eng.boot_load(*d, reg)
    Sa, Se, W = eng.boot_debug_grams(R, wa, we)
    phi, inter, r2, info = eng.boot_interactions_run(R, 0, wa, we)
    other = HipEngine(0)
    try:
        for r in range(R):
            args, kw = reduced_of(Sa, Se, W, r, p, reg)
            other.load_reduced(*args, **kw)
            want_phi, want, bits = other.subsets_interactions()
            assert bits == 0 and info[r] == 0
            np.testing.assert_array_equal(phi[r], want_phi)
            np.testing.assert_array_equal(inter[r], want)
    finally:
        other.close()


# ---- 2. bits do not depend on how the run is cut -------------------------------------------------------------------------
def test_bits_do_not_depend_on_the_run_the_block_or_the_form_of_the_weights(eng):
    p, n, m, R, seed = 9, 300, 270, 7, 11
    eng.boot_load(*data(p, n=n, m=m, seed=3), 0.0)
    base = eng.boot_interactions_run(R, seed)
    assert not base[3].any()
    for block in (0, 1, 3):
        again = eng.boot_interactions_run(R, seed, block=block)
        for a, b in zip(base, again):
            np.testing.assert_array_equal(a, b)
    tail = eng.boot_interactions_run(R - 2, seed, first=2)          # a run cut into calls
    for a, b in zip(base, tail):
        np.testing.assert_array_equal(a[2:], b)
    wa = np.array([eng.boot_debug_counts(seed, r, 0) for r in range(R)], dtype=np.float64)
    we = np.array([eng.boot_debug_counts(seed, r, 1) for r in range(R)], dtype=np.float64)
    explicit = eng.boot_interactions_run(R, 999, wa, we)
    for a, b in zip(base, explicit):
        np.testing.assert_array_equal(a, b)
    for a, b in zip(base, eng.boot_interactions_run(R, seed)):      # two identical calls
        np.testing.assert_array_equal(a, b)
    assert np.abs(base[1] - base[1][0]).max() > 0                   # the replicates do differ


# ---- 3. agreement with the phi bootstrap ---------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [9, 12])
def test_phi_is_the_phi_bootstraps_and_the_matrix_sums_to_it(eng, p):
    R, seed = 5, 17
    eng.boot_load(*data(p, n=200, m=150, seed=p), 0.0)
    phi, inter, r2, info = eng.boot_interactions_run(R, seed)
    want = eng.boot_run(R, seed)
    np.testing.assert_array_equal(phi, want[0])
    np.testing.assert_array_equal(r2, want[1])
    np.testing.assert_array_equal(info, want[2])
    assert not info.any()
    for r in range(R):
        np.testing.assert_array_equal(inter[r], inter[r].T)
        assert not np.diag(inter[r]).any()
        Phi = shap_matrix(inter[r], phi[r])
        np.testing.assert_array_equal(Phi, Phi.T)
        np.testing.assert_allclose(Phi.sum(axis=1), phi[r], rtol=0, atol=1e-12)
        assert abs(Phi.sum() - r2[r]) <= 1e-12


# ---- 4. truth ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [6, 7])
def test_a_replicate_is_the_interaction_index_of_the_repeated_rows(eng, p):
    """Judged as the one-problem enumeration is in tests/test_gpu_interactions.py: against the long-double index, with
    the error of the fp64 host oracle on the same route as the yardstick (judge)."""
    n, m, R, r = 3 * p + 20, 2 * p + 15, 2, 1
    d = hp_ref.gen(p, n, m, 10.0, 8200 + p)
    rng = np.random.default_rng(p)
    wa, we = rng.integers(0, 4, size=(R, n)), rng.integers(0, 4, size=(R, m))
    eng.boot_load(*d, 0.0)
    phi, inter, r2, info = eng.boot_interactions_run(R, 0, wa.astype(np.float64), we.astype(np.float64))
    assert not info.any()
    rows = (np.repeat(d[0], wa[r], axis=0), np.repeat(d[1], we[r], axis=0), np.repeat(d[2], wa[r]), np.repeat(d[3], we[r]))
    truth = hp_ref.Problem(*rows)
    want = truth_interactions(truth)
    e_plain = float(np.abs(exact_interactions(*gram_problem(*rows)) - want).max())
    judge(f"interactions bootstrap replicate p={p} r={r}", inter[r], want, e_plain, 0, truth.min_pivot / threshold(p))


# ---- 5. a failed replicate stays alone -----------------------------------------------------------------------------------
def test_a_failed_replicate_is_flagged_alone(eng):
    d, wa, we = one_hot_case()
    eng.boot_load(*d, 0.0)
    phi, inter, r2, info = eng.boot_interactions_run(len(wa), 0, wa, we)
    keep = [0, 1, 3, 4]
    assert info[2] & 1 and not info[keep].any()
    ref = eng.boot_interactions_run(4, 0, wa[keep], we[keep])
    np.testing.assert_array_equal(phi[keep], ref[0])
    np.testing.assert_array_equal(inter[keep], ref[1])
    np.testing.assert_array_equal(r2[keep], ref[2])
    with pytest.warns(RuntimeWarning, match="1 of 5 bootstrap replicates"):
        res = ls_spa_interactions_bootstrap(*d, n_boot=5, weights=(wa, we))
    assert res.n_failed == 1 and np.isnan(res.replicates[2]).all() and np.isfinite(res.replicates[keep]).all()
    np.testing.assert_array_equal(res.attribution_replicates[keep], phi[keep])


# ---- 6. context hygiene and the public call --------------------------------------------------------------------------------
def test_a_run_leaves_the_rest_of_the_context_alone():
    p = 8
    d = data(p, n=120, m=90, seed=8)
    e = HipEngine(0)
    try:
        kw = dict(method="argsort", seed=3, batch_size=16, max_samples=32, tolerance=0.0, _engine=e)
        before_run = ls_spa(*d, **kw)
        before = (e.subsets_interactions()[:2], e.stats(), e.info())
        e.boot_load(*hp_ref.gen(5, 33, 21, 1.0, 1), 0.5)
        boot_before = e.boot_run(9, 4)
        e.boot_interactions_run(9, 4)
        assert e.boot_timing()["enumeration"] > 0
        for a, b in zip(boot_before, e.boot_run(9, 4)):             # the phi bootstrap still works, with the same bits
            np.testing.assert_array_equal(a, b)
        after = (e.subsets_interactions()[:2], e.stats(), e.info())
        np.testing.assert_array_equal(before[0][0], after[0][0])
        np.testing.assert_array_equal(before[0][1], after[0][1])
        assert before[1][0] == after[1][0] and before[2] == after[2]
        np.testing.assert_array_equal(before[1][1], after[1][1])
        np.testing.assert_array_equal(before[1][2], after[1][2])
        e.boot_free()
        after_run = ls_spa(*d, **kw)
        np.testing.assert_array_equal(before_run.attribution, after_run.attribution)
        np.testing.assert_array_equal(before_run.error_history, after_run.error_history)
    finally:
        e.close()


def test_refusals_leave_a_working_context():
    e = HipEngine(0)
    try:
        with pytest.raises(LSSPANativeError, match="lsspa_boot_load comes first"):
            e.boot_interactions_run(3, 0)
        d = data(4, n=30, m=20, seed=2)
        e.boot_load(*data(40, n=70, m=60, seed=2), 0.0, grouped=True)
        with pytest.raises(ValueError, match="at most p = 32 features"):
            e.boot_interactions_run(3, 1)
        e.boot_load(*d, 0.0)
        good = e.boot_interactions_run(3, 1)
        lib, h = e._lib, e._h
        out = [np.zeros(3 * 16) for _ in range(3)]
        inf = np.zeros(3, dtype=np.int32)
        from ls_spa import _native as N
        for k in range(4):                                             # a NULL output pointer, each in turn
            ptrs = [N.dptr(out[0]), N.dptr(out[1]), N.dptr(out[2]), N.iptr(inf)]
            ptrs[k] = None
            assert lib.lsspa_boot_interactions_run(h, 3, 1, 0, None, None, 0, *ptrs) == 1    # LSSPA_ERR_ARG
        for bad, what in ((-1.0, "finite and >= 0"), (np.nan, "finite and >= 0")):
            w = np.ones((3, 30))
            w[1, 7] = bad
            with pytest.raises(ValueError, match=what):
                e.boot_interactions_run(3, 1, w, None)
        w = np.ones((3, 20))
        w[2] = 0.0
        with pytest.raises(ValueError, match="replicate 2 sum to 0"):
            e.boot_interactions_run(3, 1, None, w)
        for a, b in zip(good, e.boot_interactions_run(3, 1)):
            np.testing.assert_array_equal(a, b)
        e.load_data(*d, 0.0)
        e.full_fit()
        assert np.isfinite(e.subsets_interactions()[1]).all()
    finally:
        e.close()


def test_public_call():
    p, n_boot = 8, 64
    d = data(p, n=400, m=400, seed=9)
    res = ls_spa_interactions_bootstrap(*d, n_boot=n_boot, seed=5)
    point = ls_spa_interactions(*d)
    np.testing.assert_array_equal(res.interactions, point.interactions)
    np.testing.assert_array_equal(res.attribution, point.attribution)
    np.testing.assert_array_equal(res.theta, point.theta)
    assert res.r_squared == point.r_squared and res.n_failed == 0
    assert res.replicates.shape == (n_boot, p, p) and res.attribution_replicates.shape == (n_boot, p)
    assert res.std_error.shape == res.lower.shape == res.upper.shape == res.prob_positive.shape == (p, p)
    assert res.baseline_r_squared_replicates is None
    assert np.all(res.lower <= res.upper)
    # an interval brackets at least one replicate, entry by entry
    inside = (res.replicates >= res.lower) & (res.replicates <= res.upper)
    assert inside.any(axis=0).all()
    np.testing.assert_array_equal(res.replicates, np.swapaxes(res.replicates, 1, 2))
    np.testing.assert_allclose(res.replicates.sum(axis=2), res.attribution_replicates, rtol=0, atol=1e-12)
    np.testing.assert_allclose(res.replicates.sum(axis=(1, 2)), res.r_squared_replicates, rtol=0, atol=1e-12)
    np.testing.assert_array_equal(res.prob_positive, (res.replicates > 0).mean(axis=0))
    # a given seed resamples the rows of ls_spa_bootstrap: the replicates' attribution is that call's, bit for bit
    np.testing.assert_array_equal(res.attribution_replicates, ls_spa_bootstrap(*d, n_boot=n_boot, seed=5).replicates)
    again = ls_spa_interactions_bootstrap(*d, n_boot=n_boot, seed=5)
    np.testing.assert_array_equal(again.replicates, res.replicates)
    np.testing.assert_array_equal(again.r_squared_replicates, res.r_squared_replicates)
    one = ls_spa_interactions_bootstrap(*d, n_boot=8, seed=5, resample="train")
    ones = ls_spa_interactions_bootstrap(*d, n_boot=8, seed=5, weights=(None, np.ones((8, 400))))
    np.testing.assert_array_equal(one.replicates, ones.replicates)
    assert one.replicates.shape == (8, p, p) and np.isfinite(one.replicates).all()
