"""ls_spa_interactions_bootstrap(groups=) on the MI355X (the INTER && REPS instantiation of csrc/k_groups.hip,
lsspa_boot_groups_interactions_run of include/lsspa.h): a replicate against the one-problem grouped interaction
enumeration bit for bit, independence of how a run is cut, agreement with the grouped phi bootstrap, a replicate against
the long-double truth of tests/hp_ref.py on the repeated rows, isolation of a failed replicate, refusals and the public
call."""
import numpy as np
import pytest

import hp_ref
from ls_spa import ls_spa_bootstrap, ls_spa_interactions, ls_spa_interactions_bootstrap
from ls_spa._engine import HipEngine, debug_boot_groups_plan
from ls_spa._native import LSSPANativeError
from test_gpu_accuracy import judge, threshold
from test_gpu_group_bootstrap import one_hot_case
from test_gpu_group_interactions import truth_group_interactions
from test_group_interactions_host import group_interactions
from test_groups_host import labels_of
from test_interactions_host import shap_matrix
from test_subsets_host import data, gram_problem

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eng():
    e = HipEngine(0)
    yield e
    e.close()


# ---- 1. same problem, same bits ----------------------------------------------------------------------------------------
# name: (labels, gh).  The low groups are the smallest ones while their columns total at most six.
LAYOUTS = {
    "g4_p9_baseline_gh0": (labels_of([2, 2, 1, 1], 3, seed=4), 0),
    "g7_p12_gh1": (labels_of([1] * 6 + [6]), 1),
    "g7_p12_baseline_gh1": (labels_of([1] * 6 + [4], 2, seed=7), 1),
    "g9_p20": (labels_of([1, 1, 1, 1, 2, 3, 3, 4, 4], 0, seed=9), 4),
    "g9_p20_baseline": (labels_of([1, 1, 1, 1, 2, 3, 3, 3, 3], 2, seed=9), 4),
    "g13_p30_baseline": (labels_of([1] * 6 + [3] * 6 + [2], 4, seed=13), 7),
    "g13_p30": (labels_of([1] * 6 + [4, 4, 4, 3, 3, 3, 3]), 7),
    "g10_p64_five_column_blocks": (labels_of([1, 1, 1, 1, 2, 12, 12, 12, 11, 11], 0, seed=64), 5),
    "g10_p64_baseline": (labels_of([1, 1, 1, 1, 2, 11, 11, 11, 10, 10], 5, seed=64), 5),
}


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_a_replicate_has_the_bits_of_the_one_problem_interactions(eng, name):
    labels, gh = LAYOUTS[name]
    p, n, m, R, reg = len(labels), 80, 70, 3, 0.25
    plan = debug_boot_groups_plan(R, n, m, labels, inter=True)
    assert plan["units"] * plan["per"] == 1 << gh and plan["cb"] == (p + 16) // 16
    d = data(p, n=n, m=m, seed=40 + p)
    rng = np.random.default_rng(p)
    wa, we = rng.integers(0, 4, size=(R, n)).astype(np.float64), rng.integers(0, 4, size=(R, m)).astype(np.float64)
    eng.boot_load(*d, reg, grouped=True)
    Sa, Se, W = eng.boot_debug_grams(R, wa, we)
    phi, inter, r2, base, info = eng.boot_groups_interactions_run(labels, R, 0, wa, we)
    if not (labels == -1).any():
        assert not base.any()
    other = HipEngine(0)
    try:
        for r in range(R):
            G = Sa[r, :p, :p] / W[r] + reg * np.eye(p)
            g = Sa[r, :p, p] / W[r]
            other.load_reduced(G, g, float(g @ np.linalg.solve(G, g)) * 1.01 + 1.0, Se[r, p, p], H=Se[r, :p, :p],
                               h=Se[r, :p, p])
            want_phi, want, bits = other.groups_interactions(labels)
            assert bits == 0 and info[r] == 0
            np.testing.assert_array_equal(phi[r], want_phi)
            np.testing.assert_array_equal(inter[r], want)
    finally:
        other.close()


# ---- 2. bits do not depend on how the run is cut -------------------------------------------------------------------------
def test_bits_do_not_depend_on_the_run_the_block_or_the_form_of_the_weights(eng):
    labels = labels_of([1] * 6 + [3, 3, 4, 4], 2, seed=8)                   # g = 10 over p = 22, four high groups
    p, n, m, R, seed = len(labels), 300, 270, 7, 11
    eng.boot_load(*data(p, n=n, m=m, seed=3), 0.0, grouped=True)
    base = eng.boot_groups_interactions_run(labels, R, seed)
    assert not base[4].any()
    for block in (0, 1, 3):
        again = eng.boot_groups_interactions_run(labels, R, seed, block=block)
        for a, b in zip(base, again):
            np.testing.assert_array_equal(a, b)
    tail = eng.boot_groups_interactions_run(labels, R - 2, seed, first=2)   # a run cut into calls
    for a, b in zip(base, tail):
        np.testing.assert_array_equal(a[2:], b)
    wa = np.array([eng.boot_debug_counts(seed, r, 0) for r in range(R)], dtype=np.float64)
    we = np.array([eng.boot_debug_counts(seed, r, 1) for r in range(R)], dtype=np.float64)
    explicit = eng.boot_groups_interactions_run(labels, R, 999, wa, we)
    for a, b in zip(base, explicit):
        np.testing.assert_array_equal(a, b)
    for a, b in zip(base, eng.boot_groups_interactions_run(labels, R, seed)):   # two identical calls
        np.testing.assert_array_equal(a, b)
    assert np.abs(base[1] - base[1][0]).max() > 0                           # the replicates do differ


# ---- 3. agreement with the grouped phi bootstrap ---------------------------------------------------------------------------
@pytest.mark.parametrize("labels", [labels_of([2, 2, 2, 3], 0, seed=1), labels_of([1] * 6 + [3, 4, 5], 3, seed=2)])
def test_phi_is_the_phi_bootstraps_and_the_matrix_sums_to_it(eng, labels):
    p, R, seed = len(labels), 5, 17
    eng.boot_load(*data(p, n=200, m=150, seed=p), 0.0, grouped=True)
    phi, inter, r2, base, info = eng.boot_groups_interactions_run(labels, R, seed)
    want = eng.boot_groups_run(labels, R, seed)
    for a, b in zip((phi, r2, base, info), want):
        np.testing.assert_array_equal(a, b)
    assert not info.any()
    for r in range(R):
        np.testing.assert_array_equal(inter[r], inter[r].T)
        assert not np.diag(inter[r]).any()
        Phi = shap_matrix(inter[r], phi[r])
        np.testing.assert_array_equal(Phi, Phi.T)
        np.testing.assert_allclose(Phi.sum(axis=1), phi[r], rtol=0, atol=1e-12)
        assert abs(Phi.sum() - (r2[r] - base[r])) <= 1e-12


# ---- 4. truth ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("labels", [labels_of([2, 3, 1, 4, 2], 2, seed=3), labels_of([1] * 6 + [3, 4], 0, seed=5)])
def test_a_replicate_is_the_group_interaction_index_of_the_repeated_rows(eng, labels):
    """Judged as the one-problem grouped enumeration is in tests/test_gpu_group_interactions.py: against the long-double
    index, with the error of the fp64 host oracle on the same route as the yardstick (judge)."""
    p = len(labels)
    n, m, R, r = 3 * p + 20, 2 * p + 15, 2, 1
    d = hp_ref.gen(p, n, m, 10.0, 8300 + p)
    rng = np.random.default_rng(p)
    wa, we = rng.integers(0, 4, size=(R, n)), rng.integers(0, 4, size=(R, m))
    eng.boot_load(*d, 0.0, grouped=True)
    phi, inter, r2, base, info = eng.boot_groups_interactions_run(labels, R, 0, wa.astype(np.float64),
                                                                  we.astype(np.float64))
    assert not info.any()
    rows = (np.repeat(d[0], wa[r], axis=0), np.repeat(d[1], we[r], axis=0), np.repeat(d[2], wa[r]), np.repeat(d[3], we[r]))
    truth = hp_ref.Problem(*rows)
    want = truth_group_interactions(truth, labels)
    e_plain = float(np.abs(group_interactions(*gram_problem(*rows), labels) - want).max())
    judge(f"grouped interactions bootstrap replicate p={p} r={r}", inter[r], want, e_plain, 0,
          truth.min_pivot / threshold(p))


# ---- 5. a failed replicate stays alone -----------------------------------------------------------------------------------
def test_a_failed_replicate_is_flagged_alone(eng):
    labels, d, wa, we = one_hot_case()
    eng.boot_load(*d, 0.0, grouped=True)
    phi, inter, r2, base, info = eng.boot_groups_interactions_run(labels, len(wa), 0, wa, we)
    keep = [0, 1, 3, 4]
    assert info[2] & 1 and not info[keep].any()
    ref = eng.boot_groups_interactions_run(labels, 4, 0, wa[keep], we[keep])
    np.testing.assert_array_equal(phi[keep], ref[0])
    np.testing.assert_array_equal(inter[keep], ref[1])
    np.testing.assert_array_equal(r2[keep], ref[2])


# ---- 6. context hygiene, refusals and the public call ----------------------------------------------------------------------
def test_refusals_leave_a_working_context():
    e = HipEngine(0)
    try:
        with pytest.raises(LSSPANativeError, match="lsspa_boot_load comes first"):
            e.boot_groups_interactions_run(np.arange(4), 3, 0)
        labels = labels_of([5] * 8)
        e.boot_load(*data(40, n=70, m=60, seed=2), 0.0, grouped=True)
        good = e.boot_groups_interactions_run(labels, 3, 1)
        phi_before = e.boot_groups_run(labels, 3, 1)
        bad = labels.copy()
        bad[0] = -2
        gap = labels.copy()
        gap[gap == 2] = 3
        for lab, what in ((bad, "outside -1"), (gap, "no column"), (labels[:-1], "length p = 40"),
                          (np.arange(40), "at most g = 32"), (np.full(40, -1), "at least one group")):
            with pytest.raises(ValueError, match=what):
                e.boot_groups_interactions_run(lab, 3, 1)
        w = np.ones((3, 70))
        w[1, 7] = -1.0
        with pytest.raises(ValueError, match="finite and >= 0"):
            e.boot_groups_interactions_run(labels, 3, 1, w, None)
        for a, b in zip(good, e.boot_groups_interactions_run(labels, 3, 1)):
            np.testing.assert_array_equal(a, b)
        for a, b in zip(phi_before, e.boot_groups_run(labels, 3, 1)):
            np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(good[0], phi_before[0])
        assert e.boot_debug_grams(2)[0].shape == (2, 41, 41) and e.boot_timing()["enumeration"] > 0
    finally:
        e.close()


def test_public_call():
    labels = labels_of([8, 8, 6, 6, 5, 4], 3, seed=2)
    p, g, n_boot = 40, 6, 64
    d = data(p, n=400, m=400, seed=9)
    res = ls_spa_interactions_bootstrap(*d, n_boot=n_boot, seed=5, groups=labels)
    point = ls_spa_interactions(*d, groups=labels)
    np.testing.assert_array_equal(res.interactions, point.interactions)
    np.testing.assert_array_equal(res.attribution, point.attribution)
    np.testing.assert_array_equal(res.theta, point.theta)
    assert res.r_squared == point.r_squared and res.n_failed == 0
    assert res.interactions.shape == (g, g) and res.theta.shape == (p,) and res.replicates.shape == (n_boot, g, g)
    assert res.std_error.shape == res.lower.shape == res.upper.shape == res.prob_positive.shape == (g, g)
    assert res.r_squared_replicates.shape == res.baseline_r_squared_replicates.shape == (n_boot,)
    assert np.all(res.lower <= res.upper)
    inside = (res.replicates >= res.lower) & (res.replicates <= res.upper)
    assert inside.any(axis=0).all()                                        # an interval brackets at least one replicate
    np.testing.assert_array_equal(res.replicates, np.swapaxes(res.replicates, 1, 2))
    np.testing.assert_allclose(res.replicates.sum(axis=2), res.attribution_replicates, rtol=0, atol=1e-12)
    np.testing.assert_allclose(res.replicates.sum(axis=(1, 2)),
                               res.r_squared_replicates - res.baseline_r_squared_replicates, rtol=0, atol=1e-12)
    np.testing.assert_array_equal(res.prob_positive, (res.replicates > 0).mean(axis=0))
    np.testing.assert_array_equal(res.attribution_replicates,
                                  ls_spa_bootstrap(*d, n_boot=n_boot, seed=5, groups=labels).replicates)
    again = ls_spa_interactions_bootstrap(*d, n_boot=n_boot, seed=5, groups=labels)
    np.testing.assert_array_equal(again.replicates, res.replicates)
    one = ls_spa_interactions_bootstrap(*d, n_boot=8, seed=5, resample="train", groups=labels)
    assert one.replicates.shape == (8, g, g) and np.isfinite(one.replicates).all()
