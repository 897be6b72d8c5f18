"""ls_spa_bootstrap_sampled without a GPU: lsspa_debug_boot_lift_plan at its edges, the driver through a NumPy double of
the engine's boot_lift_* methods (the refusals before any engine call, the result fields and tallies, failed replicates,
the orderings every replicate shares), and the truth of tests/boot_sampled_ref.py against hp_ref at p = 6."""
import itertools
import warnings

import numpy as np
import pytest

import boot_ref
import boot_sampled_ref as ref
import hp_ref
from ls_spa import (SampledBootstrapGroupResults, SampledBootstrapResults, SizeIncompatible, ls_spa_bootstrap_sampled)
from ls_spa._engine import debug_boot_lift_plan, debug_expand_groups


# ---- the planner -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c, cb, gram_form, lift_form", [(80, 5, 0, 0), (81, 6, 1, 0), (96, 6, 1, 0), (97, 7, 1, 0),
                                                         (112, 7, 1, 0), (113, 8, 1, 1), (128, 8, 1, 1)])
def test_plan_forms_at_the_column_block_edges(c, cb, gram_form, lift_form):
    plan = debug_boot_lift_plan(200, 10000, 9000, c - 1, c - 1, 1024, True)
    assert (plan["cb"], plan["gram_form"], plan["lift_form"]) == (cb, gram_form, lift_form)
    assert plan["rps_train"] % 4 == 0 and plan["slices_train"] * plan["rps_train"] >= 10000
    assert (plan["slices_train"] - 1) * plan["rps_train"] < 10000 and plan["slices_test"] * plan["rps_test"] >= 9000


@pytest.mark.parametrize("p", [1, 9, 40, 111, 112, 127])
@pytest.mark.parametrize("n_samples, anti", [(2, False), (3, True), (128, True), (129, True), (257, False), (1024, True)])
def test_plan_launch_bounds_and_a_cut_that_is_not_the_runs(p, n_samples, anti):
    base = debug_boot_lift_plan(1, 500, 400, p, p, n_samples, anti)
    per = 2 if anti else 1
    assert base["orderings_per_launch"] == per * base["samples_per_launch"] <= 256
    assert base["samples_per_launch"] == min(n_samples, 256 // per)
    assert base["sample_cuts"] == -(-n_samples // base["samples_per_launch"])
    grid = 2 ** 13 if p + 1 > 112 else 2 ** 16
    assert base["orderings_per_launch"] * base["reps_per_launch"] <= grid
    assert base["orderings_per_launch"] * base["reps_per_launch"] * p * 8 <= 256 << 20
    for R, block in ((1000, 0), (37, 1), (5, 3), (10 ** 6, 1024)):
        plan = debug_boot_lift_plan(R, 500, 400, p, p, n_samples, anti, block)
        for key in ("samples_per_launch", "orderings_per_launch", "reps_per_launch", "sample_cuts", "cb", "gram_form",
                    "rps_train", "rps_test", "slices_train", "slices_test"):
            assert plan[key] == base[key], key
        assert 1 <= plan["block"] <= min(R, 1024) and (block == 0 or plan["block"] <= block)
        assert plan["block"] == 1 or plan["block"] * plan["rep_bytes"] <= 256 << 20
        assert plan["n_blocks"] == -(-R // plan["block"]) and plan["raw_bytes"] <= 256 << 20
        assert plan["launches"] >= plan["n_blocks"] * plan["sample_cuts"]
    # a map's dimension does not enter the cut either
    assert debug_boot_lift_plan(1, 500, 400, p, 1, n_samples, anti)["reps_per_launch"] == base["reps_per_launch"]


def test_plan_refusals():
    for bad in ((1, 10, 10, 128, 128, 4, True), (1, 10, 10, 0, 1, 4, True), (1, 10, 10, 8, 9, 4, True),
                (1, 10, 10, 8, 0, 4, True), (1, 10, 10, 8, 8, 0, True), (0, 10, 10, 8, 8, 4, True),
                (1, 0, 10, 8, 8, 4, True), (1, 10, 2 ** 31, 8, 8, 4, True)):
        with pytest.raises(ValueError):
            debug_boot_lift_plan(*bad)
    with pytest.raises(ValueError):
        debug_boot_lift_plan(1, 10, 10, 8, 8, 4, True, -1)


# ---- the driver through a double of the engine ---------------------------------------------------------------------------
class NumpyEngine:
    """boot_lift_* in NumPy: a replicate's rows by boot_ref.indices (or its weights as integer repeats), its lifts by
    hp_ref.plain_lifts, the statistics as the plain moments of all samples.  fail: replicates to flag."""

    def __init__(self, fail=()):
        self.calls, self.labels, self.fail, self.seen = [], None, set(fail), []

    def boot_lift_load(self, Xa, Xe, ya, ye, reg):
        self.calls.append("load")
        self.data, self.reg = tuple(np.asarray(a, float) for a in (Xa, Xe, ya, ye)), reg
        self.p = self.data[0].shape[1]

    def boot_lift_set_players(self, labels):
        self.calls.append("players")
        self.labels = np.asarray(labels)

    def boot_lift_set_orderings(self, perms, antithetical):
        self.calls.append(("orderings", len(perms), bool(antithetical)))
        self.perms, self.anti = np.asarray(perms), bool(antithetical)

    def _rows(self, seed, r, wa, we):
        Xa, Xe, ya, ye = self.data
        ia = boot_ref.indices(seed, r, 0, len(Xa)) if wa is None else np.repeat(np.arange(len(Xa)), wa.astype(int))
        ie = boot_ref.indices(seed, r, 1, len(Xe)) if we is None else np.repeat(np.arange(len(Xe)), we.astype(int))
        return Xa[ia], Xe[ie], ya[ia], ye[ie]

    def _one(self, rows):
        self.seen.append(self.perms.copy())
        if self.labels is None:
            x = hp_ref.plain_lifts(*rows, self.reg, self.perms, self.anti)
            base = 0.0
        else:
            exp = debug_expand_groups(self.labels, self.perms, False)
            if self.anti:
                rev = debug_expand_groups(self.labels, np.ascontiguousarray(self.perms[:, ::-1]), False)
                exp = np.stack([exp, rev], axis=1).reshape(2 * len(self.perms), -1)
            x = ref.group_fold(hp_ref.plain_lifts(*rows, self.reg, exp, False), self.labels)
            if self.anti:
                x = 0.5 * x[0::2] + 0.5 * x[1::2]
            cols = np.nonzero(self.labels == -1)[0]
            base = float(hp_ref.Problem(*rows, self.reg).to_float(hp_ref.Problem(*rows, self.reg).subset_value(cols)))
        mean = x.mean(axis=0)
        r2 = float(hp_ref.Problem(*rows, self.reg).to_float(hp_ref.Problem(*rows, self.reg).subset_value(range(self.p))))
        return mean, ((x - mean) ** 2).sum(axis=0), r2, base

    def boot_lift_run(self, R, seed, w_train=None, w_test=None, block=0, first=0):
        self.calls.append(("run", R, seed, first, w_train is not None, w_test is not None))
        out = [self._one(self._rows(seed, first + r, None if w_train is None else w_train[r],
                                    None if w_test is None else w_test[r])) for r in range(R)]
        info = np.array([int(first + r in self.fail) for r in range(R)], dtype=np.int32)
        return tuple(np.array([o[k] for o in out]) for k in range(4)) + (info,)

    def boot_lift_point(self):
        self.calls.append("point")
        return self._one(self.data) + (0,)

    def boot_lift_problem(self, r, seed=0, w_train=None, w_test=None):
        assert r < 0
        G, g, H, h, yy = hp_ref.plain_gram(*self.data, self.reg)
        return G, g, H, h, 1.0 / yy

    def boot_lift_free(self):
        self.calls.append("free")


def small(p=6, seed=66):
    return hp_ref.gen(p, 60, 50, 1e1, seed)


def test_result_fields_tallies_and_the_shared_orderings():
    p = 6
    data = small(p)
    eng = NumpyEngine()
    res = ls_spa_bootstrap_sampled(*data, n_boot=8, n_samples=12, boot_seed=5, confidence=0.9, _engine=eng)
    assert isinstance(res, SampledBootstrapResults) and not isinstance(res, SampledBootstrapGroupResults)
    assert eng.calls[0] == "load" and eng.calls[-1] == "free" and "players" not in eng.calls
    assert eng.calls[1] == ("orderings", 12, True) and eng.calls[2] == "point"
    assert ("run", 8, 5, 0, False, False) in eng.calls
    # one set of orderings: the point problem and all eight replicates saw the same rows
    assert len(eng.seen) == 9 and all(np.array_equal(s, eng.seen[0]) for s in eng.seen)
    assert res.replicates.shape == (8, p) and res.replicate_errors.shape == (8, p) and res.n_samples == 12
    assert res.attribution.shape == res.attribution_errors.shape == res.std_error.shape == (p,)
    assert res.lower.shape == res.upper.shape == (p,) and res.prob_greater.shape == (p, p) and res.theta.shape == (p,)
    assert res.n_failed == 0 and res.confidence == 0.9 and res.r_squared_replicates.shape == (8,)
    alpha = (1.0 - 0.9) / 2.0
    np.testing.assert_array_equal(res.lower, np.quantile(res.replicates, alpha, axis=0))
    np.testing.assert_array_equal(res.upper, np.quantile(res.replicates, 1.0 - alpha, axis=0))
    np.testing.assert_array_equal(res.std_error, res.replicates.std(axis=0, ddof=1))
    np.testing.assert_array_equal(res.prob_greater, (res.replicates[:, :, None] > res.replicates[:, None, :]).mean(axis=0))
    assert np.abs(res.replicates.sum(axis=1) - res.r_squared_replicates).max() <= 1e-10
    assert abs(res.attribution.sum() - res.r_squared) <= 1e-10
    # the errors are sqrt(M2 / (n (n - 1)))
    rows = eng._rows(5, 3, None, None)
    x = hp_ref.plain_lifts(*rows, 0.0, eng.perms, True)
    np.testing.assert_allclose(res.replicates[3], x.mean(axis=0), rtol=0, atol=1e-14)
    np.testing.assert_allclose(res.replicate_errors[3], x.std(axis=0, ddof=1) / np.sqrt(12), rtol=1e-12)
    assert "bootstrap replicates" in repr(res)


def test_weights_resample_groups_and_perms():
    p, g = 6, 3
    data = small(p)
    labels = np.array([-1, 0, 1, 2, 0, 1])
    perms = np.array(list(itertools.permutations(range(g))), dtype=np.int32)
    eng = NumpyEngine()
    res = ls_spa_bootstrap_sampled(*data, n_boot=4, perms=perms, antithetical=False, groups=labels, _engine=eng)
    assert isinstance(res, SampledBootstrapGroupResults) and res.replicates.shape == (4, g) and res.n_samples == 6
    assert "players" in eng.calls and ("orderings", 6, False) in eng.calls and res.theta.shape == (p,)
    assert res.baseline_r_squared_replicates.shape == (4,) and res.baseline_r_squared > 0
    assert np.abs(res.replicates.sum(axis=1) - (res.r_squared_replicates - res.baseline_r_squared_replicates)).max() <= 1e-10
    # all orderings of the groups: the exact Shapley value of the grouped game of every replicate
    want = hp_ref.Problem(*eng._rows(42, 1, None, None)).shapley(labels)
    np.testing.assert_allclose(res.replicates[1], want, rtol=0, atol=1e-10)
    # a side that is not resampled gets ones; the caller's weights go through
    eng = NumpyEngine()
    ls_spa_bootstrap_sampled(*data, n_boot=3, n_samples=4, resample="train", _engine=eng)
    run = [c for c in eng.calls if isinstance(c, tuple) and c[0] == "run"]
    assert run == [("run", 3, 42, 0, False, True)]
    w = np.ones((3, 60))
    eng = NumpyEngine()
    ls_spa_bootstrap_sampled(*data, n_boot=3, n_samples=4, weights=(w, None), boot_seed=9, _engine=eng)
    assert [c for c in eng.calls if isinstance(c, tuple) and c[0] == "run"] == [("run", 3, 9, 0, True, False)]


def test_failed_replicates_are_nan_counted_warned_about_and_half_of_them_is_an_error():
    data = small()
    eng = NumpyEngine(fail={2})
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        res = ls_spa_bootstrap_sampled(*data, n_boot=6, n_samples=4, _engine=eng)
    assert [w.category for w in caught] == [RuntimeWarning] and "1 of 6" in str(caught[0].message)
    assert res.n_failed == 1 and np.isnan(res.replicates[2]).all() and np.isnan(res.replicate_errors[2]).all()
    assert np.isnan(res.r_squared_replicates[2]) and np.isfinite(np.delete(res.replicates, 2, axis=0)).all()
    ok = np.delete(res.replicates, 2, axis=0)
    np.testing.assert_array_equal(res.std_error, ok.std(axis=0, ddof=1))
    with pytest.raises(RuntimeError, match="4 of 6"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ls_spa_bootstrap_sampled(*data, n_boot=6, n_samples=4, _engine=NumpyEngine(fail={0, 1, 2, 3}))


def test_every_refusal_comes_before_any_engine_call():
    p = 6
    Xa, Xe, ya, ye = small(p)
    wide = hp_ref.gen(128, 130, 130, 1e1, 1)
    bad = [
        (dict(), (Xa, Xe, ya[:-1], ye), SizeIncompatible, None),
        (dict(), wide, ValueError, "at most p = 127"),
        (dict(), (Xa[:5], Xe, ya[:5], ye), ValueError, "at least p = 6 rows"),
        (dict(), (Xa, Xe[:5], ya, ye[:5]), ValueError, "at least p = 6 rows"),
        (dict(n_boot=1), None, ValueError, "n_boot"),
        (dict(n_samples=1), None, ValueError, "n_samples"),
        (dict(perms=np.array([[0, 1, 2, 3, 4, 5]] * 2), method="argsort"), None, ValueError, "either perms= or method="),
        (dict(method="nothing"), None, ValueError, "method must be"),
        (dict(groups=[0, 1, 2, 3, 4]), None, ValueError, None),
        (dict(groups=[0, 0, 0, 2, 2, 2]), None, ValueError, None),
        (dict(weights=(np.ones((3, 60)), None)), None, ValueError, "w_train"),
        (dict(weights=(-np.ones((200, 60)), None)), None, ValueError, "w_train"),
        (dict(resample="both"), None, ValueError, "resample"),
        (dict(confidence=1.0), None, ValueError, "confidence"),
        (dict(), (Xa, Xe, ya, np.zeros_like(ye)), ValueError, "identically zero"),
    ]
    for kwargs, data, exc, match in bad:
        eng = NumpyEngine()
        with pytest.raises(exc, match=match):
            ls_spa_bootstrap_sampled(*(data or (Xa, Xe, ya, ye)), _engine=eng, **kwargs)
        assert eng.calls == [], (kwargs, eng.calls)


# ---- the truth helper ------------------------------------------------------------------------------------------------------
def test_truth_helper_against_hp_ref_at_p_6():
    p = 6
    data = small(p, 77)
    orders = hp_ref.orderings(p, 77)
    # the point problem is hp_ref's own problem; a replicate is that of the drawn rows, whatever their order
    P = ref.problem(data, 3, -1)
    np.testing.assert_array_equal(ref.truth_lifts(P, orders, True), hp_ref.Problem(*data).lifts(orders, True))
    ia, ie = boot_ref.indices(3, 4, 0, 60), boot_ref.indices(3, 4, 1, 50)
    Q = hp_ref.Problem(data[0][np.sort(ia)], data[1][np.sort(ie)], data[2][np.sort(ia)], data[3][np.sort(ie)])
    np.testing.assert_allclose(ref.truth_lifts(ref.problem(data, 3, 4), orders, False), Q.lifts(orders, False), rtol=0,
                               atol=1e-15)
    # the weighted Grams with the counts as weights are the replicate's problem
    G, g, H, h, inv_yy = ref.weighted_problem(data, boot_ref.counts(3, 4, 0, 60), boot_ref.counts(3, 4, 1, 50), 0.5)
    R = ref.problem(data, 3, 4, 0.5)
    for got, want in ((G, R.G), (g, R.g), (H, R.H), (h, R.h)):
        np.testing.assert_allclose(got, R.to_float(want), rtol=0, atol=1e-13 * np.abs(got).max())
    assert abs(inv_yy * float(R.yy) - 1) <= 1e-14
    # plain lifts sit within round-off of the truth on this well-conditioned case; all orderings give the Shapley value
    np.testing.assert_allclose(ref.plain_lifts(data, 3, 4, 0.0, orders, True),
                               ref.truth_lifts(ref.problem(data, 3, 4), orders, True), rtol=0, atol=1e-12)
    allp = np.array(list(itertools.permutations(range(p))), dtype=np.int32)
    np.testing.assert_allclose(ref.truth_lifts(ref.problem(data, 3, 4), allp, False).mean(axis=0),
                               ref.problem(data, 3, 4).shapley(), rtol=0, atol=1e-12)
    # the statistics helper: one launch is Welford, several merge to the same moments
    x = np.random.default_rng(0).standard_normal((37, 3))
    for cut in (37, 16, 5):
        mean, m2 = ref.welford(x, cut)
        np.testing.assert_allclose(mean, x.mean(axis=0), rtol=0, atol=1e-15)
        np.testing.assert_allclose(m2, ((x - x.mean(axis=0)) ** 2).sum(axis=0), rtol=1e-13)
    lab = np.array([0, -1, 1, 0, 1, 1])
    np.testing.assert_array_equal(ref.group_fold(np.arange(12.0).reshape(2, 6), lab), [[3.0, 11.0], [15.0, 29.0]])
