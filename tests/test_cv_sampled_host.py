"""ls_spa_cv_sampled without a GPU: the driver through a NumPy double of the engine's cv_lift_* methods (sources, perms,
the groups' expansion, the stop rule, n_samples, result shapes, the refusals in their order before any engine call),
lsspa_debug_cv_lift_plan at its edges, and the truth of tests/cv_sampled_ref.py against a brute-force Shapley value of
the CV game."""
import math

import numpy as np
import pytest

import cv_sampled_ref as ref
import hp_ref
from ls_spa import SampledCVGroupResults, SampledCVResults, SizeIncompatible, ls_spa_cv_sampled
from ls_spa._engine import debug_cv_lift_plan, debug_expand_groups


class NumpyEngine:
    """cv_lift_* in NumPy: lifts by hp_ref.plain_lifts per fold, Welford replaced by the plain moments of all samples."""

    def __init__(self):
        self.calls, self.labels, self.samples = [], None, []

    def cv_lift_load(self, X, y, ids, K, reg):
        self.calls.append("load")
        self.X, self.y, self.ids, self.K, self.reg = np.asarray(X, float), np.asarray(y, float), np.asarray(ids), K, reg
        self.p = self.X.shape[1]

    def cv_lift_set_players(self, labels):
        self.calls.append("players")
        self.labels = np.asarray(labels)

    def cv_lift_batch(self, perms, antithetical, want_lifts=False, accumulate=True):
        self.calls.append(("batch", len(perms), bool(antithetical)))
        perms = np.asarray(perms)
        if self.labels is None:
            fold, _ = ref.plain_lifts(self.X, self.y, self.ids, self.K, self.reg, perms, antithetical)
        else:
            rows = debug_expand_groups(self.labels, perms, False)      # each group's columns ascending, in both rows
            if antithetical:
                rev = debug_expand_groups(self.labels, np.ascontiguousarray(perms[:, ::-1]), False)
                rows = np.stack([rows, rev], axis=1).reshape(2 * len(perms), -1)
            col, _ = ref.plain_lifts(self.X, self.y, self.ids, self.K, self.reg, rows, False)
            fold = ref.group_fold(col, self.labels)
            if antithetical:
                fold = 0.5 * fold[0::2] + 0.5 * fold[1::2]
        self.samples.extend(np.concatenate([f, f.sum(axis=0)[None]]) for f in fold)

    def cv_lift_get(self):
        x = np.array(self.samples)
        mean = x.mean(axis=0)
        return len(x), mean, ((x - mean) ** 2).sum(axis=0)

    def cv_lift_info(self):
        return np.zeros(self.K, dtype=np.int32)

    def cv_lift_problem(self, f):
        tr, te = self.ids != f, self.ids == f
        G, g, H, h, _ = hp_ref.plain_gram(self.X[tr], self.X[te], self.y[tr], self.y[te], self.reg)
        return G, g, H, h, 1.0 / float(self.y @ self.y)

    def cv_lift_free(self):
        self.calls.append("free")


def data(p, K, seed, extra=0):
    n = K * (2 * p + 6) + 1 + extra
    Xa, _, ya, _ = hp_ref.gen(p, n, 1, 1e1, seed)
    return Xa, ya


def test_all_orderings_give_the_brute_force_shapley_value_of_the_cv_game():
    p, K = 5, 3
    Xa, ya = data(p, K, 55)
    eng = NumpyEngine()
    res = ls_spa_cv_sampled(Xa, ya, 0.0, K, method="exact", antithetical=False, max_samples=1000, shuffle=False,
                            _engine=eng)
    assert isinstance(res, SampledCVResults) and res.n_samples == math.factorial(p)
    ids = np.arange(len(ya)) % K
    np.testing.assert_array_equal(res.fold_ids, ids)
    probs, scale = ref.fold_problems(Xa, ya, ids, K)
    phi = np.asarray(ref.brute_shapley(probs, scale, p), dtype=np.float64)
    np.testing.assert_allclose(res.attribution, phi, rtol=0, atol=1e-10)
    # the truth module's lifts average to the same value
    import itertools
    orders = np.array(list(itertools.permutations(range(p))), dtype=np.int32)
    fold, tot = ref.truth_lifts(probs, scale, orders, False)
    np.testing.assert_allclose(tot.mean(axis=0), phi, rtol=0, atol=1e-13)
    np.testing.assert_allclose(fold.sum(axis=1), tot, rtol=0, atol=1e-15)
    assert res.attribution.shape == (p,) and res.fold_attribution.shape == (K, p)
    assert res.attribution_errors.shape == (p,) and res.fold_attribution_errors.shape == (K, p)
    assert res.fold_r_squared.shape == (K,) and res.theta.shape == (p,)
    assert abs(res.attribution.sum() - res.r_squared) <= 1e-10
    np.testing.assert_allclose(res.fold_attribution.sum(axis=0), res.attribution, rtol=0, atol=1e-13)
    assert eng.calls[0] == "load" and eng.calls[-1] == "free" and "players" not in eng.calls


def test_sources_perms_batches_and_the_stop_rule():
    p, K = 6, 2
    Xa, ya = data(p, K, 66)
    eng = NumpyEngine()
    res = ls_spa_cv_sampled(Xa, ya, 0.0, K, max_samples=20, batch_size=8, _engine=eng)
    assert res.n_samples == 20
    assert [c for c in eng.calls if isinstance(c, tuple)] == [("batch", 8, True), ("batch", 8, True), ("batch", 4, True)]
    rng = np.random.default_rng(0)
    perms = np.array([rng.permutation(p) for _ in range(5)])
    eng = NumpyEngine()
    res = ls_spa_cv_sampled(Xa, ya, 0.0, K, perms=perms, antithetical=False, batch_size=2, _engine=eng)
    assert res.n_samples == 5
    fold, tot = ref.plain_lifts(Xa, ya, res.fold_ids, K, 0.0, perms, False)
    np.testing.assert_allclose(res.attribution, tot.mean(axis=0), rtol=0, atol=1e-13)
    np.testing.assert_allclose(res.fold_attribution, fold.mean(axis=0), rtol=0, atol=1e-13)
    # the stop rule looks at the summed attribution's errors after the first batch with n >= 2
    eng = NumpyEngine()
    res = ls_spa_cv_sampled(Xa, ya, 0.0, K, max_samples=64, batch_size=4, tolerance=10.0, _engine=eng)
    assert res.n_samples == 4 and res.attribution_errors.max() <= 10.0
    eng = NumpyEngine()
    res = ls_spa_cv_sampled(Xa, ya, 0.0, K, max_samples=24, batch_size=8, tolerance=0.0, _engine=eng)
    assert res.n_samples == 24
    with pytest.raises(ValueError, match="perms is empty"):
        ls_spa_cv_sampled(Xa, ya, 0.0, K, perms=np.zeros((0, p), dtype=int), _engine=NumpyEngine())


def test_groups_run_in_dimension_g():
    p, K = 7, 2
    labels = np.array([-1, 0, 1, 2, 0, 1, 2])
    Xa, ya = data(p, K, 77)
    eng = NumpyEngine()
    res = ls_spa_cv_sampled(Xa, ya, 0.0, K, groups=labels, method="exact", antithetical=False, _engine=eng)
    assert isinstance(res, SampledCVGroupResults) and res.n_samples == 6
    assert res.attribution.shape == (3,) and res.fold_attribution.shape == (K, 3) and res.theta.shape == (p,)
    assert eng.calls[:2] == ["load", "players"]
    probs, scale = ref.fold_problems(Xa, ya, res.fold_ids, K)
    full = float(ref.cv_value(probs, scale, list(range(p))))
    base = float(ref.cv_value(probs, scale, [0]))
    assert abs(res.r_squared - full) <= 1e-10 and abs(res.baseline_r_squared - base) <= 1e-10
    assert abs(res.attribution.sum() - (full - base)) <= 1e-10
    assert res.fold_baseline_r_squared.shape == (K,)
    # group orderings as perms, antithetical: the baseline first in both rows
    eng = NumpyEngine()
    res2 = ls_spa_cv_sampled(Xa, ya, 0.0, K, groups=labels, perms=np.array([[2, 0, 1]]), antithetical=True, _engine=eng)
    rows = debug_expand_groups(labels, np.array([[2, 0, 1]]), True)
    assert rows[0][0] == 0 and rows[1][0] == 0 and res2.n_samples == 1
    assert np.isinf(res2.attribution_errors).all()


def test_refusals_come_before_any_engine_call_in_their_order():
    eng = NumpyEngine()
    X, y = np.ones((40, 3)), np.arange(40.0)
    bad = [
        (ValueError, "two-dimensional", dict(X=np.ones(5), y=np.ones(5))),
        (SizeIncompatible, "rows", dict(X=np.ones((5, 2)), y=np.ones(4))),
        (ValueError, "at most p = 127", dict(X=np.ones((300, 128)), y=np.ones(300))),
        (ValueError, "2 .. 32 folds", dict(X=X, y=y, folds=1)),
        (ValueError, "2 .. 32 folds", dict(X=X, y=y, folds=33)),
        (ValueError, "0 .. K-1", dict(X=X, y=y, folds=np.r_[np.full(20, -1), np.ones(20, dtype=int)])),
        (ValueError, "is empty", dict(X=X, y=y, folds=np.r_[np.zeros(20, dtype=int), np.full(20, 2)])),
        (ValueError, "fold 1 of 2 has 2 rows, fewer than p = 3", dict(X=X, y=y, folds=np.r_[np.zeros(38, dtype=int), 1, 1])),
        (ValueError, "identically zero", dict(X=X, y=np.zeros(40))),
        (ValueError, "one label per column", dict(X=X, y=y, groups=[0, 1])),
        (ValueError, "gap in its numbering", dict(X=X, y=y, groups=[0, 2, 2])),
        (ValueError, "either perms= or method=", dict(X=X, y=y, perms=[[0, 1, 2]], method="argsort")),
        (ValueError, "method must be one of", dict(X=X, y=y, method="nope")),
        (ValueError, "must be positive", dict(X=X, y=y, batch_size=0)),
    ]
    for exc, match, kw in bad:
        kw = dict(kw)
        Xk, yk = kw.pop("X"), kw.pop("y")
        with pytest.raises(exc, match=match):
            ls_spa_cv_sampled(Xk, yk, 0.0, kw.pop("folds", 2), _engine=eng, **kw)
    assert eng.calls == []
    # the order: the column limit before the folds, the folds before y, y before the labels, the labels before perms
    with pytest.raises(ValueError, match="at most p = 127"):
        ls_spa_cv_sampled(np.ones((300, 128)), np.zeros(300), 0.0, 99, _engine=eng)
    with pytest.raises(ValueError, match="2 .. 32 folds"):
        ls_spa_cv_sampled(X, np.zeros(40), 0.0, 99, groups=[0], _engine=eng)
    with pytest.raises(ValueError, match="identically zero"):
        ls_spa_cv_sampled(X, np.zeros(40), 0.0, 2, groups=[0], _engine=eng)
    with pytest.raises(ValueError, match="one label per column"):
        ls_spa_cv_sampled(X, y, 0.0, 2, groups=[0], perms=[[0]], method="argsort", _engine=eng)
    assert eng.calls == []


def test_the_launch_plan_at_its_edges():
    P = debug_cv_lift_plan
    a, b, c = P(111, 111, 2, 256, True), P(112, 112, 2, 256, True), P(127, 127, 2, 256, True)
    assert (a["nb"], a["form"], a["workgroup"]) == (7, 0, 128)
    assert (b["nb"], b["form"], b["workgroup"]) == (8, 1, 512) and (c["nb"], c["form"]) == (8, 1)
    assert a["lds_bytes"] <= 80 * 1024 and b["lds_bytes"] <= 160 * 1024      # two workgroups a CU; one
    for plan in (a, b, c):
        assert plan["workgroups_per_sample"] == 4 and plan["samples_per_launch"] == 256 and plan["launches"] == 1
    assert P(40, 40, 32, 256, True)["workgroups_per_sample"] == 64 and P(40, 40, 32, 256, False)["workgroups_per_sample"] == 32
    # the cut: whole samples, at most 2^16 workgroups (2^13 of the LDS form) and 256 MB of raw lifts a launch
    for p, K, anti in ((9, 3, True), (40, 32, True), (111, 2, False), (112, 2, True), (127, 32, True)):
        S = P(p, p, K, 1 << 22, anti)["samples_per_launch"]
        per = 2 if anti else 1
        cap = 1 << 13 if p + 1 > 112 else 1 << 16
        assert S == max(1, min(cap // (per * K), (256 << 20) // 8 // (per * K * p)))
        assert S * per * K <= cap and S * per * K * p * 8 <= 256 << 20
        two = P(p, p, K, S + 1, anti)
        assert two["launches"] == 2 and two["samples_per_launch"] == S
        assert P(p, p, K, S, anti)["launches"] == 1
    # d does not move the cut (the raw lifts are p wide)
    assert P(112, 5, 2, 5000, True) == P(112, 112, 2, 5000, True)
    for args in ((128, 128, 2, 1, 0), (0, 0, 2, 1, 0), (9, 10, 2, 1, 0), (9, 9, 1, 1, 0), (9, 9, 33, 1, 0), (9, 9, 2, 0, 0)):
        with pytest.raises(ValueError):
            P(*args)
