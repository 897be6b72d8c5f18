"""ls_spa_best_subsets: the best subset of every size by out-of-sample R^2 -- CPU side.

The brute-force truth of tests/best_ref.py vetted on the reference's exact fixtures; the gap between best and runner-up
of every case the GPU tests compare with that truth (no GPU assertion then meets a near-tie); and the driver's plumbing
through a NumPy double of the engine whose enumeration is that truth."""
import warnings

import numpy as np
import pytest

import best_ref as B
from ls_spa import BestSubsetsResults, SizeIncompatible, _driver, ls_spa, ls_spa_best_subsets
from oracle_engine import OracleEngine
from test_subsets_host import SubsetsOracleEngine, data, golden, gram_problem, subset_values


# ---- the truth ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["toy", "exact_p4", "exact_p8"])
def test_truth_on_the_reference_fixtures(name):
    g = golden(name)
    d = [g[k] for k in ("X_train", "X_test", "y_train", "y_test")]
    p = d[0].shape[1]
    v = B.all_values(d)
    best, masks, found, runner = B.best_truth(v, p)
    assert found.all() and best[0] == 0.0 and masks[0] == 0
    assert abs(best[p] - float(g["r_squared"])) < 1e-12 and masks[p] == (1 << p) - 1
    assert runner[0] == runner[p] == -np.inf and (runner[1:p] <= best[1:p]).all()
    # long double and the fp64 oracle agree on every value
    np.testing.assert_allclose(v, subset_values(*gram_problem(*d), np.arange(1 << p, dtype=np.uint64)), rtol=0,
                               atol=1e-12)


def test_truth_tie_rule_and_include():
    v = np.array([0.0, 0.5, 0.5, 0.2, 0.5, 0.7, 0.7, 0.1])          # p = 3
    best, masks, found, runner = B.best_truth(v, 3)
    assert list(masks) == [0, 1, 5, 7] and list(best) == [0.0, 0.5, 0.7, 0.1]
    assert runner[1] == 0.5 and runner[2] == 0.7
    best, masks, found, _ = B.best_truth(v, 3, include=0b010)
    assert list(found) == [False, True, True, True] and list(masks) == [0, 2, 6, 7] and np.isnan(best[0])


CASES = [(p, reg) for p in B.BRUTE_P for reg in B.BRUTE_REG] + [("edge", 0.0)]


@pytest.mark.parametrize("p, reg", CASES)
def test_every_gpu_case_has_a_clear_winner(p, reg):
    d, v = B.brute_case(p, reg)
    n = d[0].shape[1]
    includes = [0]
    if p in B.INCLUDE_P and reg == 0.0:
        includes += [B.mask_of(s) for s in B.include_sets(n)]
    for inc in includes:
        best, _, found, runner = B.best_truth(v, n, inc)
        assert found[bin(inc).count("1"):].all() and not found[:bin(inc).count("1")].any()
        assert ((best - runner)[found] > B.MIN_GAP).all(), (p, reg, inc, (best - runner)[found].min())


# ---- driver plumbing on a test double -----------------------------------------------------------------------------------
class BestOracleEngine(OracleEngine):
    """OracleEngine with the best-subsets entry point, computed by the brute-force truth.  info: the info word it
    reports; drop: sizes it reports as not found; values: v of every mask instead of the oracle's."""

    def __init__(self, info=0, drop=(), values=None):
        super().__init__()
        self.best_calls, self.touched = [], 0
        self._info, self._drop, self._values = info, tuple(drop), values

    def load_data(self, *a):
        self.touched += 1
        super().load_data(*a)

    def subsets_best(self, include=0):
        self.best_calls.append(include)
        G, g, H, h = self.gram()
        p = self.p
        v = self._values
        if v is None:
            v = subset_values(G, g, H, h, self.y_norm_sq, np.arange(1 << p, dtype=np.uint64))
        best, masks, found, _ = B.best_truth(np.asarray(v, dtype=np.float64), p, include)
        for k in self._drop:
            best[k], masks[k], found[k] = np.nan, 0, False
        return best, masks, found, self._info


def test_result_shapes_and_fields():
    p = 7
    d = data(p, seed=3)
    eng = BestOracleEngine()
    res = ls_spa_best_subsets(*d, _engine=eng)
    assert isinstance(res, BestSubsetsResults) and eng.best_calls == [0]
    assert res.sizes.tolist() == list(range(p + 1))
    assert res.subsets.shape == (p + 1, p) and res.subsets.dtype == bool
    assert res.r_squared.shape == (p + 1,) and res.theta.shape == (p + 1, p)
    assert res.subsets.sum(axis=1).tolist() == list(range(p + 1))
    v = subset_values(*eng.gram(), eng.y_norm_sq, np.arange(1 << p, dtype=np.uint64))     # the double's own problem
    best, masks, _, _ = B.best_truth(v, p)
    np.testing.assert_array_equal(res.r_squared, best)
    np.testing.assert_allclose(v, subset_values(*gram_problem(*d), np.arange(1 << p, dtype=np.uint64)), rtol=0,
                               atol=1e-12)
    for i in range(p + 1):
        assert B.mask_of(np.nonzero(res.subsets[i])[0]) == masks[i]
    assert res.best_size == int(np.argmax(best))
    np.testing.assert_array_equal(res.best_subset, res.subsets[res.best_size])
    full = ls_spa(*d, method="subsets", _engine=SubsetsOracleEngine())
    assert res.full_r_squared == full.r_squared
    np.testing.assert_allclose(res.theta[p], full.theta, rtol=1e-9, atol=1e-12)
    assert "Best model" in repr(res)


def test_theta_is_the_refit_with_exact_zeros():
    p = 8
    d = data(p, seed=5)
    res = ls_spa_best_subsets(*d, reg=0.05, _engine=BestOracleEngine())
    G, g, H, h, yy = gram_problem(*d, reg=0.05)
    for i in range(p + 1):
        cols = np.nonzero(res.subsets[i])[0]
        out = np.nonzero(~res.subsets[i])[0]
        assert (res.theta[i, out] == 0.0).all() and not np.signbit(res.theta[i, out]).any()
        if len(cols):
            th = np.linalg.solve(G[np.ix_(cols, cols)], g[cols])
            np.testing.assert_allclose(res.theta[i, cols], th, rtol=1e-9, atol=1e-12)
            r2 = (2.0 * th @ h[cols] - th @ H[np.ix_(cols, cols)] @ th) / yy
            assert abs(r2 - res.r_squared[i]) < 1e-12


@pytest.mark.parametrize("make", [lambda: [2], lambda: (5, 0), lambda: np.array([1, 3, 4]), lambda: range(6),
                                  lambda: iter([3]), lambda: {4, 2}])
def test_include(make):
    p = 6
    d = data(p, seed=8)
    cols, include = sorted(int(j) for j in make()), make()
    eng = BestOracleEngine()
    res = ls_spa_best_subsets(*d, include=include, _engine=eng)
    assert eng.best_calls == [B.mask_of(cols)]
    assert res.sizes.tolist() == list(range(len(cols), p + 1))
    assert res.subsets[:, cols].all() and res.subsets.sum(axis=1).tolist() == res.sizes.tolist()
    v = subset_values(*eng.gram(), eng.y_norm_sq, np.arange(1 << p, dtype=np.uint64))
    best, _, _, _ = B.best_truth(v, p, B.mask_of(cols))
    np.testing.assert_array_equal(res.r_squared, best[len(cols):])
    assert not np.isnan(res.r_squared).any()


def test_best_size_takes_the_smallest_of_equal_maxima_and_skips_nan():
    p = 3
    d = data(p, seed=2)
    v = np.array([0.0, 0.6, 0.1, 0.6, 0.2, 0.3, 0.1, 0.9])         # sizes: 0 | 0.6 | 0.6 | 0.9
    res = ls_spa_best_subsets(*d, _engine=BestOracleEngine(values=v))
    assert res.best_size == 3
    with pytest.warns(RuntimeWarning, match="not numerically positive definite"):
        res = ls_spa_best_subsets(*d, _engine=BestOracleEngine(values=v, drop=(3,), info=1))
    assert res.best_size == 1 and res.best_subset.tolist() == [True, False, False]        # size 1 before size 2
    assert np.isnan(res.r_squared[3]) and np.isnan(res.theta[3]).all() and not res.subsets[3].any()
    assert res.r_squared[:3].tolist() == [0.0, 0.6, 0.6]
    with pytest.warns(RuntimeWarning):
        res = ls_spa_best_subsets(*d, include=[0, 1, 2], _engine=BestOracleEngine(values=v, drop=(3,), info=1))
    assert res.best_size == -1 and not res.best_subset.any() and res.sizes.tolist() == [3]


def test_not_positive_definite_warns_and_names_this_file():
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        ls_spa_best_subsets(*data(5, seed=2), _engine=BestOracleEngine(info=1))
    assert len(seen) == 1 and issubclass(seen[0].category, RuntimeWarning)
    assert "not numerically positive definite" in str(seen[0].message) and seen[0].filename == __file__


def test_no_warning_without_the_info_bit():
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ls_spa_best_subsets(*data(5, seed=2), _engine=BestOracleEngine())


def _zero_y(d):
    return d[0], d[1], d[2], np.zeros_like(d[3])


@pytest.mark.parametrize("make, kw, error, text", [
    (lambda: data(33, n=80, m=50, seed=1), {}, ValueError, "at most p = 32"),
    (lambda: data(6), dict(include=[6]), ValueError, "outside 0 .. 5"),
    (lambda: data(6), dict(include=[-1]), ValueError, "outside 0 .. 5"),
    (lambda: data(6), dict(include=[1, 4, 1]), ValueError, "twice"),
    (lambda: data(6), dict(include=[1.5]), ValueError, "integer column indices"),
    (lambda: data(6), dict(include=[True, False]), ValueError, "integer column indices"),
    (lambda: data(6), dict(include=3), ValueError, "iterable of column indices"),
    (lambda: data(6), dict(include="01"), ValueError, "iterable of column indices"),
    (lambda: _zero_y(data(6)), {}, ValueError, "identically zero"),
    (lambda: (data(6)[0], data(5)[1]) + data(6)[2:], {}, SizeIncompatible, None),
    (lambda: (data(6)[0][:-1],) + data(6)[1:], {}, SizeIncompatible, None),
    (lambda: data(6)[:2] + (data(6)[2][:, None], data(6)[3]), {}, (ValueError, SizeIncompatible), None),
])
def test_refusals_come_before_any_engine_work(monkeypatch, make, kw, error, text):
    def no_engine(*a, **k):
        raise AssertionError("an engine was acquired")
    monkeypatch.setattr(_driver, "_acquire_engine", no_engine)
    eng = BestOracleEngine()
    with pytest.raises(error, match=text):
        ls_spa_best_subsets(*make(), _engine=eng, **kw)
    assert eng.touched == 0 and eng.best_calls == []
    with pytest.raises(error, match=text):
        ls_spa_best_subsets(*make(), **kw)          # no engine of the caller's: none is acquired either


def test_kept_engine_back_to_float64():
    class Float32Engine(BestOracleEngine):
        precision = "float32"

        def set_precision(self, dtype):
            self.precision = np.dtype(dtype).name

        def full_fit(self):
            assert self.precision == "float64", "full fit with fp32 factorisation"
            return super().full_fit()

    eng = Float32Engine()
    ls_spa_best_subsets(*data(6, seed=3), _engine=eng)
    assert eng.precision == "float64"


def test_the_callers_engine_is_left_open_and_a_kept_one_is_reset(monkeypatch):
    import threading
    log = []

    class Kept(BestOracleEngine):
        def set_flags(self, flags):
            log.append(("set_flags", flags))

        def history_enable(self, n):
            log.append(("history_enable", n))

        def close(self):
            log.append(("close",))

    kept = Kept()
    lock = threading.Lock()
    lock.acquire()
    monkeypatch.setattr(_driver, "_acquire_engine", lambda device: (kept, lock))
    res = ls_spa_best_subsets(*data(5, seed=4))
    assert res.best_size >= 0 and log == [("set_flags", 0), ("history_enable", 0)] and not lock.locked()
    own = Kept()
    ls_spa_best_subsets(*data(5, seed=4), _engine=own)
    assert log == [("set_flags", 0), ("history_enable", 0)]          # the caller's engine: nothing reset, nothing closed
