"""ls_spa_multi_sampled: the sampled attribution of many responses on one design matrix -- CPU side.

The driver's argument errors, all raised before an engine exists, and its result contract, stop rule, sum check and
lifecycle through a test double of the engine whose lift vectors are hp_ref.plain_lifts per response."""
from itertools import permutations

import numpy as np
import pytest

import hp_ref
from ls_spa import SampledMultiResults, SizeIncompatible, _driver, ls_spa_multi_sampled
from ls_spa._native import LSSPANativeError
from test_multi_host import multi_data, multi_fit, multi_gram_problem, multi_oracle
from test_subsets_host import data


class MultiLiftOracleEngine:
    """What ls_spa_multi_sampled asks of an engine, computed with NumPy: Welford statistics of plain_lifts."""

    def __init__(self, info=0, drop=False):
        self.calls, self._info, self._drop = [], info, drop

    def multi_lift_load(self, Xa, Xe, Ya, Ye, reg):
        self.calls.append("load")
        self._d, self._reg = (Xa, Xe, Ya, Ye), reg
        self._x = []

    def multi_lift_batch(self, perms, antithetical, want_lifts=False, accumulate=True):
        self.calls.append(("batch", len(perms), bool(antithetical)))
        Xa, Xe, Ya, Ye = self._d
        out = np.stack([hp_ref.plain_lifts(Xa, Xe, Ya[:, r], Ye[:, r], self._reg, perms, antithetical)
                        for r in range(Ya.shape[1])], axis=1)                  # [B][m][p]
        if self._drop:
            out[0, -1, 0] = 0.0          # one lift of the last response lost
        if accumulate:
            self._x.extend(out)
        return out if want_lifts else None

    def multi_lift_get(self):
        self.calls.append("get")
        x = np.array(self._x)
        mean = x.mean(axis=0)
        return len(x), mean, ((x - mean) ** 2).sum(axis=0)

    def multi_lift_info(self):
        return self._info

    def multi_lift_gram(self):
        return multi_gram_problem(*self._d, self._reg)

    def multi_lift_free(self):
        self.calls.append("free")


def batches(eng):
    return [c for c in eng.calls if isinstance(c, tuple)]


# ---- argument errors: all before an engine exists ------------------------------------------------------------------
@pytest.fixture
def no_engine(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("an engine was acquired")
    monkeypatch.setattr(_driver, "_acquire_engine", refuse)


def _shapes(n=30, rows=20, p=4, m=3, p_test=None, n_y=None, rows_y=None, m_test=None):
    z = np.zeros
    return (z((n, p)), z((rows, p if p_test is None else p_test)), z((n if n_y is None else n_y, m)),
            z((rows if rows_y is None else rows_y, m if m_test is None else m_test)))


@pytest.mark.parametrize("kw, text", [
    (dict(p_test=5), "same number of columns"),
    (dict(n_y=29), "X_train should have the same number of rows"),
    (dict(rows_y=21), "X_test should have the same number of rows"),
    (dict(m_test=2), "Y_train and Y_test should have the same number of columns"),
    (dict(n=3), "at most the number of observations"),
])
def test_mismatched_shapes_raise_size_incompatible(no_engine, kw, text):
    with pytest.raises(SizeIncompatible, match=text):
        ls_spa_multi_sampled(*_shapes(**kw))


def test_p105_is_refused_naming_the_limit(no_engine):
    with pytest.raises(ValueError, match="at most p = 104"):
        ls_spa_multi_sampled(*_shapes(n=200, rows=150, p=105))
    assert _driver.MULTI_LIFT_MAX_P == 104


def test_fewer_test_rows_than_features_are_refused_naming_the_limit(no_engine):
    with pytest.raises(ValueError, match="M >= p test rows \\(M = 9, p = 10\\)"):
        ls_spa_multi_sampled(*_shapes(n=40, rows=9, p=10))


def test_too_many_columns_are_refused_naming_the_limit(no_engine):
    with pytest.raises(ValueError, match="p \\+ m <= 32767"):
        ls_spa_multi_sampled(*_shapes(p=4, m=32764))


@pytest.mark.parametrize("bad", ["X_train 1-D", "Y 3-D", "no responses"])
def test_malformed_arrays_are_refused(no_engine, bad):
    Xa, Xe, Ya, Ye = _shapes()
    if bad == "X_train 1-D":
        Xa = Xa[:, 0]
    elif bad == "Y 3-D":
        Ya, Ye = Ya[:, :, None], Ye[:, :, None]
    else:
        Ya, Ye = Ya[:, :0], Ye[:, :0]
    with pytest.raises(ValueError):
        ls_spa_multi_sampled(Xa, Xe, Ya, Ye)


def test_perms_together_with_a_method_is_refused(no_engine):
    d = multi_data(5, 2, seed=1)
    with pytest.raises(ValueError, match="either perms= or method="):
        ls_spa_multi_sampled(*d, perms=[np.arange(5)], method="argsort")
    with pytest.raises(ValueError, match="method must be one of"):
        ls_spa_multi_sampled(*d, method="subsets")
    with pytest.raises(ValueError, match="must be positive"):
        ls_spa_multi_sampled(*d, batch_size=0)


# ---- the result contract through the test double ---------------------------------------------------------------------
@pytest.mark.parametrize("reg", [0.0, 0.1])
def test_fields_and_shapes(reg):
    p, m = 10, 4
    d = multi_data(p, m, seed=3)
    eng = MultiLiftOracleEngine()
    res = ls_spa_multi_sampled(*d, reg, max_samples=12, batch_size=5, _engine=eng)
    assert eng.calls[0] == "load" and eng.calls[-1] == "free"
    assert batches(eng) == [("batch", 5, True), ("batch", 5, True), ("batch", 2, True)]
    assert isinstance(res, SampledMultiResults)
    assert [f for f in res.__dataclass_fields__] == ["attribution", "attribution_errors", "theta", "r_squared",
                                                     "n_samples"]
    assert res.attribution.shape == (m, p) and res.attribution_errors.shape == (m, p)
    assert res.theta.shape == (m, p) and res.r_squared.shape == (m,) and res.n_samples == 12
    theta, r2 = multi_fit(*d, reg=reg)
    np.testing.assert_allclose(res.theta, theta, rtol=0, atol=1e-12)
    np.testing.assert_allclose(res.r_squared, r2, rtol=0, atol=1e-12)
    np.testing.assert_allclose(res.attribution.sum(axis=1), res.r_squared, rtol=0, atol=1e-11)
    n, mean, m2 = eng.multi_lift_get()
    np.testing.assert_array_equal(res.attribution, mean)
    np.testing.assert_allclose(res.attribution_errors, np.sqrt(m2 / (12 * 11)), rtol=1e-15, atol=0)
    assert "m = 4 responses, 12 samples" in repr(res)


def test_one_dimensional_y_is_one_response():
    Xa, Xe, ya, ye = data(4, seed=6)
    res = ls_spa_multi_sampled(Xa, Xe, ya, ye, method="exact", _engine=MultiLiftOracleEngine())
    assert res.attribution.shape == (1, 4) and res.r_squared.shape == (1,) and res.n_samples == 24


def test_one_sample_has_infinite_errors():
    d = multi_data(5, 2, seed=4)
    res = ls_spa_multi_sampled(*d, perms=[np.arange(5)], _engine=MultiLiftOracleEngine())
    assert res.n_samples == 1 and np.all(np.isinf(res.attribution_errors))


def test_all_orderings_give_the_exact_attribution():
    p, m = 4, 3
    d = multi_data(p, m, seed=11)
    eng = MultiLiftOracleEngine()
    res = ls_spa_multi_sampled(*d, method="exact", antithetical=False, _engine=eng)
    assert res.n_samples == 24 and batches(eng) == [("batch", 24, False)]
    np.testing.assert_allclose(res.attribution, multi_oracle(*d), rtol=0, atol=1e-12)
    by_hand = ls_spa_multi_sampled(*d, perms=list(permutations(range(p))), antithetical=False,
                                   _engine=MultiLiftOracleEngine())
    np.testing.assert_allclose(by_hand.attribution, res.attribution, rtol=0, atol=1e-14)


# ---- the stop rule -------------------------------------------------------------------------------------------------------
def test_a_generous_tolerance_stops_at_the_first_batch_with_two_samples():
    d = multi_data(10, 3, seed=5)
    eng = MultiLiftOracleEngine()
    res = ls_spa_multi_sampled(*d, max_samples=64, batch_size=4, tolerance=1e3, _engine=eng)
    assert res.n_samples == 4 and len(batches(eng)) == 1
    eng = MultiLiftOracleEngine()
    res = ls_spa_multi_sampled(*d, max_samples=64, batch_size=1, tolerance=1e3, _engine=eng)
    assert res.n_samples == 2 and len(batches(eng)) == 2             # one sample has no standard error yet
    assert np.all(np.isfinite(res.attribution_errors))


def test_no_tolerance_runs_to_max_samples():
    d = multi_data(10, 3, seed=5)
    eng = MultiLiftOracleEngine()
    res = ls_spa_multi_sampled(*d, max_samples=10, batch_size=4, _engine=eng)
    assert res.n_samples == 10 and [b[1] for b in batches(eng)] == [4, 4, 2]
    assert eng.calls.count("get") == 1                                 # the state is read once, at the end
    eng = MultiLiftOracleEngine()
    res = ls_spa_multi_sampled(*d, max_samples=10, batch_size=4, tolerance=0.0, _engine=eng)
    assert res.n_samples == 10                                         # a tolerance nobody meets: the same


# ---- the sum check and the lifecycle -----------------------------------------------------------------------------------
def test_a_dropped_lift_fails_the_sum_check_and_frees():
    eng = MultiLiftOracleEngine(drop=True)
    with pytest.raises(LSSPANativeError, match="did not sum to the R\\^2"):
        ls_spa_multi_sampled(*multi_data(10, 3, seed=7), max_samples=4, batch_size=4, _engine=eng)
    assert eng.calls[-1] == "free"


def test_not_positive_definite_warns_and_frees():
    eng = MultiLiftOracleEngine(info=1, drop=True)                     # with the flag the sums are not judged
    with pytest.warns(RuntimeWarning, match="not numerically positive definite"):
        ls_spa_multi_sampled(*multi_data(10, 2, seed=8), max_samples=4, batch_size=4, _engine=eng)
    assert eng.calls[-1] == "free"


def test_an_error_inside_the_loop_frees():
    class Failing(MultiLiftOracleEngine):
        def multi_lift_batch(self, *a, **k):
            raise LSSPANativeError("boom")
    eng = Failing()
    with pytest.raises(LSSPANativeError, match="boom"):
        ls_spa_multi_sampled(*multi_data(10, 2, seed=9), max_samples=4, _engine=eng)
    assert eng.calls == ["load", "free"]


def test_empty_perms_are_refused_and_free():
    eng = MultiLiftOracleEngine()
    with pytest.raises(ValueError, match="perms is empty"):
        ls_spa_multi_sampled(*multi_data(10, 2, seed=9), perms=[], _engine=eng)
    assert eng.calls[-1] == "free"
