"""ls_spa_multi_sampled(groups=): the sampled attribution of many responses over groups of columns -- CPU side.

The driver's label and limit errors, all raised before an engine exists, and its result contract, stop rule, sum check
and lifecycle through the NumPy double of tests/test_multi_sampled_host.py, extended by the player map: the group
orderings are expanded (baseline first, every group's columns ascending, the groups reversed for the second row of a
pair) and the column lifts folded per group."""
from itertools import permutations

import numpy as np
import pytest

import hp_ref
from ls_spa import SampledMultiGroupResults, SampledMultiResults, _driver, ls_spa_multi_sampled
from ls_spa._native import LSSPANativeError
from test_multi_host import multi_data, multi_fit
from test_multi_sampled_host import MultiLiftOracleEngine, batches


def expand(labels, gperm, reverse=False):
    labels = np.asarray(labels)
    order = list(gperm)[::-1] if reverse else list(gperm)
    return np.concatenate([np.nonzero(labels == -1)[0]] + [np.nonzero(labels == k)[0] for k in order]).astype(np.int32)


class GroupedOracleEngine(MultiLiftOracleEngine):
    """The double with multi_lift_set_players: a batch's group orderings are expanded and the column lifts folded."""

    def multi_lift_load(self, *a):
        super().multi_lift_load(*a)
        self._labels = None

    def multi_lift_set_players(self, labels):
        self.calls.append("players")
        self._labels, self._x = np.asarray(labels), []

    def multi_lift_batch(self, perms, antithetical, want_lifts=False, accumulate=True):
        if self._labels is None:
            return super().multi_lift_batch(perms, antithetical, want_lifts, accumulate)
        Xa, Xe, Ya, Ye = self._d
        lab, g = self._labels, int(self._labels.max()) + 1
        perms = np.asarray(perms)
        assert perms.shape[1] == g
        if not all(sorted(row) == list(range(g)) for row in perms.tolist()):       # as the library refuses it
            raise ValueError("lsspa: a row of perms is not a permutation of 0 .. g-1")
        self.calls.append(("batch", len(perms), bool(antithetical)))
        rows = [expand(lab, gp, rev) for gp in perms for rev in ((False, True) if antithetical else (False,))]
        col = np.stack([hp_ref.plain_lifts(Xa, Xe, Ya[:, r], Ye[:, r], self._reg, rows, False)
                        for r in range(Ya.shape[1])], axis=1)                 # [rows][m][p]
        fold = np.stack([col[:, :, lab == k].sum(axis=2) for k in range(g)], axis=2)
        out = 0.5 * (fold[0::2] + fold[1::2]) if antithetical else fold
        if self._drop:
            out[0, -1, 0] = 0.0
        if accumulate:
            self._x.extend(out)
        return out if want_lifts else None


LABELS = np.array([-1, 2, 0, 1, 2, 0, 1, 2, 0, -1], dtype=np.int32)      # p = 10, g = 3, a two-column baseline


@pytest.fixture
def no_engine(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("an engine was acquired")
    monkeypatch.setattr(_driver, "_acquire_engine", refuse)


# ---- label and limit errors: all before an engine exists -----------------------------------------------------------
@pytest.mark.parametrize("groups, text", [
    (np.zeros(9, dtype=np.int32), "one label per column"),
    (np.zeros(10), "integer labels"),
    (np.array([0, -2] + [0] * 8), "label below -1"),
    (np.full(10, -1), "names no group at all"),
    (np.array([0, 2] + [0] * 8), "gap in its numbering"),
])
def test_label_errors_are_raised_before_any_engine_call(no_engine, groups, text):
    with pytest.raises(ValueError, match=text):
        ls_spa_multi_sampled(*multi_data(10, 3, seed=1), groups=groups)


def test_the_limits_hold_with_groups(no_engine):
    z = np.zeros
    with pytest.raises(ValueError, match="at most p = 104"):
        ls_spa_multi_sampled(z((200, 105)), z((150, 105)), z((200, 2)), z((150, 2)), groups=np.zeros(105, dtype=int))
    with pytest.raises(ValueError, match="M >= p test rows \\(M = 9, p = 10\\)"):
        ls_spa_multi_sampled(z((40, 10)), z((9, 10)), z((40, 2)), z((9, 2)), groups=LABELS)
    # g > p: labels of length p with every group used cannot name more than p groups -- the nearest is a gap
    with pytest.raises(ValueError, match="gap in its numbering"):
        ls_spa_multi_sampled(*multi_data(4, 2, seed=1), groups=np.array([0, 1, 2, 5]))


def test_more_than_32_groups_are_fine():
    p = 40
    d = multi_data(p, 2, n=90, rows=60, seed=2)
    res = ls_spa_multi_sampled(*d, groups=np.arange(p)[::-1].copy(), max_samples=2, batch_size=2,
                               _engine=GroupedOracleEngine())
    assert res.attribution.shape == (2, p)


def test_perms_are_validated_in_dimension_g():
    d = multi_data(10, 2, seed=3)
    eng = GroupedOracleEngine()
    with pytest.raises(ValueError, match="length p = 3"):              # a column ordering is no group ordering
        ls_spa_multi_sampled(*d, groups=LABELS, perms=[np.arange(10)], _engine=eng)
    assert eng.calls[-1] == "free" and not batches(eng)
    eng = GroupedOracleEngine()
    with pytest.raises(ValueError, match="not a permutation of 0 .. g-1"):      # the engine's refusal comes through
        ls_spa_multi_sampled(*d, groups=LABELS, perms=[[0, 1, 1]], _engine=eng)
    assert eng.calls[-1] == "free" and not batches(eng)
    res = ls_spa_multi_sampled(*d, groups=LABELS, perms=[[2, 0, 1], [0, 1, 2]], _engine=GroupedOracleEngine())
    assert res.n_samples == 2


# ---- the result contract through the test double ---------------------------------------------------------------------
@pytest.mark.parametrize("anti", [False, True])
def test_fields_shapes_and_the_exact_value(anti):
    p, m, g = 10, 4, 3
    d = multi_data(p, m, seed=3)
    eng = GroupedOracleEngine()
    res = ls_spa_multi_sampled(*d, groups=LABELS, method="exact", antithetical=anti, _engine=eng)
    assert eng.calls[:2] == ["load", "players"] and eng.calls[-1] == "free"
    assert batches(eng) == [("batch", 6, False)]                      # all g! = 6 group orderings, never paired
    assert isinstance(res, SampledMultiGroupResults)
    assert [f for f in res.__dataclass_fields__] == ["attribution", "attribution_errors", "theta", "r_squared",
                                                     "baseline_r_squared", "n_samples"]
    assert res.attribution.shape == (m, g) and res.attribution_errors.shape == (m, g)
    assert res.theta.shape == (m, p) and res.r_squared.shape == (m,) and res.baseline_r_squared.shape == (m,)
    assert res.n_samples == 6
    theta, r2 = multi_fit(*d)
    np.testing.assert_allclose(res.theta, theta, rtol=0, atol=1e-12)
    np.testing.assert_allclose(res.r_squared, r2, rtol=0, atol=1e-12)
    base = LABELS == -1
    np.testing.assert_allclose(res.baseline_r_squared, multi_fit(d[0][:, base], d[1][:, base], d[2], d[3])[1],
                               rtol=0, atol=1e-12)
    np.testing.assert_allclose(res.attribution.sum(axis=1), res.r_squared - res.baseline_r_squared, rtol=0, atol=1e-11)
    # all group orderings: the Shapley values of the group game, from hp_ref's table of all subsets
    for r in range(m):
        want = hp_ref.Problem(d[0], d[1], d[2][:, r], d[3][:, r]).shapley(LABELS)
        np.testing.assert_allclose(res.attribution[r], want, rtol=0, atol=1e-11)
    assert "g = 3 groups, p = 10, m = 4 responses, 6 samples" in repr(res)
    by_hand = ls_spa_multi_sampled(*d, groups=LABELS, perms=list(permutations(range(g))), antithetical=False,
                                   _engine=GroupedOracleEngine())
    np.testing.assert_allclose(by_hand.attribution, res.attribution, rtol=0, atol=1e-14)


def test_an_antithetical_sample_is_the_mean_of_the_two_expansions():
    d = multi_data(10, 2, seed=4)
    res = ls_spa_multi_sampled(*d, groups=LABELS, perms=[[1, 2, 0]], antithetical=True, _engine=GroupedOracleEngine())
    two = ls_spa_multi_sampled(*d, groups=LABELS, perms=[[1, 2, 0], [0, 2, 1]], antithetical=False,
                               _engine=GroupedOracleEngine())
    np.testing.assert_allclose(res.attribution, two.attribution, rtol=0, atol=1e-14)
    assert res.n_samples == 1 and np.all(np.isinf(res.attribution_errors))


def test_groups_none_is_untouched():
    d = multi_data(10, 3, seed=5)
    eng = GroupedOracleEngine()
    a = ls_spa_multi_sampled(*d, max_samples=6, batch_size=4, groups=None, _engine=eng)
    b = ls_spa_multi_sampled(*d, max_samples=6, batch_size=4, _engine=MultiLiftOracleEngine())
    assert "players" not in eng.calls
    assert isinstance(a, SampledMultiResults) and a.attribution.shape == (3, 10)
    np.testing.assert_array_equal(a.attribution, b.attribution)
    np.testing.assert_array_equal(a.attribution_errors, b.attribution_errors)


# ---- the stop rule reads the [m][g] errors -----------------------------------------------------------------------------
def test_the_stop_rule_reads_the_group_errors():
    d = multi_data(10, 3, seed=5)
    eng = GroupedOracleEngine()
    res = ls_spa_multi_sampled(*d, groups=LABELS, max_samples=64, batch_size=4, tolerance=1e3, _engine=eng)
    assert res.n_samples == 4 and len(batches(eng)) == 1 and np.all(np.isfinite(res.attribution_errors))
    # a tolerance between the errors after one batch and after three: the run stops where the [m][g] errors say so
    eng = GroupedOracleEngine()
    full = ls_spa_multi_sampled(*d, groups=LABELS, max_samples=12, batch_size=4, _engine=eng)
    assert full.n_samples == 12 and eng.calls.count("get") == 1
    seen = []

    class Watching(GroupedOracleEngine):
        def multi_lift_get(self):
            out = super().multi_lift_get()
            assert out[1].shape == (3, 3) and out[2].shape == (3, 3)
            seen.append(float(_driver._multi_standard_errors(out[0], out[2]).max()))
            return out
    ls_spa_multi_sampled(*d, groups=LABELS, max_samples=12, batch_size=4, tolerance=0.0, _engine=Watching())
    tol = 0.5 * (seen[0] + seen[1])
    assert seen[1] < tol < seen[0]
    res = ls_spa_multi_sampled(*d, groups=LABELS, max_samples=12, batch_size=4, tolerance=tol,
                               _engine=GroupedOracleEngine())
    assert res.n_samples == 8


# ---- the sum check and the lifecycle -----------------------------------------------------------------------------------
def test_a_dropped_lift_fails_the_sum_check_and_frees():
    eng = GroupedOracleEngine(drop=True)
    with pytest.raises(LSSPANativeError, match="did not sum to the R\\^2"):
        ls_spa_multi_sampled(*multi_data(10, 3, seed=7), groups=LABELS, max_samples=4, batch_size=4, _engine=eng)
    assert eng.calls[-1] == "free"


def test_not_positive_definite_warns_and_frees():
    eng = GroupedOracleEngine(info=1, drop=True)
    with pytest.warns(RuntimeWarning, match="not numerically positive definite"):
        ls_spa_multi_sampled(*multi_data(10, 2, seed=8), groups=LABELS, max_samples=4, batch_size=4, _engine=eng)
    assert eng.calls[-1] == "free"


@pytest.mark.parametrize("where", ["multi_lift_set_players", "multi_lift_batch", "multi_lift_get"])
def test_an_error_on_any_engine_call_frees(where):
    class Failing(GroupedOracleEngine):
        pass

    def boom(self, *a, **k):
        raise LSSPANativeError("boom")
    setattr(Failing, where, boom)
    eng = Failing()
    with pytest.raises(LSSPANativeError, match="boom"):
        ls_spa_multi_sampled(*multi_data(10, 2, seed=9), groups=LABELS, max_samples=4, _engine=eng)
    assert eng.calls[0] == "load" and eng.calls[-1] == "free" and eng.calls.count("free") == 1


def test_empty_perms_are_refused_and_free():
    eng = GroupedOracleEngine()
    with pytest.raises(ValueError, match="perms is empty"):
        ls_spa_multi_sampled(*multi_data(10, 2, seed=9), groups=LABELS, perms=[], _engine=eng)
    assert eng.calls[-1] == "free"

