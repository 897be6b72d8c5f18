"""ls_spa_best_subsets(groups=): the best set of groups of every size by out-of-sample R^2 -- CPU side.

The gap between best and runner-up of every case the GPU tests compare with the brute-force truth of
tests/group_best_ref.py (no GPU assertion then meets a near-tie); what the layouts of those cases reach, through the
host-only planner lsspa_debug_groups_best_plan; the exact-tie problem; and the driver's plumbing through a NumPy double
of the engine whose enumeration is that truth."""
import warnings

import numpy as np
import pytest

import best_ref as B
import group_best_ref as R
from ls_spa import BestGroupSubsetsResults, BestSubsetsResults, _driver, ls_spa, ls_spa_best_subsets
from ls_spa._engine import GROUPS_BEST_PLAN_FIELDS, debug_groups_best_plan
from test_best_subsets_host import BestOracleEngine
from test_groups_host import GroupsOracleEngine, group_values, labels_of, value
from test_subsets_host import data, gram_problem

ALL = [(name, reg) for name in R.CASES for reg in R.REGS]


# ---- the truth ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, reg", ALL)
def test_every_gpu_case_has_a_clear_winner(name, reg):
    d, labels, u = R.brute_case(name, reg)
    g = int(labels.max()) + 1
    best, masks, found, runner = B.best_truth(u, g)
    assert found.all() and masks[0] == 0 and masks[g] == (1 << g) - 1
    assert ((best - runner) > R.MIN_GAP).all(), (name, reg, (best - runner).min())
    # size 0 is the baseline alone, size g the full model
    G, gv, H, h, yy = gram_problem(*d, reg=reg)
    base = np.nonzero(labels < 0)[0]
    r2_base = value(G, gv, H, h, yy, base)
    assert abs(best[0] - r2_base) < 1e-13 and (len(base) > 0 or best[0] == 0.0)
    assert (d[1].shape[0] < d[0].shape[1]) == (name in R.RECT)


def test_truth_is_the_column_truth_on_singletons():
    d, v = B.brute_case(9, 0.0)
    u = R.all_group_values(d, np.arange(9))
    np.testing.assert_allclose(u, v, rtol=0, atol=1e-12)
    np.testing.assert_array_equal(B.best_truth(u, 9)[1], B.best_truth(v, 9)[1])


# ---- reach: what the layouts of the cases make the kernel do -------------------------------------------------------------
def all_plans():
    plans = {name: (R.case_labels(name), want) for name, want in R.PLAN.items()}
    plans.update(R.PLANTED)
    return plans


@pytest.mark.parametrize("name", list(R.PLAN) + list(R.PLANTED))
def test_plan_of_every_case(name):
    labels, want = all_plans()[name]
    got = debug_groups_best_plan(labels)
    assert tuple(got) == GROUPS_BEST_PLAN_FIELDS and got == want
    assert got["units"] * got["per"] == 1 << got["gh"] and got["classes"] == got["per"].bit_length()
    assert got["gl"] + got["gh"] == int(np.max(labels)) + 1


def test_the_cases_together_reach_every_edge():
    plans = [debug_groups_best_plan(labels) for labels, _ in all_plans().values()]
    plans += [debug_groups_best_plan(R.tie_case(run)[1]) for run in R.TIE_RUNS]
    assert any(q["gl"] == 0 for q in plans)                                   # only lane 0 holds a value
    assert any(q["gl"] == 6 and q["ql"] == 6 for q in plans)                  # all 64 lanes
    assert any(0 < q["gl"] < q["ql"] < 6 and q["gh"] > 0 for q in plans)      # a mixed low set that stops early
    assert any(q["gh"] == 0 and q["units"] == 1 and q["per"] == 1 for q in plans)
    assert any(q["nb"] == 0 for q in plans) and any(q["nb"] > 0 for q in plans)
    assert any(q["per"] > 1 for q in plans) and any(q["launches"] > 1 for q in plans)
    assert max(q["classes"] for q in plans) == 10                             # the deepest class a few-second test reaches


def test_the_kernel_holds_the_classes_of_the_largest_plan():
    # 32 groups of 2: three low groups, gh = 29 -- as many high groups as 64 columns allow at g = 32
    labels = np.repeat(np.arange(32), 2)
    q = debug_groups_best_plan(labels)
    assert q["gl"] == 3 and q["gh"] == 29 and q["units"] == 8192 and q["per"] == 1 << 16 and q["classes"] == 17
    assert q["classes"] <= 19                    # GROUPS_BEST_CLASSES (csrc/kernels.h): gh <= 31 over 8192 units


@pytest.mark.parametrize("labels", [[0, 0, 2, 2], [-2, 0, 0, 1], [-1, -1, -1], np.arange(33), np.zeros(65, dtype=int)])
def test_plan_refuses_what_the_call_refuses(labels):
    with pytest.raises(ValueError, match="lsspa_debug_groups_best_plan"):
        debug_groups_best_plan(labels)


# ---- the exact-tie problem ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", list(R.TIE_RUNS))
def test_tie_problem_is_tied_exactly_and_only_there(run):
    d, labels, u = R.tie_case(run)
    lab = R.TIE_RUNS[run]
    abc = sum(1 << lab[k] for k in "abc")
    inside = np.array([m for m in range(32) if not m & ~abc])
    outside = np.array([m for m in range(32) if m & ~abc])
    assert (u[inside] == 0.0).all() and (u[outside] < -1e-9).all()
    # exactly zero because g is: no rounding is involved
    G, gv, _, _, _ = gram_problem(*d)
    assert (gv[np.isin(labels, [lab[k] for k in "abc"])] == 0.0).all()
    assert (d[0] == np.round(d[0]))[:, np.isin(labels, [lab[k] for k in "abc"])].all()
    best, masks, found, runner = B.best_truth(u, 5)
    assert list(masks[1:4]) == R.tie_winners(run) and (best[1:4] == 0.0).all() and (runner[1:3] == 0.0).all()
    q = debug_groups_best_plan(labels)
    assert q["gl"] == 3 and q["gh"] == 2         # a (with d and e) low, b and c high


def test_tie_runs_disagree_about_the_order():
    # "disagree": a layout-order tie-break would take a (low: the layout's group 0) at size 1; the caller's smallest is b
    assert R.tie_winners("agree")[0] == 1 << R.TIE_RUNS["agree"]["a"]
    assert R.tie_winners("disagree")[0] == 1 << R.TIE_RUNS["disagree"]["b"] == 1
    assert R.TIE_RUNS["disagree"]["a"] > R.TIE_RUNS["disagree"]["c"]


# ---- driver plumbing on a test double -----------------------------------------------------------------------------------
class GroupBestOracleEngine(GroupsOracleEngine, BestOracleEngine):
    """The oracle engines of the grouped attribution and of the column selection with the grouped selection's entry
    point, computed by the brute-force truth.  info: the info word it reports; drop: sizes it reports as not found;
    values: u of every group mask instead of the oracle's."""

    def __init__(self, info=0, drop=(), values=None):
        BestOracleEngine.__init__(self, info=info, drop=drop, values=values)
        self.subsets_calls, self.groups_calls, self.group_best_calls = 0, [], []

    def groups_best(self, labels):
        assert isinstance(labels, np.ndarray) and labels.dtype == np.int32 and labels.shape == (self.p,)
        self.group_best_calls.append(labels.copy())
        g = int(labels.max()) + 1
        u = self._values
        if u is None:
            G, gv, H, h = self.gram()
            u = group_values(G, gv, H, h, self.y_norm_sq, labels, np.arange(1 << g))
        best, masks, found, _ = B.best_truth(np.asarray(u, dtype=np.float64), g)
        for k in self._drop:
            best[k], masks[k], found[k] = np.nan, 0, False
        return best, masks, found, self._info


def test_result_shapes_and_fields():
    labels = labels_of([2, 3, 1, 2], 2, seed=7)
    p, g = len(labels), 4
    d = data(p, seed=70)
    eng = GroupBestOracleEngine()
    res = ls_spa_best_subsets(*d, groups=labels, _engine=eng)
    assert isinstance(res, BestGroupSubsetsResults) and len(eng.group_best_calls) == 1 and eng.best_calls == []
    np.testing.assert_array_equal(eng.group_best_calls[0], labels)
    assert res.sizes.tolist() == list(range(g + 1))
    assert res.group_subsets.shape == (g + 1, g) and res.group_subsets.dtype == bool
    assert res.subsets.shape == (g + 1, p) and res.subsets.dtype == bool
    assert res.r_squared.shape == (g + 1,) and res.theta.shape == (g + 1, p) and res.n_columns.shape == (g + 1,)
    assert res.group_subsets.sum(axis=1).tolist() == list(range(g + 1))
    u = group_values(*eng.gram(), eng.y_norm_sq, labels, np.arange(1 << g))          # the double's own problem
    best, masks, _, _ = B.best_truth(u, g)
    np.testing.assert_array_equal(res.r_squared, best)
    for k in range(g + 1):
        assert B.mask_of(np.nonzero(res.group_subsets[k])[0]) == masks[k]
        np.testing.assert_array_equal(res.subsets[k], R.columns_of(labels, masks[k]))
        assert res.n_columns[k] == res.subsets[k].sum()
    assert res.subsets[:, labels < 0].all() and res.n_columns[0] == 2 and res.n_columns[g] == p
    assert res.best_size == int(np.argmax(best))
    np.testing.assert_array_equal(res.best_group_subset, res.group_subsets[res.best_size])
    np.testing.assert_array_equal(res.best_subset, res.subsets[res.best_size])
    assert res.baseline_r_squared == res.r_squared[0]
    full = ls_spa(*d, method="subsets", groups=labels, _engine=GroupsOracleEngine())
    assert res.full_r_squared == full.r_squared
    np.testing.assert_allclose(res.theta[g], full.theta, rtol=1e-9, atol=1e-12)
    assert "Best model" in repr(res) and "groups" in repr(res)


def test_no_baseline_starts_at_zero():
    labels = labels_of([2, 2, 3], 0, seed=3)
    res = ls_spa_best_subsets(*data(7, seed=4), groups=labels, _engine=GroupBestOracleEngine())
    assert res.r_squared[0] == 0.0 and res.baseline_r_squared == 0.0 and not res.subsets[0].any()
    assert (res.theta[0] == 0.0).all() and res.n_columns[0] == 0


def test_theta_is_the_refit_with_exact_zeros():
    labels = labels_of([3, 1, 2, 2], 1, seed=5)
    p, g = len(labels), 4
    d = data(p, seed=5)
    res = ls_spa_best_subsets(*d, reg=0.05, groups=labels, _engine=GroupBestOracleEngine())
    G, gv, H, h, yy = gram_problem(*d, reg=0.05)
    for k in range(g + 1):
        cols, out = np.nonzero(res.subsets[k])[0], np.nonzero(~res.subsets[k])[0]
        assert (res.theta[k, out] == 0.0).all() and not np.signbit(res.theta[k, out]).any()
        th = np.linalg.solve(G[np.ix_(cols, cols)], gv[cols])
        np.testing.assert_allclose(res.theta[k, cols], th, rtol=1e-9, atol=1e-12)
        r2 = (2.0 * th @ h[cols] - th @ H[np.ix_(cols, cols)] @ th) / yy
        assert abs(r2 - res.r_squared[k]) < 1e-12


def test_best_size_takes_the_smallest_of_equal_maxima_and_skips_nan():
    labels = np.array([0, 1, 1, 2])
    d = data(4, seed=2)
    u = np.array([0.0, 0.6, 0.1, 0.6, 0.2, 0.3, 0.1, 0.9])         # sizes: 0 | 0.6 | 0.6 | 0.9
    res = ls_spa_best_subsets(*d, groups=labels, _engine=GroupBestOracleEngine(values=u))
    assert res.best_size == 3
    with pytest.warns(RuntimeWarning, match="not numerically positive definite"):
        res = ls_spa_best_subsets(*d, groups=labels, _engine=GroupBestOracleEngine(values=u, drop=(3,), info=1))
    assert res.best_size == 1 and res.best_group_subset.tolist() == [True, False, False]        # size 1 before size 2
    assert res.best_subset.tolist() == [True, False, False, False]
    assert np.isnan(res.r_squared[3]) and np.isnan(res.theta[3]).all()
    assert not res.subsets[3].any() and not res.group_subsets[3].any() and res.n_columns[3] == 0
    assert res.r_squared[:3].tolist() == [0.0, 0.6, 0.6]
    with pytest.warns(RuntimeWarning):
        res = ls_spa_best_subsets(*d, groups=labels,
                                  _engine=GroupBestOracleEngine(values=u, drop=(0, 1, 2, 3), info=1))
    assert res.best_size == -1 and not res.best_subset.any() and not res.best_group_subset.any()
    assert np.isnan(res.baseline_r_squared)


def test_not_positive_definite_warns_and_names_this_file():
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        ls_spa_best_subsets(*data(5, seed=2), groups=[0, 0, 1, 1, -1], _engine=GroupBestOracleEngine(info=1))
    assert len(seen) == 1 and issubclass(seen[0].category, RuntimeWarning)
    assert "not numerically positive definite" in str(seen[0].message) and seen[0].filename == __file__


def test_no_warning_without_the_info_bit():
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ls_spa_best_subsets(*data(5, seed=2), groups=[0, 0, 1, 1, -1], _engine=GroupBestOracleEngine())


def _zero_y(d):
    return d[0], d[1], d[2], np.zeros_like(d[3])


@pytest.mark.parametrize("make, kw, error, text", [
    (lambda: data(65, n=140, m=100, seed=1), dict(groups=np.arange(65) % 8), ValueError, "at most p = 64"),
    (lambda: data(40, n=100, m=80, seed=1), dict(groups=np.minimum(np.arange(40), 32)), ValueError, "at most g = 32"),
    (lambda: data(4), dict(groups=[0, 2, 2, 0]), ValueError, "gap in its numbering.*label 1"),
    (lambda: data(4), dict(groups=[0, -2, 1, 1]), ValueError, "below -1"),
    (lambda: data(4), dict(groups=[-1, -1, -1, -1]), ValueError, "no group at all"),
    (lambda: data(4), dict(groups=[0, 1, 1]), ValueError, "length p = 4"),
    (lambda: data(4), dict(groups=[0.0, 1.0, 1.0, 0.0]), ValueError, "integer labels"),
    (lambda: data(4), dict(groups=[0, 0, 1, 1], include=[0]), ValueError, "label the columns.*-1"),
    (lambda: data(4), dict(groups=[0, 0, 1, 1], include=[]), ValueError, "label the columns.*-1"),
    (lambda: _zero_y(data(4)), dict(groups=[0, 0, 1, 1]), ValueError, "identically zero"),
])
def test_refusals_come_before_any_engine_work(monkeypatch, make, kw, error, text):
    def no_engine(*a, **k):
        raise AssertionError("an engine was acquired")
    monkeypatch.setattr(_driver, "_acquire_engine", no_engine)
    eng = GroupBestOracleEngine()
    with pytest.raises(error, match=text):
        ls_spa_best_subsets(*make(), _engine=eng, **kw)
    assert eng.touched == 0 and eng.group_best_calls == [] and eng.best_calls == []
    with pytest.raises(error, match=text):
        ls_spa_best_subsets(*make(), **kw)          # no engine of the caller's: none is acquired either


def test_groups_none_reaches_the_column_selection():
    d = data(7, seed=71)
    eng = GroupBestOracleEngine()
    res = ls_spa_best_subsets(*d, groups=None, include=[2], _engine=eng)
    assert isinstance(res, BestSubsetsResults) and eng.best_calls == [4] and eng.group_best_calls == []
    ref = ls_spa_best_subsets(*d, include=[2], _engine=BestOracleEngine())
    for name in ("sizes", "subsets", "r_squared", "theta", "best_subset"):
        np.testing.assert_array_equal(getattr(res, name), getattr(ref, name))
    assert res.best_size == ref.best_size and res.full_r_squared == ref.full_r_squared
    with pytest.raises(ValueError, match="at most p = 32"):         # the column call's limit stays
        ls_spa_best_subsets(*data(33, n=80, m=50, seed=1), _engine=GroupBestOracleEngine())


def test_more_than_32_columns_are_taken_with_groups():
    labels = labels_of([5] * 7, 1, seed=8)     # p = 36
    res = ls_spa_best_subsets(*data(36, n=150, m=110, seed=72), groups=labels, _engine=GroupBestOracleEngine())
    assert res.subsets.shape == (8, 36) and res.n_columns.tolist() == [1 + 5 * k for k in range(8)]


def test_kept_engine_back_to_float64():
    class Float32Engine(GroupBestOracleEngine):
        precision = "float32"

        def set_precision(self, dtype):
            self.precision = np.dtype(dtype).name

        def full_fit(self):
            assert self.precision == "float64", "full fit with fp32 factorisation"
            return super().full_fit()

    eng = Float32Engine()
    ls_spa_best_subsets(*data(6, seed=3), groups=[0, 0, 1, 1, -1, 2], _engine=eng)
    assert eng.precision == "float64"
