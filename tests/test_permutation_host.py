"""ls_spa_permutation_test without a GPU: the permutations of csrc/host_perms.cpp against their NumPy restatement
(tests/perm_ref.py), the plan of a run (which edges the GPU cases of tests/test_gpu_permutation_test.py reach), and the
driver -- fields, formulas, refusals, lifecycle -- through a NumPy double of the engine."""
import collections
import warnings

import numpy as np
import pytest

import perm_ref
from ls_spa import PermutationTestResults, SizeIncompatible, _driver, ls_spa_permutation_test
from ls_spa._engine import debug_perm_indices, debug_perm_plan
from test_subsets_host import data


# ---- the permutations ------------------------------------------------------------------------------------------------
STREAMS = [(1, 0, 0), (1, 0, 1), (2 ** 63 + 5, 7, 1), (42, 2 ** 32 + 3, 0), (2 ** 64 - 1, 2 ** 40, 1)]


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 8, 9, 257, 4099])
def test_indices_equal_the_restatement_and_are_permutations(n):
    for seed, r, side in STREAMS:
        got = debug_perm_indices(seed, r, side, n)
        assert got.dtype == np.uint32
        np.testing.assert_array_equal(got, perm_ref.indices(seed, r, side, n))
        np.testing.assert_array_equal(np.sort(got), np.arange(n))


def test_train_and_test_streams_differ():
    for seed, r in [(1, 0), (42, 5), (7, 2 ** 32)]:
        assert not np.array_equal(debug_perm_indices(seed, r, 0, 257), debug_perm_indices(seed, r, 1, 257))
    assert not np.array_equal(debug_perm_indices(1, 0, 0, 257), debug_perm_indices(1, 1, 0, 257))
    assert not np.array_equal(debug_perm_indices(1, 0, 0, 257), debug_perm_indices(2, 0, 0, 257))


def test_bad_arguments_of_the_hook():
    for args in [(1, 0, 2, 4), (1, 0, -1, 4), (1, 0, 0, 0), (1, 0, 0, 2 ** 31)]:
        with pytest.raises(ValueError):
            debug_perm_indices(*args)


def test_all_24_permutations_of_four_occur_evenly():
    """r = 0 .. 23999 at seed 2024, training side: 1000 expected of each of the 24 permutations.  The chi-square of the
    counts is deterministic: 14.512 by the restatement (23 degrees of freedom: the mean is 23, the 99.9 % point 49.7).
    The bound is that value and a margin of rounding in the sum only."""
    cnt = collections.Counter(tuple(int(v) for v in perm_ref.indices(2024, r, 0, 4)) for r in range(24000))
    lib = collections.Counter(tuple(int(v) for v in debug_perm_indices(2024, r, 0, 4)) for r in range(24000))
    assert cnt == lib and len(cnt) == 24
    chi2 = sum((c - 1000) ** 2 / 1000 for c in cnt.values())
    print(f"chi2 = {chi2:.3f}")
    assert chi2 < 14.6


# ---- the plan: which edges the GPU cases reach -----------------------------------------------------------------------
def _plans():
    return [(c, debug_perm_plan(c[4], c[0], c[1], c[2], c[5])) for c in perm_ref.XTY_CASES]


def test_plan_basics():
    P = debug_perm_plan(1000, 100000, 100000, 12)
    assert P["cb"] == 1 and P["rps_train"] % 16 == 0 and P["slices_train"] <= 128
    assert P["slices_train"] == -(-100000 // P["rps_train"])
    assert P["rep_bytes"] * P["block"] <= 256 << 20 and P["n_blocks"] == -(-1000 // P["block"])
    assert debug_perm_plan(5000, 300, 300, 4)["block"] == 1024            # the cap
    assert debug_perm_plan(5, 7, 9, 64)["ldi_train"] == 8 and debug_perm_plan(5, 7, 9, 64)["cb"] == 4
    # the slices are a function of the rows alone
    for R, block in [(1, 0), (37, 0), (37, 8), (2000, 16)]:
        Q = debug_perm_plan(R, 100000, 777, 12, block)
        assert (Q["rps_train"], Q["slices_train"], Q["rps_test"], Q["slices_test"]) == \
               (P["rps_train"], P["slices_train"], 256, 4)
    for bad in [(0, 10, 10, 4, 0), (1, 0, 10, 4, 0), (1, 10, 2 ** 31, 4, 0), (1, 10, 10, 65, 0), (1, 10, 10, 0, 0),
                (1, 10, 10, 4, -1)]:
        with pytest.raises(ValueError):
            debug_perm_plan(*bad)


def test_the_gpu_cases_reach_the_edges():
    plans = _plans()
    sides = [(n, P["rps_" + s], P["slices_" + s]) for (c, P) in plans for n, s in ((c[0], "train"), (c[1], "test"))]
    assert any(sl > 1 and n % rps == 1 for n, rps, sl in sides), "a one-row slice tail"
    assert any(sl > 1 and n % rps == 0 for n, rps, sl in sides), "a full last slice behind another"
    assert any(sl == 1 and n == rps - 1 for n, rps, sl in sides), "one row short of a slice"
    assert any(n % 16 not in (0,) and n % 4 == 0 for n, _, _ in sides) and any(n % 4 for n, _, _ in sides)
    assert {n for n, _, _ in sides} >= {1, 3, 4, 5, 63, 64, 65, 255, 256, 257}
    last = [c[4] - (P["n_blocks"] - 1) * P["block"] for c, P in plans]
    blocks = [P["block"] for _, P in plans]
    assert any(b % 16 for b in blocks + last) and any(b % 64 and b > 64 for b in blocks)
    assert any(P["n_blocks"] > 1 for _, P in plans) and any(b == 16 for b in blocks)
    assert any(x < P["block"] for x, (_, P) in zip(last, plans)), "a ragged last block"
    assert {c[2] for c in perm_ref.XTY_CASES} >= {1, 15, 16, 17, 32, 33, 48, 64}
    assert {c[4] for c in perm_ref.XTY_CASES} >= {1, 15, 16, 17, 63, 65}
    assert {P["cb"] for _, P in plans} == {1, 2, 3, 4}
    assert any(c[1] < c[2] for c in perm_ref.XTY_CASES), "M < p"


# ---- the driver through the double -----------------------------------------------------------------------------------
LABELS = np.array([0, 1, -1, 1, 2, 0])


def _formulas(res):
    att, null = res.attribution, res.null_attribution
    n = res.n_perm - res.n_failed
    np.testing.assert_array_equal(res.p_values, (1 + (null >= att).sum(axis=0)) / (1 + n))
    np.testing.assert_array_equal(res.p_values_adjusted, (1 + (null.max(axis=1)[:, None] >= att).sum(axis=0)) / (1 + n))
    assert res.r_squared_p_value == (1 + (res.null_r_squared >= res.r_squared).sum()) / (1 + n)
    assert np.all(res.p_values_adjusted >= res.p_values)


@pytest.mark.parametrize("reg", [0.0, 0.1])
def test_fields_shapes_and_sums(reg):
    p, R = 5, 23
    d = data(p, seed=3)
    eng = perm_ref.PermOracleEngine()
    res = ls_spa_permutation_test(*d, reg, n_perm=R, seed=11, _engine=eng)
    assert eng.calls == ["load", "observed", "run", "free"]
    assert isinstance(res, PermutationTestResults)
    assert res.attribution.shape == (p,) and res.theta.shape == (p,) and res.null_attribution.shape == (R, p)
    assert res.null_r_squared.shape == (R,) and res.p_values.shape == (p,) and res.p_values_adjusted.shape == (p,)
    assert res.n_perm == R and res.n_failed == 0
    assert res.baseline_r_squared is None and res.null_baseline_r_squared is None
    assert isinstance(res.r_squared, float) and isinstance(res.r_squared_p_value, float)
    np.testing.assert_allclose(res.attribution.sum(), res.r_squared, rtol=0, atol=1e-9)
    np.testing.assert_allclose(res.null_attribution.sum(axis=1), res.null_r_squared, rtol=0, atol=1e-9)
    _formulas(res)
    assert "n_perm = 23" in repr(res)


def test_fields_with_groups():
    R = 9
    d = data(len(LABELS), seed=4)
    res = ls_spa_permutation_test(*d, n_perm=R, groups=LABELS, _engine=perm_ref.PermOracleEngine())
    assert res.attribution.shape == (3,) and res.theta.shape == (6,) and res.null_attribution.shape == (R, 3)
    assert res.null_baseline_r_squared.shape == (R,) and isinstance(res.baseline_r_squared, float)
    np.testing.assert_allclose(res.attribution.sum(), res.r_squared - res.baseline_r_squared, rtol=0, atol=1e-9)
    np.testing.assert_allclose(res.null_attribution.sum(axis=1), res.null_r_squared - res.null_baseline_r_squared,
                               rtol=0, atol=1e-9)
    _formulas(res)


def test_the_same_seed_gives_the_same_permutations_with_and_without_groups():
    d = data(len(LABELS), seed=4)
    a = ls_spa_permutation_test(*d, n_perm=5, seed=3, groups=LABELS, _engine=perm_ref.PermOracleEngine())
    b = ls_spa_permutation_test(*d, n_perm=5, seed=3, _engine=perm_ref.PermOracleEngine())
    np.testing.assert_array_equal(a.null_r_squared, b.null_r_squared)


class _Spy(perm_ref.PermOracleEngine):
    def perm_run(self, *a, **k):
        out = super().perm_run(*a, **k)
        self.sides, self.gperm, self.hperm = k["sides"], out[1], out[2]
        return out


@pytest.mark.parametrize("permute, bits", [("train", 1), (("test",), 2), (("test", "train"), 3)])
def test_permute_one_side_keeps_the_other_sides_observed_sums(permute, bits):
    d = data(4, seed=5)
    eng = _Spy()
    ls_spa_permutation_test(*d, n_perm=6, permute=permute, _engine=eng)
    assert eng.sides == bits
    _, g, _, h, _ = eng.perm_gram()
    # (the double forms the sums by a matrix product: equal to the last bits of a sum of 40 .. 60 terms, or far apart)
    assert np.allclose(eng.hperm, h[None], rtol=1e-12, atol=0) == (not bits & 2)
    assert np.allclose(eng.gperm, g[None], rtol=1e-12, atol=0) == (not bits & 1)


def test_not_positive_definite_warns_and_frees():
    eng = perm_ref.PermOracleEngine(info=1)
    with pytest.warns(RuntimeWarning, match="not numerically positive definite"):
        res = ls_spa_permutation_test(*data(4, seed=8), n_perm=3, _engine=eng)
    assert eng.calls[-1] == "free" and res.n_failed in (0, 3)


@pytest.mark.parametrize("where", ["load", "observed", "run"])
def test_perm_free_is_called_after_an_exception(where):
    eng = perm_ref.PermOracleEngine(fail_in=where)
    with pytest.raises(RuntimeError, match="planted"):
        ls_spa_permutation_test(*data(4, seed=8), n_perm=3, _engine=eng)
    assert eng.calls[-1] == "free"


def test_non_finite_replicates_are_left_out():
    null = np.array([[0.1, 0.2], [np.nan, 0.0], [0.3, 0.0]])
    res = PermutationTestResults.from_null(np.array([0.2, 0.1]), np.zeros(2), 0.3, null, np.array([0.3, 0.1, 0.3]))
    assert res.n_failed == 1 and res.n_perm == 3
    np.testing.assert_array_equal(res.p_values, [2 / 3, 2 / 3])
    np.testing.assert_array_equal(res.p_values_adjusted, [1.0, 1.0])
    assert res.r_squared_p_value == 1.0


# ---- refusals: all before an engine exists -----------------------------------------------------------------------------
@pytest.fixture
def no_engine(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("an engine was acquired")
    monkeypatch.setattr(_driver, "_acquire_engine", refuse)


def _ones(n=80, m=70, p=4):
    return np.ones((n, p)), np.ones((m, p)), np.ones(n), np.ones(m)


@pytest.mark.parametrize("kw, exc, text", [
    (dict(), ValueError, None),
    (dict(n_perm=0), ValueError, "n_perm must be an integer >= 1"),
    (dict(n_perm=2.5), ValueError, "n_perm must be an integer >= 1"),
    (dict(permute=()), ValueError, "permute must name"),
    (dict(permute="both"), ValueError, "permute must name"),
    (dict(permute=("train", "train")), ValueError, "permute must name"),
    (dict(groups=[0, 1, 3, 0]), ValueError, None),
    (dict(groups=[0, 1]), ValueError, None),
])
def test_refused_before_any_engine(no_engine, kw, exc, text):
    d = _ones()
    if not kw:
        d = d[:3] + (np.zeros(70),)
        text = "y_test is identically zero"
    with pytest.raises(exc, match=text):
        ls_spa_permutation_test(*d, **kw)


def test_limits_are_named(no_engine):
    with pytest.raises(ValueError, match="at most p = 32"):
        ls_spa_permutation_test(*_ones(p=33))
    with pytest.raises(ValueError, match="at most p = 64"):
        ls_spa_permutation_test(*_ones(p=65), groups=np.arange(65) % 3)
    with pytest.raises(ValueError):
        ls_spa_permutation_test(*_ones(p=40), groups=np.arange(40) % 33)        # g = 33
    with pytest.raises(SizeIncompatible):
        ls_spa_permutation_test(np.ones((80, 4)), np.ones((70, 5)), np.ones(80), np.ones(70))
    with pytest.raises(SizeIncompatible):
        ls_spa_permutation_test(np.ones((80, 4)), np.ones((70, 4)), np.ones(79), np.ones(70))
    with pytest.raises(ValueError, match="one-dimensional"):
        ls_spa_permutation_test(np.ones((80, 4)), np.ones((70, 4)), np.ones((80, 1)), np.ones((70, 1)))


# ---- a planted effect ---------------------------------------------------------------------------------------------------
def test_planted_effect_gets_the_smallest_possible_p_value():
    """N = M = 200, p = 4, y = 3 x_0 + noise, 199 permutations: by the reference arithmetic of the double the observed
    share of x_0 is 0.919 against a largest null share of 0.028, and R^2 0.898 against 0.035 -- room to spare."""
    rng = np.random.default_rng(5)
    Xa, Xe = rng.standard_normal((200, 4)), rng.standard_normal((200, 4))
    ya, ye = 3 * Xa[:, 0] + rng.standard_normal(200), 3 * Xe[:, 0] + rng.standard_normal(200)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        res = ls_spa_permutation_test(Xa, Xe, ya, ye, n_perm=199, seed=7, _engine=perm_ref.PermOracleEngine())
    assert res.p_values[0] == 1 / 200 and res.p_values_adjusted[0] == 1 / 200 and res.r_squared_p_value == 1 / 200
    assert res.attribution[0] > 0.9 and res.null_attribution.max() < 0.05
    assert np.all(res.p_values[1:] > 0.2)
