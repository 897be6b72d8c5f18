"""ls_spa_multi(groups=labels): the exact attribution of many responses over groups of columns -- CPU side.

The batched oracle solves every group subset once with all responses as right-hand sides and takes the Shapley values
from the table of all 2^g values; it is checked here against the loop of the one-response oracle of
tests/test_groups_host.py, by efficiency and on the reference fixtures.  Then the driver's refusals, all raised before
an engine exists, and its result contract through a test double of the engine whose enumeration is that oracle."""
from math import comb

import numpy as np
import pytest

from ls_spa import MultiGroupResults, MultiResponseResults, _driver, ls_spa_multi
from test_groups_host import group_shapley, group_values, labels_of, value
from test_multi_host import multi_data, multi_fit, multi_gram_problem, multi_oracle, with_responses
from test_subsets_host import data, golden


# ---- the batched oracle ----------------------------------------------------------------------------------------------
def multi_group_values(G, g, H, h, yy, labels, masks):
    """u [n][m]: u_r(S) = v_r(B + columns of the groups in S) for every mask (bit k = group k) and response, one
    factorisation per mask with all responses as right-hand sides."""
    labels = np.asarray(labels)
    ng = int(labels.max()) + 1
    member = [np.nonzero(labels == k)[0] for k in range(ng)]
    base = np.nonzero(labels == -1)[0]
    out = np.zeros((len(masks), len(yy)))
    for i, mk in enumerate(masks):
        mk = int(mk)
        cols = np.sort(np.concatenate([base] + [member[k] for k in range(ng) if (mk >> k) & 1]).astype(np.int64))
        if len(cols) == 0:
            continue
        sub = np.ix_(cols, cols)
        th = np.linalg.solve(G[sub], g[:, cols].T)                     # [k][m]
        out[i] = (2.0 * np.einsum("km,mk->m", th, h[:, cols]) - np.einsum("km,km->m", th, H[sub] @ th)) / yy
    return out


def multi_shapley_of_table(u, ng):
    """phi [m][g] from the table u [2^g][m]: test_groups_host.shapley_of_table for every column at once."""
    masks = np.arange(1 << ng, dtype=np.int64)
    size = ((masks[:, None] >> np.arange(ng)) & 1).sum(axis=1)
    w = np.array([1.0 / (ng * comb(ng - 1, k)) for k in range(ng)])
    phi = np.zeros((u.shape[1], ng))
    for k in range(ng):
        S_ = masks[(masks >> k) & 1 == 0]
        phi[:, k] = (w[size[S_]][:, None] * (u[S_ | (1 << k)] - u[S_])).sum(axis=0)
    return phi


def multi_group_oracle(Xa, Xe, Ya, Ye, labels, reg=0.0):
    """phi [m][g] of ls_spa_multi(groups=labels)."""
    prob = multi_gram_problem(Xa, Xe, Ya, Ye, reg)
    ng = int(np.max(labels)) + 1
    return multi_shapley_of_table(multi_group_values(*prob, labels, np.arange(1 << ng)), ng)


def baseline_r_squared(Xa, Xe, Ya, Ye, labels, reg=0.0):
    G, g, H, h, yy = multi_gram_problem(Xa, Xe, Ya, Ye, reg)
    base = np.nonzero(np.asarray(labels) == -1)[0]
    return np.array([value(G, g[r], H, h[r], yy[r], base) for r in range(len(yy))])


def grouped_data(sizes, nb, m, seed):
    """(labels shuffled, (Xa, Xe, Ya, Ye)) of groups with the given sizes, nb baseline columns and m responses."""
    labels = labels_of(sizes, nb, seed=seed)
    p = len(labels)
    return labels, with_responses(*data(p, n=4 * p + 8, m=3 * p + 5, seed=seed), m, seed)


CASES = [([1, 2, 3], 0), ([2, 1, 2], 2), ([3, 3, 1, 2], 1)]


@pytest.mark.parametrize("reg", [0.0, 0.1])
@pytest.mark.parametrize("sizes, nb", CASES)
def test_batched_oracle_equals_the_loop_per_column(sizes, nb, reg):
    labels, d = grouped_data(sizes, nb, 3, seed=10 + len(sizes) + nb)
    G, g, H, h, yy = multi_gram_problem(*d, reg)
    got = multi_group_oracle(*d, labels, reg=reg)
    assert got.shape == (3, len(sizes))
    masks = np.arange(1 << len(sizes))
    u = multi_group_values(G, g, H, h, yy, labels, masks)
    for r in range(3):
        np.testing.assert_allclose(got[r], group_shapley(G, g[r], H, h[r], yy[r], labels), rtol=0, atol=1e-13)
        np.testing.assert_allclose(u[:, r], group_values(G, g[r], H, h[r], yy[r], labels, masks), rtol=0, atol=1e-13)


@pytest.mark.parametrize("sizes, nb", CASES)
def test_rows_sum_to_r_squared_minus_the_baselines(sizes, nb):
    labels, d = grouped_data(sizes, nb, 3, seed=30 + len(sizes))
    base = baseline_r_squared(*d, labels)
    assert np.all(base == 0.0) == (nb == 0)
    np.testing.assert_allclose(multi_group_oracle(*d, labels).sum(axis=1), multi_fit(*d)[1] - base, rtol=0, atol=1e-12)


@pytest.mark.parametrize("name", ["toy", "exact_p4", "exact_p8"])
def test_singleton_labels_on_the_reference_fixtures(name):
    g = golden(name)
    d = with_responses(g["X_train"], g["X_test"], g["y_train"], g["y_test"], 4, seed=len(name))
    p = d[0].shape[1]
    phi = multi_group_oracle(*d, np.arange(p))
    np.testing.assert_allclose(phi, multi_oracle(*d), rtol=0, atol=1e-13)
    np.testing.assert_allclose(phi[0], g["attribution"], rtol=0, atol=1e-12)      # column 0 is the fixture's y


# ---- the result contract through a test double -----------------------------------------------------------------------
class MultiGroupOracleEngine:
    """What ls_spa_multi asks of an engine, with and without groups, computed by the oracles."""

    def __init__(self, info=0):
        self.calls, self.labels, self._info = [], [], info

    def multi_load(self, Xa, Xe, Ya, Ye, reg):
        self.calls.append("load")
        self._d, self._reg = (Xa, Xe, Ya, Ye), reg

    def multi_shapley(self, first=0, count=None, block=0):
        self.calls.append("shapley")
        return multi_oracle(*self._d, reg=self._reg), self._info

    def multi_groups_shapley(self, labels, first=0, count=None, block=0):
        assert isinstance(labels, np.ndarray) and labels.dtype == np.int32 and labels.shape == (self._d[0].shape[1],)
        self.calls.append("shapley")
        self.labels.append(labels.copy())
        return multi_group_oracle(*self._d, labels, reg=self._reg), self._info

    def multi_gram(self):
        return multi_gram_problem(*self._d, self._reg)

    def multi_free(self):
        self.calls.append("free")


@pytest.mark.parametrize("reg", [0.0, 0.1])
@pytest.mark.parametrize("kind", ["int64", "uint16", "list"])
def test_fields_shapes_and_repr(kind, reg):
    # an unsigned dtype cannot carry the baseline label
    sizes, nb = ([2, 3, 3], 0) if kind == "uint16" else ([2, 3, 1], 2)
    labels, d = grouped_data(sizes, nb, 4, seed=5)
    p, m, ng = len(labels), 4, 3
    eng = MultiGroupOracleEngine()
    res = ls_spa_multi(*d, reg, groups=labels.tolist() if kind == "list" else labels.astype(kind), _engine=eng)
    assert eng.calls == ["load", "shapley", "free"]
    assert len(eng.labels) == 1
    np.testing.assert_array_equal(eng.labels[0], labels)
    assert isinstance(res, MultiGroupResults)
    assert [f for f in res.__dataclass_fields__] == ["attribution", "theta", "r_squared", "baseline_r_squared"]
    assert res.attribution.shape == (m, ng) and res.theta.shape == (m, p)
    assert res.r_squared.shape == (m,) and res.baseline_r_squared.shape == (m,)
    theta, r2 = multi_fit(*d, reg=reg)
    np.testing.assert_allclose(res.theta, theta, rtol=0, atol=1e-12)
    np.testing.assert_allclose(res.r_squared, r2, rtol=0, atol=1e-12)
    np.testing.assert_allclose(res.baseline_r_squared, baseline_r_squared(*d, labels, reg=reg), rtol=0, atol=1e-12)
    assert np.all(res.baseline_r_squared == 0.0) == (nb == 0)
    np.testing.assert_allclose(res.attribution.sum(axis=1), res.r_squared - res.baseline_r_squared, rtol=0, atol=1e-12)
    text = repr(res)
    assert f"g = 3 groups, p = {p}, m = 4 responses" in text and "baseline" in text


def test_groups_none_still_returns_the_three_fields():
    d = multi_data(5, 4, seed=3)
    eng = MultiGroupOracleEngine()
    res = ls_spa_multi(*d, groups=None, _engine=eng)
    assert eng.calls == ["load", "shapley", "free"] and eng.labels == []
    assert isinstance(res, MultiResponseResults) and not isinstance(res, MultiGroupResults)
    assert [f for f in res.__dataclass_fields__] == ["attribution", "theta", "r_squared"]
    assert res.attribution.shape == (4, 5)


def test_not_positive_definite_warns_and_frees():
    labels, d = grouped_data([2, 1, 2], 1, 2, seed=8)
    eng = MultiGroupOracleEngine(info=1)
    with pytest.warns(RuntimeWarning, match="not numerically positive definite"):
        ls_spa_multi(*d, groups=labels, _engine=eng)
    assert eng.calls == ["load", "shapley", "free"]


def test_p36_is_taken_with_groups():
    labels, d = grouped_data([5] * 7, 1, 2, seed=36)
    assert len(labels) == 36
    res = ls_spa_multi(*d, groups=labels, _engine=MultiGroupOracleEngine())
    assert res.attribution.shape == (2, 7) and res.theta.shape == (2, 36)
    np.testing.assert_allclose(res.attribution.sum(axis=1), res.r_squared - res.baseline_r_squared, rtol=0, atol=1e-12)


# ---- refusals: all before an engine exists ---------------------------------------------------------------------------
@pytest.fixture
def no_engine(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("an engine was acquired")
    monkeypatch.setattr(_driver, "_acquire_engine", refuse)


def _zeros(p, m=3):
    z = np.zeros
    return z((2 * p + 10, p)), z((p + 10, p)), z((2 * p + 10, m)), z((p + 10, m))


@pytest.mark.parametrize("p, groups, text", [
    (40, np.minimum(np.arange(40), 32), "at most g = 32"),
    (65, np.arange(65) % 8, "at most p = 64"),
    (4, [0, 2, 2, 0], "gap in its numbering.*label 1"),
    (4, np.array([0, 3, 3, 0], dtype=np.uint8), "gap in its numbering.*label 1"),
    (4, [0, 1, 1], "length p = 4"),
    (4, [0, -2, 1, 1], "below -1"),
    (4, [-1, -1, -1, -1], "no group at all"),
    (4, [0.0, 1.0, 1.0, 0.0], "integer labels"),
])
def test_refused_before_any_engine(no_engine, p, groups, text):
    with pytest.raises(ValueError, match=text):
        ls_spa_multi(*_zeros(p), groups=groups)


def test_p33_without_groups_still_names_p32(no_engine):
    with pytest.raises(ValueError, match="at most p = 32"):
        ls_spa_multi(*_zeros(33))
    with pytest.raises(ValueError, match="at most p = 32"):
        ls_spa_multi(*_zeros(36), groups=None)
