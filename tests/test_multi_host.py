"""ls_spa_multi: the exact attribution of many responses on one design matrix -- CPU side.

The multi-response oracle is a loop of the single-response oracle of tests/test_subsets_host.py over the columns of Y;
a second form of it solves every subset once with all responses as right-hand sides (the GPU tests use it at sizes where
the loop takes minutes) and is checked against the loop here.  Then the driver's argument errors, all raised before an
engine exists, and its result contract through a test double of the engine whose enumeration is the oracle."""
from math import comb

import numpy as np
import pytest

from ls_spa import MultiResponseResults, SizeIncompatible, _driver, ls_spa_multi
from test_subsets_host import data, exact_shapley, golden, gram_problem, mask_bits, subset_values


# ---- data and oracle -------------------------------------------------------------------------------------------------
def with_responses(Xa, Xe, ya, ye, m, seed):
    """(Xa, Xe, Ya [N][m], Ye [M][m]): column 0 is the given y, the others fixed linear mixes of X columns plus noise."""
    rng = np.random.default_rng([int(seed), 7])
    p = Xa.shape[1]
    Wm = rng.standard_normal((p, max(m - 1, 0))) * (rng.random((p, max(m - 1, 0))) < 0.6)
    Ya = np.column_stack([ya, Xa @ Wm + rng.standard_normal((len(ya), m - 1))]) if m > 1 else np.asarray(ya)[:, None]
    Ye = np.column_stack([ye, Xe @ Wm + rng.standard_normal((len(ye), m - 1))]) if m > 1 else np.asarray(ye)[:, None]
    return np.asarray(Xa, dtype=np.float64), np.asarray(Xe, dtype=np.float64), Ya.astype(np.float64), Ye.astype(np.float64)


def multi_data(p, m, n=60, rows=40, seed=0):
    return with_responses(*data(p, n=n, m=rows, seed=seed), m, seed)


def multi_gram_problem(Xa, Xe, Ya, Ye, reg=0.0):
    """(G, g [m][p], H, h [m][p], yy [m]) of the reduced problem (include/lsspa.h, lsspa_multi_load)."""
    n, p = Xa.shape
    return (Xa.T @ Xa / n + reg * np.eye(p), (Xa.T @ Ya / n).T.copy(), Xe.T @ Xe, (Xe.T @ Ye).T.copy(),
            np.einsum("ir,ir->r", Ye, Ye))


def multi_oracle(Xa, Xe, Ya, Ye, reg=0.0):
    """phi [m][p]: the loop of exact_shapley(*gram_problem(...)) over the responses."""
    return np.stack([exact_shapley(*gram_problem(Xa, Xe, Ya[:, r], Ye[:, r], reg=reg)) for r in range(Ya.shape[1])])


def multi_subset_values(G, g, H, h, yy, masks):
    """v [n][m]: subset_values with every response as a right-hand side of one batched solve per subset size."""
    p = G.shape[0]
    bits = mask_bits(masks, p)
    size = bits.sum(axis=1)
    v = np.zeros((len(bits), len(yy)))
    for k in np.unique(size):
        if k == 0:
            continue
        sel = size == k
        idx = np.nonzero(bits[sel])[1].reshape(-1, k)
        Gs = G[idx[:, :, None], idx[:, None, :]]
        Hs = H[idx[:, :, None], idx[:, None, :]]
        th = np.linalg.solve(Gs, g.T[idx])                     # [n_k][k][m]
        v[sel] = (2.0 * np.einsum("nkm,nkm->nm", th, h.T[idx]) - np.einsum("nkm,nkm->nm", th, Hs @ th)) / yy
    return v


def multi_shapley_from_values(v, p):
    masks = np.arange(1 << p, dtype=np.int64)
    size = mask_bits(masks.astype(np.uint64), p).sum(axis=1)
    w = np.array([1.0 / (p * comb(p - 1, k)) for k in range(p)])
    phi = np.zeros((v.shape[1], p))
    for j in range(p):
        S_ = masks[(masks & (1 << j)) == 0]
        phi[:, j] = (w[size[S_]][:, None] * (v[S_ | (1 << j)] - v[S_])).sum(axis=0)
    return phi


def multi_oracle_batched(Xa, Xe, Ya, Ye, reg=0.0):
    prob = multi_gram_problem(Xa, Xe, Ya, Ye, reg)
    p = Xa.shape[1]
    return multi_shapley_from_values(multi_subset_values(*prob, np.arange(1 << p, dtype=np.uint64)), p)


def multi_fit(Xa, Xe, Ya, Ye, reg=0.0):
    """(theta [m][p], r_squared [m]) of the full models."""
    G, g, H, h, yy = multi_gram_problem(Xa, Xe, Ya, Ye, reg)
    theta = np.linalg.solve(G, g.T).T
    return theta, (2.0 * np.einsum("rj,rj->r", theta, h) - np.einsum("ri,ij,rj->r", theta, H, theta)) / yy


def _fixture(name, m):
    g = golden(name)
    return with_responses(g["X_train"], g["X_test"], g["y_train"], g["y_test"], m, seed=len(name)), g


# ---- the oracle ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["toy", "exact_p4", "exact_p8"])
def test_oracle_on_the_reference_fixtures(name):
    d, g = _fixture(name, 4)
    phi = multi_oracle(*d)
    np.testing.assert_allclose(phi[0], g["attribution"], rtol=0, atol=1e-12)      # column 0 is the fixture's y
    assert abs(phi[0].sum() - float(g["r_squared"])) < 1e-12
    np.testing.assert_allclose(phi.sum(axis=1), multi_fit(*d)[1], rtol=0, atol=1e-12)
    assert np.abs(phi[1:] - phi[0]).max() > 1e-3                                   # the other columns are other problems


@pytest.mark.parametrize("p, m, reg", [(1, 3, 0.0), (5, 9, 0.1), (8, 4, 0.0)])
def test_rows_sum_to_each_columns_r_squared(p, m, reg):
    d = multi_data(p, m, seed=20 + p)
    np.testing.assert_allclose(multi_oracle(*d, reg=reg).sum(axis=1), multi_fit(*d, reg=reg)[1], rtol=0, atol=1e-12)


@pytest.mark.parametrize("p, m, reg", [(1, 1, 0.0), (3, 9, 0.0), (7, 5, 0.1), (9, 3, 0.0)])
def test_batched_oracle_equals_the_loop(p, m, reg):
    d = multi_data(p, m, seed=40 + p)
    np.testing.assert_allclose(multi_oracle_batched(*d, reg=reg), multi_oracle(*d, reg=reg), rtol=0, atol=1e-13)
    prob = multi_gram_problem(*d, reg)
    masks = np.arange(1 << p, dtype=np.uint64)
    v = multi_subset_values(*prob, masks)
    for r in range(m):
        np.testing.assert_allclose(v[:, r], subset_values(prob[0], prob[1][r], prob[2], prob[3][r], prob[4][r], masks),
                                   rtol=0, atol=1e-13)


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
        ls_spa_multi(*_shapes(**kw))


def test_p33_is_refused_naming_the_limit(no_engine):
    with pytest.raises(ValueError, match="at most p = 32"):
        ls_spa_multi(*_shapes(n=40, p=33))


def test_too_many_columns_are_refused_naming_the_limit(no_engine):
    with pytest.raises(ValueError, match="p \\+ m <= 32767"):
        ls_spa_multi(*_shapes(p=4, m=32764))


@pytest.mark.parametrize("bad", ["X_train 1-D", "Y 3-D", "no responses", "no test rows"])
def test_malformed_arrays_are_refused(no_engine, bad):
    Xa, Xe, Ya, Ye = _shapes()
    if bad == "X_train 1-D":
        Xa = Xa[:, 0]
    elif bad == "Y 3-D":
        Ya, Ye = Ya[:, :, None], Ye[:, :, None]
    elif bad == "no responses":
        Ya, Ye = Ya[:, :0], Ye[:, :0]
    else:
        Xe, Ye = Xe[:0], Ye[:0]
    with pytest.raises(ValueError):
        ls_spa_multi(Xa, Xe, Ya, Ye)


# ---- the result contract through a test double --------------------------------------------------------------------
class MultiOracleEngine:
    """What ls_spa_multi asks of an engine, computed by the oracle."""

    def __init__(self, info=0):
        self.calls, self._info = [], info

    def multi_load(self, Xa, Xe, Ya, Ye, reg):
        self.calls.append("load")
        self._d, self._reg = (Xa, Xe, Ya, Ye), reg

    def multi_shapley(self, first=0, count=None, block=0):
        self.calls.append("shapley")
        return multi_oracle(*self._d, reg=self._reg), self._info

    def multi_gram(self):
        return multi_gram_problem(*self._d, self._reg)

    def multi_free(self):
        self.calls.append("free")


@pytest.mark.parametrize("reg", [0.0, 0.1])
def test_fields_and_shapes(reg):
    p, m = 5, 4
    d = multi_data(p, m, seed=3)
    eng = MultiOracleEngine()
    res = ls_spa_multi(*d, reg, _engine=eng)
    assert eng.calls == ["load", "shapley", "free"]
    assert isinstance(res, MultiResponseResults)
    assert [f for f in res.__dataclass_fields__] == ["attribution", "theta", "r_squared"]
    assert res.attribution.shape == (m, p) and res.theta.shape == (m, p) and res.r_squared.shape == (m,)
    theta, r2 = multi_fit(*d, reg=reg)
    np.testing.assert_allclose(res.theta, theta, rtol=0, atol=1e-12)
    np.testing.assert_allclose(res.r_squared, r2, rtol=0, atol=1e-12)
    np.testing.assert_allclose(res.attribution.sum(axis=1), res.r_squared, rtol=0, atol=1e-12)
    assert "m = 4 responses" in repr(res)


def test_one_dimensional_y_is_one_response():
    Xa, Xe, ya, ye = data(4, seed=6)
    res = ls_spa_multi(Xa, Xe, ya, ye, _engine=MultiOracleEngine())
    assert res.attribution.shape == (1, 4) and res.r_squared.shape == (1,)
    np.testing.assert_allclose(res.attribution[0], exact_shapley(*gram_problem(Xa, Xe, ya, ye)), rtol=0, atol=1e-13)


def test_not_positive_definite_warns_and_frees():
    eng = MultiOracleEngine(info=1)
    with pytest.warns(RuntimeWarning, match="not numerically positive definite"):
        ls_spa_multi(*multi_data(4, 2, seed=8), _engine=eng)
    assert eng.calls[-1] == "free"


def test_singular_gram_gets_the_minimal_norm_theta():
    Xa, Xe, Ya, Ye = multi_data(4, 3, seed=9)
    Xa[:, 3], Xe[:, 3] = Xa[:, 2], Xe[:, 2]                   # two identical columns: G has no Cholesky factor
    G, g, H, h, yy = multi_gram_problem(Xa, Xe, Ya, Ye)
    theta, r2, singular = _driver._multi_fit(G, g, H, h, yy)
    assert singular
    np.testing.assert_allclose(theta[:, 2], theta[:, 3], rtol=0, atol=1e-9)
    np.testing.assert_allclose(theta @ G, g, rtol=0, atol=1e-9)
