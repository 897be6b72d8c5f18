"""ls_spa(method='subsets', groups=labels): exact attribution over groups of columns -- CPU side.

A naive oracle of the group game (one numpy.linalg.solve per group subset), pinned by five facts that do not involve
the GPU: all-singleton groups give the ungrouped attribution, phi is the mean over all group orderings of the summed
lifts, efficiency, invariance under relabelling, and the baseline eliminated by a Schur complement.  Then the driver's
plumbing through a test double of the engine whose grouped enumeration is that oracle."""
from itertools import permutations
from math import comb

import numpy as np
import pytest

import lsspa_oracle as O
from ls_spa import _driver
from ls_spa import _samplers as S
from ls_spa import ls_spa
from oracle_engine import OracleEngine
from test_subsets_host import data, exact_shapley, gram_problem


# ---- the grouped oracle ----------------------------------------------------------------------------------------------
def value(G, g, H, h, yy, cols):
    """v(K) of the column set K (the project's out-of-sample R^2 of the model on K); v({}) = 0."""
    cols = np.asarray(cols, dtype=np.int64)
    if len(cols) == 0:
        return 0.0
    th = np.linalg.solve(G[np.ix_(cols, cols)], g[cols])
    return float(2.0 * th @ h[cols] - th @ H[np.ix_(cols, cols)] @ th) / yy


def group_values(G, g, H, h, yy, labels, masks):
    """u(S) = v(B + columns of the groups in S) for every mask (bit k = group k), one solve per mask."""
    labels = np.asarray(labels)
    ng = int(labels.max()) + 1
    member = [np.nonzero(labels == k)[0] for k in range(ng)]
    base = np.nonzero(labels == -1)[0]
    out = np.empty(len(masks))
    for i, m in enumerate(masks):
        m = int(m)
        cols = np.concatenate([base] + [member[k] for k in range(ng) if (m >> k) & 1])
        out[i] = value(G, g, H, h, yy, np.sort(cols))
    return out


def shapley_of_table(u, ng):
    """phi_k = sum over S without k of |S|! (g - 1 - |S|)! / g! (u(S + k) - u(S)) from the table u[mask]."""
    masks = np.arange(1 << ng, dtype=np.int64)
    size = ((masks[:, None] >> np.arange(ng)) & 1).sum(axis=1)
    w = np.array([1.0 / (ng * comb(ng - 1, k)) for k in range(ng)])
    phi = np.zeros(ng)
    for k in range(ng):
        S_ = masks[(masks >> k) & 1 == 0]
        phi[k] = np.sum(w[size[S_]] * (u[S_ | (1 << k)] - u[S_]))
    return phi


def group_shapley(G, g, H, h, yy, labels):
    ng = int(np.max(labels)) + 1
    return shapley_of_table(group_values(G, g, H, h, yy, labels, np.arange(1 << ng)), ng)


def schur_problem(G, g, H, h, yy, labels):
    """The baseline eliminated on both sides: (G', g', H', h', yy, labels of the remaining columns), whose group game
    without a baseline differs from the original one by the constant v(B)."""
    labels = np.asarray(labels)
    B, S_ = np.nonzero(labels == -1)[0], np.nonzero(labels >= 0)[0]
    W = np.linalg.solve(G[np.ix_(B, B)], G[np.ix_(B, S_)])
    t0 = np.linalg.solve(G[np.ix_(B, B)], g[B])
    G2 = G[np.ix_(S_, S_)] - G[np.ix_(S_, B)] @ W
    g2 = g[S_] - G[np.ix_(S_, B)] @ t0
    H2 = H[np.ix_(S_, S_)] - W.T @ H[np.ix_(B, S_)] - H[np.ix_(S_, B)] @ W + W.T @ H[np.ix_(B, B)] @ W
    h2 = h[S_] - W.T @ h[B] - (H[np.ix_(S_, B)] - W.T @ H[np.ix_(B, B)]) @ t0
    return G2, g2, H2, h2, yy, labels[S_]


def labels_of(sizes, baseline=0, seed=None):
    """Labels of groups with the given sizes and `baseline` columns of label -1; shuffled if a seed is given."""
    lab = np.concatenate([np.full(baseline, -1)] + [np.full(s, k) for k, s in enumerate(sizes)]).astype(np.int64)
    if seed is not None:
        np.random.default_rng(seed).shuffle(lab)
    return lab


def group_orderings(labels):
    """All g! orderings of the groups, each expanded to an ordering of the columns: the baseline first, then the groups'
    columns contiguously.  Returns the orderings [g!][p]."""
    labels = np.asarray(labels)
    ng = int(labels.max()) + 1
    base = np.nonzero(labels == -1)[0]
    member = [np.nonzero(labels == k)[0] for k in range(ng)]
    return np.array([np.concatenate([base] + [member[k] for k in o]) for o in permutations(range(ng))])


CASES = [([1, 2, 3], 0), ([2, 1, 2], 2), ([3, 3, 1, 2], 1), ([1, 1, 4], 3)]


# ---- facts 1-5 on the oracle -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [1, 3, 7])
def test_fact1_singletons_equal_the_ungrouped_attribution(p):
    prob = gram_problem(*data(p, seed=p), reg=0.05)
    np.testing.assert_allclose(group_shapley(*prob, np.arange(p)), exact_shapley(*prob), rtol=0, atol=1e-13)


@pytest.mark.parametrize("sizes, nb", CASES)
def test_fact2_mean_over_group_orderings_of_the_summed_lifts(sizes, nb):
    labels = labels_of(sizes, nb, seed=len(sizes))
    p = len(labels)
    d = data(p, seed=20 + p)
    prob = gram_problem(*d, reg=0.1)
    red = O.reduce(*d, 0.1)
    orders = group_orderings(labels)
    total = np.zeros(len(sizes))
    for o in orders:
        lift = O.ordering_lift(*red, prob[4], o)
        total += np.array([lift[labels == k].sum() for k in range(len(sizes))])
    np.testing.assert_allclose(group_shapley(*prob, labels), total / len(orders), rtol=0, atol=1e-13)


@pytest.mark.parametrize("sizes, nb", CASES + [([2] * 8, 0), ([3] * 6, 4)])
def test_fact3_efficiency(sizes, nb):
    labels = labels_of(sizes, nb, seed=1)
    prob = gram_problem(*data(len(labels), n=120, m=80, seed=30), reg=0.0)
    phi = group_shapley(*prob, labels)
    full = value(*prob, np.arange(len(labels)))
    base = value(*prob, np.nonzero(labels == -1)[0])
    assert abs(phi.sum() - (full - base)) < 1e-13
    if nb == 0:
        assert base == 0.0


def test_fact4_relabelling():
    labels = labels_of([2, 3, 1, 2], 2, seed=4)
    p = len(labels)
    Xa, Xe, ya, ye = data(p, seed=40)
    phi = group_shapley(*gram_problem(Xa, Xe, ya, ye), labels)
    perm = np.random.default_rng(41).permutation(p)
    np.testing.assert_allclose(group_shapley(*gram_problem(Xa[:, perm], Xe[:, perm], ya, ye), labels[perm]), phi,
                               rtol=0, atol=1e-13)
    renum = np.array([2, 0, 3, 1])              # group k becomes group renum[k]
    relab = np.where(labels < 0, -1, renum[np.maximum(labels, 0)])
    got = group_shapley(*gram_problem(Xa, Xe, ya, ye), relab)
    np.testing.assert_allclose(got[renum], phi, rtol=0, atol=1e-13)


@pytest.mark.parametrize("sizes, nb", [c for c in CASES if c[1]] + [([2] * 7, 5)])
def test_fact5_baseline_by_schur_complement(sizes, nb):
    labels = labels_of(sizes, nb, seed=5)
    prob = gram_problem(*data(len(labels), n=150, m=90, seed=50), reg=0.02)
    red = schur_problem(*prob, labels)
    assert (red[5] >= 0).all() and len(red[1]) == len(labels) - nb
    np.testing.assert_allclose(group_shapley(*red), group_shapley(*prob, labels), rtol=0, atol=1e-13)
    ng = len(sizes)
    u = group_values(*prob, labels, np.arange(1 << ng))
    np.testing.assert_allclose(group_values(*red[:5], red[5], np.arange(1 << ng)), u - u[0], rtol=0, atol=1e-13)


def test_summing_per_column_attributions_is_a_different_quantity():
    labels = labels_of([3, 2, 1])
    prob = gram_problem(*data(6, seed=60))
    per_column = exact_shapley(*prob)
    summed = np.array([per_column[labels == k].sum() for k in range(3)])
    assert np.abs(summed - group_shapley(*prob, labels)).max() > 1e-4


def test_oracle_takes_g12_p64_in_seconds():
    import time
    labels = labels_of([5] * 12, 4, seed=6)
    prob = gram_problem(*data(64, n=256, m=192, seed=64))
    t = time.perf_counter()
    phi = group_shapley(*prob, labels)
    assert np.isfinite(phi).all() and time.perf_counter() - t < 60


# ---- driver plumbing on a test double ----------------------------------------------------------------------------------
class GroupsOracleEngine(OracleEngine):
    """OracleEngine with both enumeration entry points, computed by the oracles."""

    def __init__(self, info=0):
        super().__init__()
        self.subsets_calls = 0
        self.groups_calls = []
        self._info = info

    def subsets_shapley(self):
        self.subsets_calls += 1
        G, g, H, h = self.gram()
        return exact_shapley(G, g, H, h, self.y_norm_sq), self._info

    def groups_shapley(self, labels):
        assert isinstance(labels, np.ndarray) and labels.dtype == np.int32 and labels.shape == (self.p,)
        self.groups_calls.append(labels.copy())
        G, g, H, h = self.gram()
        return group_shapley(G, g, H, h, self.y_norm_sq, labels), self._info


@pytest.mark.parametrize("kind", ["int64", "int8", "uint16", "list"])
def test_result_fields(kind):
    # an unsigned dtype cannot carry the baseline label
    labels = labels_of([2, 3, 3], 0, seed=7) if kind == "uint16" else labels_of([2, 3, 1], 2, seed=7)
    p = len(labels)
    d = data(p, seed=70)
    eng = GroupsOracleEngine()
    groups = labels.tolist() if kind == "list" else labels.astype(kind)
    res = ls_spa(*d, method="subsets", groups=groups, _engine=eng)
    ref = ls_spa(*d, method="subsets", _engine=GroupsOracleEngine())
    assert len(eng.groups_calls) == 1 and eng.subsets_calls == 0
    np.testing.assert_array_equal(eng.groups_calls[0], labels)
    assert res.attribution.shape == (3,) and res.theta.shape == (p,)
    # the double's Gram matrices come from its factors: equal to the direct ones up to rounding
    np.testing.assert_allclose(res.attribution, group_shapley(*gram_problem(*d), labels), rtol=0, atol=1e-13)
    np.testing.assert_array_equal(res.theta, ref.theta)
    assert res.r_squared == ref.r_squared
    assert res.overall_error == 0.0 and isinstance(res.overall_error, float)
    np.testing.assert_array_equal(res.attribution_errors, np.zeros(3))
    assert res.error_history.shape == (0,)
    assert res.attribution_history is None


def test_groups_none_reaches_the_ungrouped_enumeration():
    d = data(7, seed=71)
    eng = GroupsOracleEngine()
    res = ls_spa(*d, method="subsets", groups=None, _engine=eng)
    assert eng.subsets_calls == 1 and eng.groups_calls == []
    assert res.attribution.shape == (7,) and res.attribution_errors.shape == (7,)
    np.testing.assert_array_equal(res.attribution, ls_spa(*d, method="subsets", _engine=GroupsOracleEngine()).attribution)


def test_more_than_32_columns_are_taken_with_groups():
    labels = labels_of([5] * 7, 1, seed=8)     # p = 36
    d = data(36, n=150, m=110, seed=72)
    res = ls_spa(*d, method="subsets", groups=labels, _engine=GroupsOracleEngine())
    assert res.attribution.shape == (7,) and res.theta.shape == (36,)
    with pytest.raises(ValueError, match="at most p = 32"):
        ls_spa(*d, method="subsets", _engine=GroupsOracleEngine())


@pytest.mark.parametrize("groups, text", [
    ([0, 1, 2], "length p = 4"),
    ([[0, 1], [1, 0]], "length p = 4"),
    ([0, 1, 3, 1], "gap in its numbering.*label 2"),
    ([1, 1, 2, 2], "gap in its numbering.*label 0"),
    ([0, -2, 1, 1], "below -1"),
    ([-1, -1, -1, -1], "no group at all"),
    ([0.0, 1.0, 1.0, 0.0], "integer labels"),
    ([0, 1, 1.5, 0], "integer labels"),
    ([True, False, True, False], "integer labels"),
])
def test_refused_labels(groups, text):
    eng = GroupsOracleEngine()
    with pytest.raises(ValueError, match=text):
        ls_spa(*data(4, seed=2), method="subsets", groups=groups, _engine=eng)
    assert eng.groups_calls == [] and eng.subsets_calls == 0


@pytest.mark.parametrize("kw", [
    dict(), dict(method=None), dict(method="exact"), dict(method="random"), dict(method="argsort"),
    dict(method="permutohedron"), dict(perms=np.array([[0, 1, 2, 3]])),
    dict(method="subsets", perms=np.array([[0, 1, 2, 3]])),
])
def test_groups_exist_for_the_exact_path_only(kw):
    eng = GroupsOracleEngine()
    with pytest.raises(ValueError, match="exact path only"):
        ls_spa(*data(4, seed=2), groups=[0, 0, 1, 1], _engine=eng, **kw)
    assert eng.calls == [] and eng.launched == 0 and eng.groups_calls == []


@pytest.mark.parametrize("kw, text", [
    (dict(return_attribution_history=True), "history"),
    (dict(return_history=True), "history"),
    (dict(checkpoint="state.npz"), "checkpoint"),
])
def test_refused_options(kw, text):
    eng = GroupsOracleEngine()
    with pytest.raises(ValueError, match=text):
        ls_spa(*data(4, seed=1), method="subsets", groups=[0, 0, 1, -1], _engine=eng, **kw)
    assert eng.groups_calls == []


def _no_engine(monkeypatch):
    def no_engine(*a, **k):
        raise AssertionError("an engine was acquired")
    monkeypatch.setattr(_driver, "_acquire_engine", no_engine)


def test_g33_refused_before_any_engine(monkeypatch):
    _no_engine(monkeypatch)
    with pytest.raises(ValueError, match="at most g = 32"):
        ls_spa(*data(40, n=100, m=80, seed=1), method="subsets", groups=np.minimum(np.arange(40), 32))


def test_p65_refused_before_any_engine(monkeypatch):
    _no_engine(monkeypatch)
    with pytest.raises(ValueError, match="at most p = 64"):
        ls_spa(*data(65, n=140, m=100, seed=1), method="subsets", groups=np.arange(65) % 8)


def test_bad_labels_refused_before_any_engine(monkeypatch):
    _no_engine(monkeypatch)
    with pytest.raises(ValueError, match="gap"):
        ls_spa(*data(4, seed=1), method="subsets", groups=[0, 2, 2, 0])


def test_no_sampler_is_built(monkeypatch):
    def forbidden(*a, **k):
        raise AssertionError("a sampler was built")
    for name in ("exact_source", "RandomSource", "ArgsortSource", "PermutohedronSource", "PrefetchedSource"):
        monkeypatch.setattr(S, name, forbidden)
    monkeypatch.setattr(S.NativeArgsortSource, "make", staticmethod(forbidden))
    monkeypatch.setattr(_driver, "prepare_sampling", forbidden)
    monkeypatch.setattr(_driver, "run_estimator", forbidden)
    eng = GroupsOracleEngine()
    ls_spa(*data(10, seed=5), method="subsets", groups=np.arange(10) // 3 - 1, _engine=eng)
    assert len(eng.groups_calls) == 1 and eng.calls == [] and eng.launched == 0


def test_kept_engine_back_to_float64():
    class Float32Engine(GroupsOracleEngine):
        precision = "float32"

        def set_precision(self, dtype):
            self.precision = np.dtype(dtype).name

        def full_fit(self):
            assert self.precision == "float64", "full fit with fp32 factorisation"
            return super().full_fit()

    eng = Float32Engine()
    ls_spa(*data(6, seed=3), method="subsets", groups=[0, 0, 1, 1, -1, 2], precision="float32", _engine=eng)
    assert eng.precision == "float64"


def test_not_positive_definite_warns():
    with pytest.warns(RuntimeWarning, match="not numerically positive definite"):
        ls_spa(*data(5, seed=2), method="subsets", groups=[0, 0, 1, 1, 1], _engine=GroupsOracleEngine(info=1))
