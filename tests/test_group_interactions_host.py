"""ls_spa_interactions(groups=labels): exact pairwise Shapley interaction values between groups of columns -- CPU side.

An oracle of the index written from its definition (the four-term difference over the group subsets S without k and l, on
the table of tests/test_groups_host.group_values for all 2^g masks), vetted by the identities the index must satisfy,
against the ungrouped oracle for all-singleton labels and against the fold over subsets that the kernel uses; then the
driver's plumbing through a test double whose grouped enumeration is that oracle."""
import dataclasses
from math import comb

import numpy as np
import pytest

from ls_spa import InteractionResults, _driver, ls_spa, ls_spa_interactions
from test_groups_host import (CASES, GroupsOracleEngine, group_shapley, group_values, labels_of, schur_problem,
                              shapley_of_table)
from test_interactions_host import exact_interactions, shap_matrix
from test_subsets_host import data, exact_shapley, gram_problem

ALL_CASES = CASES + [([7, 8], 0)]


# ---- the test oracle -------------------------------------------------------------------------------------------------
def group_table(G, g, H, h, yy, labels):
    """(u of all 2^g masks, their sizes), bit k = group k."""
    ng = int(np.max(labels)) + 1
    masks = np.arange(1 << ng, dtype=np.int64)
    return group_values(G, g, H, h, yy, labels, masks), ((masks[:, None] >> np.arange(ng)) & 1).sum(axis=1)


def interactions_of_table(u, size, ng):
    """I_kl = sum over S without k, l of |S|! (g - 2 - |S|)! / (g - 1)! (u(S+k+l) - u(S+k) - u(S+l) + u(S)) from the table
    u[mask]: symmetric [g][g] with a zero diagonal."""
    out = np.zeros((ng, ng))
    if ng < 2:
        return out
    w2 = np.array([1.0 / ((ng - 1) * comb(ng - 2, s)) for s in range(ng - 1)])
    masks = np.arange(1 << ng, dtype=np.int64)
    for k in range(ng):
        for l in range(k + 1, ng):
            bk, bl = 1 << k, 1 << l
            S_ = masks[(masks & (bk | bl)) == 0]
            out[k, l] = out[l, k] = np.sum(w2[size[S_]] * (u[S_ | bk | bl] - u[S_ | bk] - u[S_ | bl] + u[S_]))
    return out


def group_interactions(G, g, H, h, yy, labels):
    """The raw interaction index between the groups of `labels`, by the definition."""
    u, size = group_table(G, g, H, h, yy, labels)
    return interactions_of_table(u, size, int(np.max(labels)) + 1)


def folded_group_interactions(G, g, H, h, yy, labels):
    """The same index by the fold over group subsets K, k = |K| (csrc/k_groups.hip):
    I_kl = T0 - T1_k - T1_l + T2_kl with weights gamma, beta + gamma, alpha + 2 beta + gamma."""
    ng = int(np.max(labels)) + 1
    u, size = group_table(G, g, H, h, yy, labels)
    w2 = lambda s: 1.0 / ((ng - 1) * comb(ng - 2, s)) if 0 <= s <= ng - 2 else 0.0
    al = np.array([w2(k - 2) for k in range(ng + 1)])[size]
    be = np.array([w2(k - 1) for k in range(ng + 1)])[size]
    ga = np.array([w2(k) for k in range(ng + 1)])[size]
    bits = ((np.arange(1 << ng)[:, None] >> np.arange(ng)) & 1).astype(bool)
    T0 = np.sum(ga * u)
    T1 = np.array([np.sum(((be + ga) * u)[bits[:, k]]) for k in range(ng)])
    out = np.zeros((ng, ng))
    for k in range(ng):
        for l in range(k + 1, ng):
            out[k, l] = out[l, k] = T0 - T1[k] - T1[l] + np.sum(((al + 2 * be + ga) * u)[bits[:, k] & bits[:, l]])
    return out


def case_problem(sizes, nb):
    labels = labels_of(sizes, nb, seed=len(sizes) + nb)
    p = len(labels)
    return gram_problem(*data(p, n=4 * p + 30, m=3 * p + 20, seed=80 + p), reg=0.05 * (p % 2)), labels


@pytest.fixture(scope="module", params=ALL_CASES, ids=[f"{'_'.join(map(str, s))}_b{b}" for s, b in ALL_CASES])
def case(request):
    sizes, nb = request.param
    prob, labels = case_problem(sizes, nb)
    return len(sizes), prob, labels, group_interactions(*prob, labels), group_shapley(*prob, labels)


def test_oracle_is_symmetric_with_a_zero_diagonal(case):
    ng, _, _, raw, _ = case
    np.testing.assert_array_equal(raw, raw.T)
    np.testing.assert_array_equal(np.diag(raw), np.zeros(ng))
    assert np.abs(raw).max() > 1e-5


@pytest.mark.parametrize("p", [1, 2, 5, 8])
def test_singleton_groups_give_the_ungrouped_index(p):
    prob = gram_problem(*data(p, seed=90 + p), reg=0.05)
    np.testing.assert_allclose(group_interactions(*prob, np.arange(p)), exact_interactions(*prob), rtol=0, atol=1e-13)


def test_the_fold_over_group_subsets_reproduces_the_definition(case):
    _, prob, labels, raw, _ = case
    np.testing.assert_allclose(folded_group_interactions(*prob, labels), raw, rtol=0, atol=1e-13)


def test_rows_sum_to_the_group_attribution_and_the_total_to_the_gain(case):
    ng, prob, labels, raw, phi = case
    Phi = shap_matrix(raw, phi)
    np.testing.assert_allclose(Phi.sum(axis=1), phi, rtol=0, atol=1e-12)
    u = group_values(*prob, labels, [0, (1 << ng) - 1])
    assert abs(Phi.sum() - (u[1] - u[0])) <= 1e-12
    np.testing.assert_array_equal(Phi, Phi.T)


def test_renumbering_the_groups_permutes_the_matrix(case):
    ng, prob, labels, raw, _ = case
    renum = np.random.default_rng(ng).permutation(ng)           # group k becomes group renum[k]
    relab = np.where(labels < 0, -1, renum[np.maximum(labels, 0)])
    got = group_interactions(*prob, relab)
    np.testing.assert_allclose(got[np.ix_(renum, renum)], raw, rtol=0, atol=1e-13)


def test_baseline_by_schur_complement_gives_the_same_matrix(case):
    _, prob, labels, raw, _ = case                  # (without a baseline the reduced problem is the problem itself)
    np.testing.assert_allclose(group_interactions(*schur_problem(*prob, labels)), raw, rtol=0, atol=1e-12)


def test_two_groups_is_the_four_term_difference():
    prob, labels = case_problem([7, 8], 0)
    u = group_values(*prob, labels, np.arange(4))
    assert abs(group_interactions(*prob, labels)[0, 1] - (u[3] - u[1] - u[2] + u[0])) < 1e-15


def test_grouping_is_not_summing_the_column_index():
    prob, labels = case_problem([1, 2, 3], 0)
    per_column = exact_interactions(*prob)
    summed = np.array([[per_column[np.ix_(labels == k, labels == l)].sum() for l in range(3)] for k in range(3)])
    np.fill_diagonal(summed, 0.0)
    assert np.abs(summed - group_interactions(*prob, labels)).max() > 1e-5


# ---- driver plumbing on a test double ----------------------------------------------------------------------------------
class GroupInteractionsOracleEngine(GroupsOracleEngine):
    """GroupsOracleEngine with both interactions entry points, computed by the oracles."""

    def __init__(self, info=0):
        super().__init__(info)
        self.group_interactions_calls = []
        self.interactions_calls = 0

    def subsets_interactions(self):
        self.interactions_calls += 1
        G, g, H, h = self.gram()
        prob = (G, g, H, h, self.y_norm_sq)
        return exact_shapley(*prob), exact_interactions(*prob), self._info

    def groups_interactions(self, labels):
        assert isinstance(labels, np.ndarray) and labels.dtype == np.int32 and labels.shape == (self.p,)
        self.group_interactions_calls.append(labels.copy())
        G, g, H, h = self.gram()
        ng = int(labels.max()) + 1
        u, size = group_table(G, g, H, h, self.y_norm_sq, labels)
        return shapley_of_table(u, ng), interactions_of_table(u, size, ng), self._info


@pytest.mark.parametrize("kind", ["int64", "int8", "list"])
def test_result_fields_and_shapes(kind):
    labels = labels_of([2, 3, 1], 2, seed=7)
    p = len(labels)
    d = data(p, seed=70)
    eng = GroupInteractionsOracleEngine()
    res = ls_spa_interactions(*d, groups=labels.tolist() if kind == "list" else labels.astype(kind), _engine=eng)
    ref = ls_spa(*d, method="subsets", groups=labels, _engine=GroupsOracleEngine())
    assert isinstance(res, InteractionResults)
    assert [f.name for f in dataclasses.fields(res)] == ["interactions", "attribution", "theta", "r_squared"]
    assert len(eng.group_interactions_calls) == 1
    assert eng.groups_calls == [] and eng.subsets_calls == 0 and eng.interactions_calls == 0
    assert eng.calls == [] and eng.launched == 0
    np.testing.assert_array_equal(eng.group_interactions_calls[0], labels)
    assert res.interactions.shape == (3, 3) and res.attribution.shape == (3,) and res.theta.shape == (p,)
    np.testing.assert_array_equal(res.attribution, ref.attribution)
    np.testing.assert_array_equal(res.theta, ref.theta)
    assert res.r_squared == ref.r_squared and isinstance(res.r_squared, float)
    prob = gram_problem(*d)
    # the double's Gram matrices come from its factors: equal to the direct ones up to rounding
    np.testing.assert_allclose(res.interactions,
                               shap_matrix(group_interactions(*prob, labels), group_shapley(*prob, labels)),
                               rtol=0, atol=1e-13)
    np.testing.assert_array_equal(res.interactions, res.interactions.T)
    np.testing.assert_allclose(res.interactions.sum(axis=1), res.attribution, rtol=0, atol=1e-14)
    u = group_values(*prob, labels, [0, 7])
    assert abs(res.interactions.sum() - (u[1] - u[0])) < 1e-12
    assert abs(res.interactions.sum() - res.r_squared) > 1e-4          # the baseline's R^2 is not attributed
    assert "p = 3" in repr(res)


def test_ridge_reaches_the_engine():
    labels = labels_of([2, 2, 3], 1, seed=3)
    d = data(len(labels), seed=6)
    res = ls_spa_interactions(*d, reg=0.3, groups=labels, _engine=GroupInteractionsOracleEngine())
    prob = gram_problem(*d, reg=0.3)
    np.testing.assert_allclose(res.interactions,
                               shap_matrix(group_interactions(*prob, labels), group_shapley(*prob, labels)),
                               rtol=0, atol=1e-13)


def test_one_group():
    labels = labels_of([4], 2, seed=1)
    d = data(6, seed=1)
    res = ls_spa_interactions(*d, groups=labels, _engine=GroupInteractionsOracleEngine())
    assert res.interactions.shape == (1, 1)
    np.testing.assert_array_equal(res.interactions, res.attribution.reshape(1, 1))


def test_more_than_32_columns_are_taken_with_groups():
    labels = labels_of([5] * 7, 5, seed=8)     # p = 40
    d = data(40, n=170, m=120, seed=72)
    eng = GroupInteractionsOracleEngine()
    res = ls_spa_interactions(*d, groups=labels, _engine=eng)
    assert res.interactions.shape == (7, 7) and res.attribution.shape == (7,) and res.theta.shape == (40,)
    assert len(eng.group_interactions_calls) == 1
    with pytest.raises(ValueError, match="at most p = 32"):
        ls_spa_interactions(*d, _engine=GroupInteractionsOracleEngine())


def test_groups_none_still_reaches_the_ungrouped_enumeration():
    d = data(7, seed=71)
    eng = GroupInteractionsOracleEngine()
    res = ls_spa_interactions(*d, groups=None, _engine=eng)
    plain_eng = GroupInteractionsOracleEngine()
    plain = ls_spa_interactions(*d, _engine=plain_eng)
    assert eng.interactions_calls == 1 and eng.group_interactions_calls == [] and eng.groups_calls == []
    assert plain_eng.interactions_calls == 1 and plain_eng.group_interactions_calls == []
    assert res.interactions.shape == (7, 7)
    np.testing.assert_array_equal(res.interactions, plain.interactions)
    assert repr(res) == repr(plain)


def _no_engine(monkeypatch):
    def no_engine(*a, **k):
        raise AssertionError("an engine was acquired")
    monkeypatch.setattr(_driver, "_acquire_engine", no_engine)


@pytest.mark.parametrize("groups, text", [
    ([0, 1, 2], "length p = 4"),
    ([0, 2, 2, 0], "gap in its numbering.*label 1"),
    ([0, -2, 1, 1], "below -1"),
    ([-1, -1, -1, -1], "no group at all"),
    ([0.0, 1.0, 1.0, 0.0], "integer labels"),
])
def test_bad_labels_refused_before_any_engine(monkeypatch, groups, text):
    _no_engine(monkeypatch)
    with pytest.raises(ValueError, match=text):
        ls_spa_interactions(*data(4, seed=1), groups=groups)


def test_g33_refused_before_any_engine(monkeypatch):
    _no_engine(monkeypatch)
    with pytest.raises(ValueError, match="at most g = 32"):
        ls_spa_interactions(*data(40, n=100, m=80, seed=1), groups=np.minimum(np.arange(40), 32))


def test_p65_refused_before_any_engine(monkeypatch):
    _no_engine(monkeypatch)
    with pytest.raises(ValueError, match="at most p = 64"):
        ls_spa_interactions(*data(65, n=140, m=100, seed=1), groups=np.arange(65) % 8)


def test_not_positive_definite_warns():
    with pytest.warns(RuntimeWarning, match="not numerically positive definite"):
        ls_spa_interactions(*data(5, seed=2), groups=[0, 0, 1, 1, 1], _engine=GroupInteractionsOracleEngine(info=1))
