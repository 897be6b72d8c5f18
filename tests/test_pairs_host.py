"""ls_spa_interactions_sampled: sampled pairwise Shapley interaction values -- CPU side.

The estimator itself (tests/pair_ref.py: a sample is an ordering and its two neighbour-swapped forms; every adjacent pair
of the ordering gets one second difference) against the definition of the interaction index over all d! orderings; the
host expansion of the library (csrc/host_perms.cpp through lsspa_debug_expand_pairs) against that restatement; and the
driver on a test double of the engine whose lifts are the oracle's and whose pair tables are pair_ref's."""
import itertools
from math import factorial

import numpy as np
import pytest

import lsspa_oracle as O
import ls_spa as package
import pair_ref
from ls_spa import _native
from ls_spa import ls_spa_interactions_sampled
from ls_spa._driver import pair_standard_errors, prepare_sampling
from ls_spa._engine import debug_expand_pairs
from test_group_sampling_host import PlayersOracleEngine
from test_groups_host import labels_of, value
from test_subsets_host import data, gram_problem


# ---- 1. the estimator against the definition -------------------------------------------------------------------------
@pytest.mark.parametrize("d", [5, 6])
def test_mean_over_all_orderings_is_the_interaction_index(d):
    """For a random game the mean of the samples' second differences over all d! orderings is I_ab (to 1e-14), and every
    unordered pair is adjacent in 2 (d - 1)! of them."""
    rng = np.random.default_rng(d)
    v = rng.standard_normal(1 << d)
    v[0] = 0.0
    perms = np.array(list(itertools.permutations(range(d))))
    lifts = pair_ref.game_lifts(v, pair_ref.expand(perms))
    total, count = np.zeros((d, d)), np.zeros((d, d), dtype=np.int64)
    for s, pi in enumerate(perms):
        x = pair_ref.deltas(lifts[3 * s:3 * s + 3], pi)
        for k in range(d - 1):
            a, b = pi[k], pi[k + 1]
            total[a, b] += x[k]
            total[b, a] += x[k]
            count[a, b] += 1
            count[b, a] += 1
    off = ~np.eye(d, dtype=bool)
    assert np.all(count[off] == 2 * factorial(d - 1)) and np.all(np.diag(count) == 0)
    want = pair_ref.interaction_index(v, d)
    np.testing.assert_allclose(total[off] / count[off], want[off], rtol=0, atol=1e-14)
    # the tables (Welford + Chan, two batches) say the same, and every row of a sample is a lift vector of the game
    t = pair_ref.PairTables(d).add_batch(lifts[:3 * 100], perms[:100]).add_batch(lifts[3 * 100:], perms[100:])
    np.testing.assert_array_equal(t.count, count)
    np.testing.assert_allclose(t.mean[off], want[off], rtol=0, atol=1e-13)
    np.testing.assert_allclose(lifts.sum(axis=1), v[-1], rtol=0, atol=1e-13)
    m2 = np.zeros((d, d))
    for s, pi in enumerate(perms):
        x = pair_ref.deltas(lifts[3 * s:3 * s + 3], pi)
        for k in range(d - 1):
            m2[pi[k], pi[k + 1]] += (x[k] - want[pi[k], pi[k + 1]]) ** 2
    np.testing.assert_allclose(t.m2, m2 + m2.T, rtol=0, atol=1e-11)


# ---- 2. the library's expansion --------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [2, 3, 4, 7, 8])
def test_expansion_against_the_restatement(d):
    """Fails on a library without the sampled interactions: the symbol is missing."""
    lib = _native.load()
    rng = np.random.default_rng(d)
    perms = np.array([rng.permutation(d) for _ in range(6)], dtype=np.int32)
    out = debug_expand_pairs(perms)
    assert out.shape == (18, d) and out.dtype == np.int32
    np.testing.assert_array_equal(out, pair_ref.expand(perms))
    np.testing.assert_array_equal(out[0::3], perms)
    assert lib.lsspa_debug_check_perms(_native.iptr(out), 18, d, 1) == 1       # rows 3 s + 1, 3 s + 2 are permutations
    for s, pi in enumerate(perms):
        for k in range(d - 1):      # positions k, k + 1 swapped in row 1 + (k & 1), and only there is pi[k + 1] at k
            assert out[3 * s + 1 + (k & 1)][k] == pi[k + 1] and out[3 * s + 1 + (k & 1)][k + 1] == pi[k]
    if d == 2:
        np.testing.assert_array_equal(out[2::3], perms)      # no pair (1, 2): the odd row is pi itself


def test_expansion_refuses_what_is_not_a_permutation():
    lib = _native.load()
    out = np.empty((6, 4), dtype=np.int32)
    for bad in ([0, 1, 1, 3], [0, 1, 2, 4], [0, -1, 2, 3]):
        rows = np.array([[3, 2, 1, 0], bad], dtype=np.int32)
        assert lib.lsspa_debug_expand_pairs(4, _native.iptr(rows), 2, _native.iptr(out)) == 1      # LSSPA_ERR_ARG
    with pytest.raises(ValueError):
        debug_expand_pairs([[0, 2, 2]])


# ---- 3. the driver on a test double ----------------------------------------------------------------------------------
class PairsOracleEngine(PlayersOracleEngine):
    """PlayersOracleEngine with the pair state: pairs_batch expands a batch (pair_ref), takes the oracle's lifts of the
    3 B rows -- group lifts under a player map -- and folds them into pair_ref's tables."""

    def __init__(self):
        super().__init__()
        self.tables = None
        self.pair_calls, self.states, self.enabled = [], [], []

    def set_precision(self, name):
        self.precision = name

    def set_flags(self, flags):
        pass

    def pairs_enable(self, on=True):
        self.enabled.append(bool(on))
        self.tables = pair_ref.PairTables(self.p) if on else None

    def pairs_batch(self, perms):
        perms = np.asarray(perms)
        assert self.tables is not None and perms.shape[1] == self.p
        self.pair_calls.append(len(perms))
        rows = pair_ref.expand(perms)
        if self._labels is None:
            lifts = np.array([O.ordering_lift(*self._red, self.y_norm_sq, r) for r in rows])
        else:
            lifts = self._group_lifts(rows, False)
        self.tables.add_batch(lifts, perms)

    def pairs_get(self, tables=True):
        t = self.tables
        self.states.append((t.count.copy(), t.m2.copy()))
        return t.n, t.phi, t.count.copy(), t.mean.copy(), t.m2.copy()


def stop_holds(counts, m2, tolerance):
    off = ~np.eye(len(counts), dtype=bool)
    with np.errstate(divide="ignore", invalid="ignore"):
        se = 0.5 * np.sqrt(m2[off] / (counts[off] * (counts[off] - 1.0)))
    return bool(np.all(counts[off] >= 2) and np.all(se <= tolerance))


def test_stop_rule():
    d = data(5, seed=31)
    kw = dict(batch_size=8, max_samples=400, seed=5)
    eng = PairsOracleEngine()
    free = ls_spa_interactions_sampled(*d, _engine=eng, **kw)
    assert free.n_samples == 400 and eng.pair_calls == [8] * 50 and len(eng.states) == 1     # no tolerance: one read
    worst = free.interaction_errors.max()
    eng = PairsOracleEngine()
    res = ls_spa_interactions_sampled(*d, tolerance=3.0 * worst, _engine=eng, **kw)
    assert 8 <= res.n_samples < 400 and res.n_samples % 8 == 0
    assert len(eng.states) == len(eng.pair_calls) == res.n_samples // 8                      # read once per batch
    verdicts = [stop_holds(c, q, 3.0 * worst) for c, q in eng.states]
    assert verdicts[-1] and not any(verdicts[:-1])                                           # the FIRST batch it holds at
    assert res.interaction_errors.max() <= 3.0 * worst and res.counts[~np.eye(5, dtype=bool)].min() >= 2
    eng = PairsOracleEngine()
    res = ls_spa_interactions_sampled(*d, tolerance=0.0, _engine=eng, **kw)
    assert res.n_samples == 400 and len(eng.states) == 50                                    # never met: runs out
    assert eng.enabled == [True, False] and eng._labels is None
    # the orderings are the 'random' source's, seeded
    src = prepare_sampling(5, max_samples=400, batch_size=8, seed=5, perms=None, antithetical=False, method="random")[1]
    t = pair_ref.PairTables(5)
    red, yy = O.reduce(*d, 0.0), float(d[3] @ d[3])
    perms = src.take(400)
    t.add_batch(np.array([O.ordering_lift(*red, yy, r) for r in pair_ref.expand(perms[:8])]), perms[:8])
    np.testing.assert_array_equal(eng.states[0][0], t.count)


def test_unhit_pairs_rows_and_total():
    d = data(6, seed=32)
    res = ls_spa_interactions_sampled(*d, perms=[[0, 1, 2, 3, 4, 5], [1, 0, 2, 3, 5, 4]], _engine=PairsOracleEngine())
    assert res.n_samples == 2 and res.interactions.shape == (6, 6) and res.counts.dtype == np.int64
    assert res.counts[0, 1] == 2 and res.counts[2, 3] == 2 and res.counts[1, 2] == 1 and res.counts[0, 2] == 1
    assert np.isfinite(res.interaction_errors[0, 1]) and res.interaction_errors[0, 1] >= 0
    assert res.interaction_errors[1, 2] == np.inf                      # one value: no standard error
    for a, b in ((0, 3), (0, 5), (1, 4), (2, 5)):                      # never neighbours
        assert res.counts[a, b] == res.counts[b, a] == 0
        assert res.interactions[a, b] == 0.0 and res.interaction_errors[a, b] == np.inf
    assert np.all(np.diag(res.interaction_errors) == 0) and np.all(np.diag(res.counts) == 0)
    np.testing.assert_array_equal(res.interactions, res.interactions.T)
    np.testing.assert_allclose(res.interactions.sum(axis=1), res.attribution, rtol=0, atol=1e-13)
    assert abs(res.interactions.sum() - res.r_squared) < 1e-12
    # all orderings: the exact values (index and attribution), through the driver
    prob = gram_problem(*d)
    from test_subsets_host import exact_shapley, subset_values
    v = subset_values(*prob, np.arange(1 << 6, dtype=np.uint64))
    res = ls_spa_interactions_sampled(*d, method="exact", _engine=PairsOracleEngine())
    off = ~np.eye(6, dtype=bool)
    assert res.n_samples == 720 and np.all(res.counts[off] == 240)
    np.testing.assert_allclose(res.interactions[off], 0.5 * pair_ref.interaction_index(v, 6)[off], rtol=0, atol=1e-12)
    np.testing.assert_allclose(res.attribution, exact_shapley(*prob), rtol=0, atol=1e-12)


def test_groups_are_the_players():
    labels = labels_of([2, 3, 1, 2], 2, seed=9)
    d = data(len(labels), seed=77)
    eng = PairsOracleEngine()
    res = ls_spa_interactions_sampled(*d, groups=labels, max_samples=40, batch_size=16, seed=1, _engine=eng)
    assert res.n_samples == 40 and eng.pair_calls == [16, 16, 8]
    assert res.interactions.shape == (4, 4) and res.attribution.shape == (4,) and res.theta.shape == (len(labels),)
    base = value(*gram_problem(*d), np.nonzero(labels == -1)[0])
    np.testing.assert_allclose(res.interactions.sum(axis=1), res.attribution, rtol=0, atol=1e-13)
    assert abs(res.interactions.sum() - (res.r_squared - base)) < 1e-12
    assert eng._labels is None and eng.p == len(labels) and len(eng.players_set) == 1      # the map does not outlive the call


def test_refusals_come_before_any_engine_work():
    eng = PairsOracleEngine()
    one = data(1, seed=3)
    with pytest.raises(ValueError, match="between 2 and 4096"):
        ls_spa_interactions_sampled(*one, _engine=eng)
    wide = (np.broadcast_to(np.zeros(1), (4097, 4097)), np.broadcast_to(np.zeros(1), (3, 4097)), np.zeros(4097), np.zeros(3))
    with pytest.raises(ValueError, match="between 2 and 4096"):
        ls_spa_interactions_sampled(*wide, _engine=eng)
    with pytest.raises(ValueError, match="between 2 and 4096"):
        ls_spa_interactions_sampled(*data(6, seed=1), groups=[0, 0, 0, -1, -1, 0], _engine=eng)      # one group
    with pytest.raises(ValueError, match="method must be"):
        ls_spa_interactions_sampled(*data(6, seed=1), method="subsets", _engine=eng)
    with pytest.raises(ValueError, match="either perms= or method="):
        ls_spa_interactions_sampled(*data(6, seed=1), method="argsort", perms=[[0, 1, 2, 3, 4, 5]], _engine=eng)
    for name in ("comm", "checkpoint"):
        with pytest.raises(TypeError):
            ls_spa_interactions_sampled(*data(6, seed=1), _engine=eng, **{name: None})
    assert eng.enabled == [] and eng.pair_calls == [] and eng.players_set == [] and eng.p == 0


def test_public_names_and_standard_errors():
    assert "ls_spa_interactions_sampled" in package.__all__ and "SampledInteractionResults" in package.__all__
    fields = list(package.SampledInteractionResults.__dataclass_fields__)
    assert fields == ["interactions", "attribution", "theta", "r_squared", "interaction_errors", "counts", "n_samples"]
    counts = np.array([[0, 4, 1], [4, 0, 0], [1, 0, 0]])
    m2 = np.array([[0.0, 3.0, 0.0], [3.0, 0.0, 0.0], [0.0, 0.0, 0.0]])
    err = pair_standard_errors(counts, m2)
    assert err[0, 1] == err[1, 0] == 0.5 * np.sqrt(3.0 / 12.0)
    assert err[0, 2] == np.inf and err[1, 2] == np.inf and np.all(np.diag(err) == 0)
    assert "independent samples" in ls_spa_interactions_sampled.__doc__
