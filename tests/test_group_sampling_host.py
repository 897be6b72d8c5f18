"""ls_spa_groups: sampled Shapley attribution over groups of columns -- CPU side.

The host half of the player map (the expansion of group orderings to column orderings, csrc/host_perms.cpp through the
test hook lsspa_debug_expand_groups) against NumPy, and the driver in dimension g on a test double of the engine whose
lifts are the oracle's and whose fold is NumPy's."""
import numpy as np
import pytest

import lsspa_oracle as O
from ls_spa import _native
from ls_spa import _samplers as S
from ls_spa import ls_spa, ls_spa_groups
from ls_spa._engine import debug_expand_groups
from test_groups_host import CASES, GroupsOracleEngine, group_shapley, labels_of, value
from test_subsets_host import data, gram_problem


# ---- 1. expansion --------------------------------------------------------------------------------------------------
def expand(labels, order):
    """The baseline's columns, then the columns of the groups in `order`, ascending inside a group (group_orderings of
    tests/test_groups_host.py for one ordering)."""
    labels = np.asarray(labels)
    return np.concatenate([np.nonzero(labels == -1)[0]] + [np.nonzero(labels == k)[0] for k in order])


EXPANSION_LABELS = [
    labels_of([1, 2, 3], 0, seed=1), labels_of([2, 1, 2], 2, seed=2), labels_of([3, 3, 1, 2], 1, seed=3),
    labels_of([5], 0), labels_of([4], 3, seed=4),                       # g = 1
    labels_of([1] * 7, 0, seed=5), labels_of([1] * 6, 2, seed=6),       # g = p, g = p - baseline
    labels_of([4, 1, 9, 2, 2, 7, 1, 3, 5, 6, 2], 5, seed=7),
]


@pytest.mark.parametrize("labels", EXPANSION_LABELS, ids=lambda l: f"p{len(l)}g{l.max() + 1}b{(l < 0).sum()}")
@pytest.mark.parametrize("antithetical", [False, True])
def test_expansion_against_numpy(labels, antithetical):
    lib = _native.load()
    p, g, nb = len(labels), int(labels.max()) + 1, int((labels < 0).sum())
    rng = np.random.default_rng(p * 31 + g)
    orders = np.array([rng.permutation(g) for _ in range(9)], dtype=np.int32)
    out = debug_expand_groups(labels, orders, antithetical)
    per = 2 if antithetical else 1
    assert out.shape == (9 * per, p) and out.dtype == np.int32
    assert lib.lsspa_debug_check_perms(_native.iptr(out), out.shape[0], p, 1) == 1
    for s, o in enumerate(orders):
        np.testing.assert_array_equal(out[per * s], expand(labels, o))
        if antithetical:
            back = expand(labels, o[::-1])
            # the reversed group ordering, baseline first: the groups' blocks in reversed order ...
            np.testing.assert_array_equal(labels[out[2 * s + 1]], labels[back])
            if nb:      # ... with a baseline exactly NumPy's expansion (the pair runs as two unpaired orderings),
                np.testing.assert_array_equal(out[2 * s + 1], back)
            else:       # without one the forward row read backwards (the kernels' paired form)
                np.testing.assert_array_equal(out[2 * s + 1], out[2 * s][::-1])


def test_expansion_refuses_bad_group_orderings_and_labels():
    lib = _native.load()
    labels = np.ascontiguousarray(labels_of([2, 1, 2], 2, seed=2), dtype=np.int32)
    out = np.empty((4, 7), dtype=np.int32)

    def rc(lab, g, rows):
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        return lib.lsspa_debug_expand_groups(_native.iptr(lab), len(lab), g, _native.iptr(rows), len(rows), 1,
                                             _native.iptr(out))
    assert rc(labels, 3, [[0, 1, 2], [2, 0, 1]]) == 0
    for bad in ([0, 1, 1], [0, 1, 3], [0, -1, 2]):
        assert rc(labels, 3, [[0, 1, 2], bad]) == 1, bad            # LSSPA_ERR_ARG
    assert rc(labels, 4, [[0, 1, 2, 3]]) == 1                       # group 3 has no column
    assert rc(labels, 2, [[0, 1]]) == 1                             # label 2 out of range
    assert rc(np.full(7, -1, dtype=np.int32), 0, [[0]]) == 1        # no group at all
    with pytest.raises(ValueError):
        debug_expand_groups(labels, [[0, 2, 2]], False)


# ---- 2. the driver on a test double ----------------------------------------------------------------------------------
class PlayersOracleEngine(GroupsOracleEngine):
    """GroupsOracleEngine with a player map: under set_players the orderings it is given are orderings of the groups,
    which it expands (NumPy), runs through the oracle's lifts and folds by label; its statistics, history and
    estimator then live in dimension g (the double keeps them in ``self.p``)."""

    def __init__(self):
        super().__init__()
        self._labels = None
        self.players_set = []
        self.group_perms = []

    def set_players(self, labels):
        labels = np.asarray(labels)
        assert labels.dtype == np.int32 and labels.shape == (self.p,)
        self._labels, self._cols = labels, self.p
        self.players_set.append(labels.copy())
        self.p = int(labels.max()) + 1
        self.reset_stats()

    def clear_players(self):
        if self._labels is not None:
            self.p, self._labels = self._cols, None

    def _group_lifts(self, perms, antithetical):
        lab, g = self._labels, self.p
        out = np.empty((len(perms), g))
        for s, o in enumerate(np.asarray(perms)):
            assert sorted(o) == list(range(g))
            self.group_perms.append(np.array(o))
            rows = [expand(lab, o)] + ([expand(lab, o[::-1])] if antithetical else [])
            lifts = [O.ordering_lift(*self._red, self.y_norm_sq, r) for r in rows]
            out[s] = np.mean([[l[lab == k].sum() for k in range(g)] for l in lifts], axis=0)
        return out

    def launch_batch(self, perms, antithetical):
        if self._labels is None:
            return super().launch_batch(perms, antithetical)
        assert len(self._tickets) < 2
        self.launched += 1
        self._tickets[self.launched] = self._group_lifts(perms, antithetical)
        return self.launched

    def run_batch(self, perms, antithetical, want_lifts=False, accumulate=True):
        if self._labels is None:
            return super().run_batch(perms, antithetical, want_lifts, accumulate)
        self.calls.append(len(perms))
        lifts = self._group_lifts(perms, antithetical)
        if accumulate:
            self._accumulate(lifts)
            if accumulate is not True and accumulate == 2:
                self.merge()
        return lifts if want_lifts else None


@pytest.mark.parametrize("sizes, nb", CASES)
def test_exact_method_equals_the_grouped_oracle(sizes, nb):
    labels = labels_of(sizes, nb, seed=len(sizes))
    p, g = len(labels), len(sizes)
    d = data(p, seed=20 + p)
    eng = PlayersOracleEngine()
    res = ls_spa_groups(*d, labels, method="exact", _engine=eng)
    prob = gram_problem(*d)
    np.testing.assert_allclose(res.attribution, group_shapley(*prob, labels), rtol=0, atol=1e-12)
    assert res.attribution.shape == (g,) and res.attribution_errors.shape == (g,) and res.theta.shape == (p,)
    assert len(eng.group_perms) == int(np.prod(np.arange(1, g + 1))) and eng.groups_calls == []
    base = value(*prob, np.nonzero(labels == -1)[0])
    assert abs(res.attribution.sum() - (res.r_squared - base)) < 1e-12
    ref = ls_spa(*d, method="subsets", groups=labels, _engine=GroupsOracleEngine())
    np.testing.assert_array_equal(res.theta, ref.theta)
    assert res.r_squared == ref.r_squared
    assert eng._labels is None and eng.p == p          # the map does not outlive the call


def test_antithetical_samples_and_history_in_dimension_g():
    labels = labels_of([2, 3, 1, 2], 2, seed=9)
    g = 4
    d = data(len(labels), seed=77)
    rng = np.random.default_rng(5)
    perms = np.array([rng.permutation(g) for _ in range(12)])
    eng = PlayersOracleEngine()
    res = ls_spa_groups(*d, labels, perms=perms, batch_size=4, tolerance=0.0, antithetical=True,
                        return_attribution_history=True, _engine=eng)
    red = O.reduce(*d, 0.0)
    yy = float(d[3] @ d[3])
    want = np.array([np.mean([[O.ordering_lift(*red, yy, expand(labels, o))[labels == k].sum() for k in range(g)]
                              for o in (q, q[::-1])], axis=0) for q in perms])
    np.testing.assert_allclose(res.attribution, want.mean(axis=0), rtol=0, atol=1e-12)
    assert res.attribution_history.shape == (12, g)
    np.testing.assert_allclose(res.attribution_history, np.cumsum(want, axis=0) / np.arange(1, 13)[:, None], atol=1e-12)
    with pytest.raises(ValueError):
        ls_spa_groups(*d, labels, perms=[np.arange(len(labels))], _engine=PlayersOracleEngine())   # a column ordering


def test_auto_takes_the_enumeration_when_it_is_cheap_and_argsort_above():
    labels = labels_of([3] * 20, 4, seed=1)                    # g = 20, p = 64
    d = data(64, n=200, m=150, seed=3)
    eng = PlayersOracleEngine()
    eng.groups_shapley = lambda lab: (eng.groups_calls.append(lab.copy()), (np.zeros(20), 0))[1]   # not 2^20 solves
    res = ls_spa_groups(*d, labels, _engine=eng)
    assert len(eng.groups_calls) == 1 and eng.players_set == [] and eng.launched == 0 and eng.calls == []
    assert res.attribution.shape == (20,) and res.error_history.shape == (0,)

    for labels in (labels_of([2] * 21, 3, seed=2), labels_of([13] * 5, 0, seed=3)):      # g = 21 / p = 65
        p, g = len(labels), int(labels.max()) + 1
        d = data(p, n=200, m=150, seed=4)
        eng = PlayersOracleEngine()
        res = ls_spa_groups(*d, labels, max_samples=24, batch_size=8, tolerance=0.0, seed=11, lanes=1, _engine=eng)
        assert eng.groups_calls == [] and len(eng.players_set) == 1
        want = S.ArgsortSource(g, 11, 24).take(24)
        assert len(eng.group_perms) >= 24          # (a look-ahead group may have drawn beyond the last sample)
        np.testing.assert_array_equal(np.array(eng.group_perms[:24]), want)
        assert res.attribution.shape == (g,) and res.attribution_errors.shape == (g,) and res.theta.shape == (p,)


@pytest.mark.parametrize("kw, text", [
    (dict(comm=object()), "comm="),
    (dict(checkpoint="state.npz"), "checkpoint="),
    (dict(row_sharded=True), "row_sharded="),
    (dict(method="sobol"), "method must be"),
    (dict(method="argsort", perms=np.array([[0, 1, 2]])), "either perms= or method="),
])
def test_refused_options(kw, text):
    eng = PlayersOracleEngine()
    with pytest.raises(ValueError, match=text):
        ls_spa_groups(*data(6, seed=1), [0, 0, 1, 1, 2, -1], _engine=eng, **kw)
    assert eng.players_set == [] and eng.calls == [] and eng.launched == 0


@pytest.mark.parametrize("groups, text", [([0, 1, 3, 1, 0, 0], "gap"), ([0, 1], "length p = 6"),
                                          ([-1] * 6, "no group at all")])
def test_refused_labels(groups, text):
    for method in ("auto", "argsort"):
        with pytest.raises(ValueError, match=text):
            ls_spa_groups(*data(6, seed=1), groups, method=method, _engine=PlayersOracleEngine())


def test_more_than_32_groups_are_taken():
    labels = labels_of([1] * 34 + [2], 1, seed=4)      # g = 35, p = 37
    res = ls_spa_groups(*data(37, n=120, m=90, seed=6), labels, method="random", max_samples=8, batch_size=4,
                        tolerance=0.0, _engine=PlayersOracleEngine())
    assert res.attribution.shape == (35,)
    with pytest.raises(ValueError, match="at most g = 32"):
        ls_spa_groups(*data(37, n=120, m=90, seed=6), labels, method="subsets", _engine=PlayersOracleEngine())


def test_ls_spa_itself_still_refuses_groups_with_a_sampling_method():
    with pytest.raises(ValueError, match="exact path only"):
        ls_spa(*data(4, seed=2), groups=[0, 0, 1, 1], method="argsort", _engine=PlayersOracleEngine())


# ---- 3. the stop rule runs in dimension g ----------------------------------------------------------------------------
@pytest.mark.parametrize("g, checked", [(8, False), (9, True)])
def test_error_check_is_guarded_by_the_number_of_groups(g, checked):
    sizes = [4] * (g - 1) + [40 - 4 * (g - 1)]
    labels = labels_of(sizes, 0, seed=g)
    assert len(labels) == 40 and labels.max() + 1 == g
    eng = PlayersOracleEngine()
    res = ls_spa_groups(*data(40, n=160, m=120, seed=8), labels, method="random", max_samples=32, batch_size=8,
                        tolerance=0.0, _engine=eng)
    assert (len(res.error_history) > 0) == checked
    assert res.attribution_errors.shape == (g,) and np.any(res.attribution_errors != 0) == checked
    assert sum(eng.calls) == 32
