"""ls_spa_interactions on the MI355X: the exact pairwise Shapley interaction values from the enumeration of all 2^p
feature subsets (csrc/k_subsets.hip, the interactions instantiation) against the CPU oracle of
tests/test_interactions_host.py at every size where the decomposition into low and high features changes shape, against
the identities of the index where the oracle gets slow, and against a long-double truth under ill-conditioning."""
from functools import lru_cache
from math import comb

import numpy as np
import pytest

from ls_spa import InteractionResults, ls_spa, ls_spa_interactions
from ls_spa._engine import HipEngine
from test_gpu_accuracy import KAPPAS, duplicated, values_case
from test_interactions_host import exact_interactions, shap_matrix
from test_subsets_host import data, exact_shapley, gram_problem

pytestmark = pytest.mark.gpu

ORACLE_TOL = dict(rtol=0, atol=1e-11)      # that of tests/test_gpu_subsets.py


def _arrays(g):
    return [g[k] for k in ("X_train", "X_test", "y_train", "y_test")]


def _data(p, seed_base=300):
    return data(p, n=max(60, 3 * p), m=max(40, 2 * p), seed=seed_base + p)


@lru_cache(maxsize=None)
def oracle(p, reg):
    """(phi, raw index, SHAP matrix) of the seeded problem of size p, computed once."""
    prob = gram_problem(*_data(p), reg=reg)
    phi, raw = exact_shapley(*prob), exact_interactions(*prob)
    for a in (phi, raw):
        a.setflags(write=False)
    return phi, raw, shap_matrix(raw, phi)


# ---- against the CPU oracle ------------------------------------------------------------------------------------------
# p = 1: no pairs; 2: the smallest pair; 5: all features low, q < 6; 6: no high feature; 7: one high feature, high-low
# pairs only; 8: the first high-high pair; 14: 28 high pairs, one slot a lane; 16: 45 high pairs
@pytest.mark.parametrize("reg", [0.0, 0.1])
@pytest.mark.parametrize("p", [1, 2, 5, 6, 7, 8, 14, 16])
def test_against_the_cpu_oracle(engine, p, reg):
    phi, raw, Phi = oracle(p, reg)
    engine.load_data(*_data(p), reg)
    got_phi, got_raw, info = engine.subsets_interactions()
    assert info == 0
    np.testing.assert_allclose(got_raw, raw, **ORACLE_TOL)
    np.testing.assert_allclose(got_phi, phi, **ORACLE_TOL)
    np.testing.assert_array_equal(got_raw, got_raw.T)
    np.testing.assert_array_equal(np.diag(got_raw), np.zeros(p))
    res = ls_spa_interactions(*_data(p), reg=reg)
    assert isinstance(res, InteractionResults) and res.interactions.shape == (p, p)
    np.testing.assert_allclose(res.interactions, Phi, **ORACLE_TOL)
    np.testing.assert_array_equal(res.attribution, got_phi)
    if p == 1:
        np.testing.assert_array_equal(res.interactions, res.attribution.reshape(1, 1))


# ---- against the identities of the index -----------------------------------------------------------------------------
def identities(engine, p, seed):
    """Symmetry (exact), rows summing to the phi of subsets_shapley, the total equal to r_squared, and a column
    permutation of the data permuting the matrix; returns the raw index."""
    Xa, Xe, ya, ye = data(p, n=300, m=200, seed=seed)
    engine.load_data(Xa, Xe, ya, ye, 0.0)
    _, r2, _ = engine.full_fit()
    phi_only, info0 = engine.subsets_shapley()
    phi, raw, info = engine.subsets_interactions()
    assert info0 == info == 0
    np.testing.assert_array_equal(phi, phi_only)
    np.testing.assert_array_equal(raw, raw.T)
    res = ls_spa_interactions(Xa, Xe, ya, ye)
    Phi = res.interactions
    np.testing.assert_array_equal(Phi, Phi.T)
    np.testing.assert_allclose(Phi.sum(axis=1), phi_only, **ORACLE_TOL)
    assert abs(Phi.sum() - res.r_squared) <= 1e-11 and abs(res.r_squared - r2) <= 1e-12
    np.testing.assert_allclose(Phi, shap_matrix(raw, phi_only), **ORACLE_TOL)
    perm = np.random.default_rng(p).permutation(p)
    engine.load_data(Xa[:, perm], Xe[:, perm], ya, ye, 0.0)
    phi_p, raw_p, info_p = engine.subsets_interactions()
    assert info_p == 0
    np.testing.assert_allclose(raw_p, raw[np.ix_(perm, perm)], **ORACLE_TOL)
    np.testing.assert_allclose(phi_p, phi[perm], **ORACLE_TOL)
    assert np.abs(raw).max() > 1e-5
    return raw


# p = 18: 66 pairs of high features, the second accumulator slot of a lane; p = 20: 2^14 high subsets on 8192 units,
# two per unit
@pytest.mark.parametrize("p", [18, 20])
def test_identities(engine, p):
    identities(engine, p, seed=400 + p)


def test_p27_two_launches(engine):
    """2^21 high subsets, 256 per unit, above the 128 steps of one launch: the table accumulates over two launches."""
    p = 27
    identities(engine, p, seed=427)
    assert engine.subsets_timing()[2] == 2
    first = engine.subsets_interactions()
    again = engine.subsets_interactions()
    np.testing.assert_array_equal(first[0], again[0])
    np.testing.assert_array_equal(first[1], again[1])


def block_game(sizes, seed):
    """A reduced problem whose G and H are block diagonal after a permutation of the features: the game is a sum of
    games on the blocks, so the index vanishes between blocks and inside a block is that of the block's own game (the
    other features are dummies there), as is phi.  Returns the problem, the expected raw index and the expected phi."""
    rng = np.random.default_rng(seed)
    p = sum(sizes)
    G, H, g, h = np.zeros((p, p)), np.zeros((p, p)), rng.standard_normal(p), rng.standard_normal(p)
    want, want_phi = np.zeros((p, p)), np.zeros(p)
    perm = rng.permutation(p)
    yy = 8.0 * p
    at = 0
    for b in sizes:
        idx = perm[at:at + b]
        at += b
        A, B = rng.standard_normal((3 * b + 5, b)), rng.standard_normal((3 * b + 5, b))
        G[np.ix_(idx, idx)] = A.T @ A / len(A)
        H[np.ix_(idx, idx)] = B.T @ B
        sub = np.ix_(idx, idx)
        want[sub] = exact_interactions(G[sub], g[idx], H[sub], h[idx], yy)
        want_phi[idx] = exact_shapley(G[sub], g[idx], H[sub], h[idx], yy)
    return (G, g, H, h, yy), want, want_phi


@pytest.mark.parametrize("sizes", [(9, 9), (8, 7, 5), (9, 9, 9)], ids=["p18", "p20", "p27"])
def test_block_games_beyond_the_oracle(engine, sizes):
    """Every pair checked at p = 18, 20 and 27 -- second slot, two subsets a unit, two launches -- at the price of three
    small oracles."""
    (G, g, H, h, yy), want, want_phi = block_game(sizes, seed=sum(sizes))
    engine.load_reduced(G, g, float(g @ np.linalg.solve(G, g)) + 1.0, yy, H=H, h=h)
    phi, raw, info = engine.subsets_interactions()
    assert info == 0
    np.testing.assert_allclose(raw, want, **ORACLE_TOL)
    np.testing.assert_allclose(phi, want_phi, **ORACLE_TOL)
    assert np.abs(want).max() > 1e-5 and np.abs(want_phi).max() > 1e-3


@pytest.mark.parametrize("p", [9, 20, 27])
def test_phi_is_bitwise_that_of_subsets_shapley(engine, p):
    engine.load_data(*data(p, n=300, m=200, seed=500 + p), 0.0)
    phi_only, _ = engine.subsets_shapley()
    phi, _, _ = engine.subsets_interactions()
    np.testing.assert_array_equal(phi, phi_only)


# ---- the public call ---------------------------------------------------------------------------------------------------
def test_result_is_that_of_the_subsets_method():
    d = _data(9)
    res = ls_spa_interactions(*d, reg=0.1)
    ref = ls_spa(*d, reg=0.1, method="subsets")
    np.testing.assert_array_equal(res.attribution, ref.attribution)
    np.testing.assert_array_equal(res.theta, ref.theta)
    assert res.r_squared == ref.r_squared


def test_fewer_test_rows_than_features(golden):
    d = _arrays(golden("edge"))               # p = 12, M = 8: the test factor itself is kept (rect mode)
    res = ls_spa_interactions(*d)
    prob = gram_problem(*d)
    np.testing.assert_allclose(res.interactions, shap_matrix(exact_interactions(*prob), exact_shapley(*prob)),
                               **ORACLE_TOL)
    assert abs(res.interactions.sum() - res.r_squared) < 1e-11


def test_float32_inputs():
    d = [a.astype(np.float32) for a in data(11, seed=9)]
    res = ls_spa_interactions(*d)
    prob = gram_problem(*d)
    np.testing.assert_allclose(res.interactions, shap_matrix(exact_interactions(*prob), exact_shapley(*prob)),
                               **ORACLE_TOL)


def test_kept_engine_float32_then_interactions():
    d = data(14, n=300, m=150, seed=140)
    ls_spa(*d, method="argsort", seed=1, max_samples=256, batch_size=128, tolerance=0.0, precision="float32")
    after = ls_spa_interactions(*d)
    fresh_engine = HipEngine(0)
    try:
        fresh = ls_spa_interactions(*d, _engine=fresh_engine)
    finally:
        fresh_engine.close()
    np.testing.assert_array_equal(after.interactions, fresh.interactions)
    np.testing.assert_array_equal(after.theta, fresh.theta)
    assert after.r_squared == fresh.r_squared


def test_engine_state_untouched(engine):
    """The running statistics, the info word and the flags of the sampling path survive an interactions call."""
    d = data(14, n=200, m=100, seed=14)
    engine.load_data(*d, 0.0)
    engine.full_fit()
    perms = np.array([np.random.default_rng(s).permutation(14) for s in range(32)], dtype=np.int32)
    engine.reset_stats()
    engine.run_batch(perms[:16], False, accumulate=2)
    n0, m0, c0 = engine.stats()
    info0 = engine.info()
    engine.subsets_interactions()
    n1, m1, c1 = engine.stats()
    assert n0 == n1 and np.array_equal(m0, m1) and np.array_equal(c0, c1)
    assert engine.info() == info0
    engine.run_batch(perms[16:], False, accumulate=2)
    with_sub = engine.stats()
    engine.reset_stats()
    engine.run_batch(perms[:16], False, accumulate=2)
    engine.run_batch(perms[16:], False, accumulate=2)
    without = engine.stats()
    assert with_sub[0] == without[0]
    np.testing.assert_array_equal(with_sub[1], without[1])
    np.testing.assert_array_equal(with_sub[2], without[2])


def test_kept_engine_sampling_unchanged_by_an_interactions_call():
    d = data(12, n=200, m=100, seed=12)
    kw = dict(method="argsort", seed=7, max_samples=512, batch_size=128, tolerance=0.0)
    before = ls_spa(*d, **kw)
    ls_spa_interactions(*d)
    after = ls_spa(*d, **kw)
    np.testing.assert_array_equal(before.attribution, after.attribution)
    np.testing.assert_array_equal(before.error_history, after.error_history)


def test_p33_refused_by_the_library(engine):
    engine.load_data(*data(33, n=80, m=60, seed=33), 0.0)
    with pytest.raises(ValueError, match="at most p = 32"):
        engine.subsets_interactions()


# ---- accuracy under ill-conditioning, against a long-double truth --------------------------------------------------------
def truth_interactions(ref):
    """The raw index from the long-double values of all 2^p masks (tests/hp_ref.py), by the definition."""
    p = ref.p
    tab = np.array([ref.mask_value(m) for m in range(1 << p)], dtype=np.longdouble)
    masks = np.arange(1 << p, dtype=np.int64)
    size = np.array([bin(m).count("1") for m in range(1 << p)])
    w2 = np.array([np.longdouble(1) / np.longdouble((p - 1) * comb(p - 2, s)) for s in range(p - 1)])
    out = np.zeros((p, p))
    for i in range(p):
        for j in range(i + 1, p):
            bi, bj = 1 << i, 1 << j
            S_ = masks[(masks & (bi | bj)) == 0]
            out[i, j] = out[j, i] = float(np.sum(w2[size[S_]] * (tab[S_ | bi | bj] - tab[S_ | bi] - tab[S_ | bj] + tab[S_])))
    return out


@pytest.mark.parametrize("kappa", KAPPAS)
def test_sweep_interactions_p10(kappa):
    def call(eng):
        _, raw, info = eng.subsets_interactions()
        return raw, info
    values_case("subsets_interactions", 10, kappa, call, truth_interactions, lambda prob: exact_interactions(*prob))


# ---- a failed pivot ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("src, dup", [(3, 9), (8, 10), (1, 4)])
def test_duplicate_column_sets_the_info_bit(engine, src, dup):
    """The cases of test_duplicate_column_in_the_exact_enumerations: the duplicate low-high, high-high and low-low."""
    engine.load_data(*duplicated(12, dup, src, seed=12), 0.0)
    assert engine.subsets_interactions()[2] & 1
