"""ls_spa_interactions(groups=labels) on the MI355X: the exact pairwise Shapley interaction values between groups of
columns (csrc/k_groups.hip, the interactions instantiation) against the CPU oracle of
tests/test_group_interactions_host.py at every layout where the decomposition into low and high groups changes form,
against the ungrouped interactions kernel for all-singleton labels, against block games and the identities of the index
where the oracle gets slow, and against a long-double truth under ill-conditioning."""
from functools import lru_cache
from math import comb

import numpy as np
import pytest

from ls_spa import InteractionResults, ls_spa, ls_spa_interactions
from test_gpu_accuracy import KAPPAS, duplicated, values_case
from test_gpu_groups import MIXED20, problem
from test_group_interactions_host import group_interactions, group_table, interactions_of_table
from test_groups_host import labels_of, shapley_of_table, value
from test_interactions_host import shap_matrix
from test_subsets_host import data, gram_problem

pytestmark = pytest.mark.gpu

ORACLE_TOL = dict(rtol=0, atol=1e-11)      # that of tests/test_gpu_subsets.py
LOW_COLS = 6                               # csrc/kernels.h, GROUPS_LOW_COLS


def layout_of(sizes):
    """(gl, ql, gh) by the layout rule: the smallest groups are low while their columns total <= 6."""
    gl = ql = 0
    for s in sorted(sizes):
        if ql + s > LOW_COLS:
            break
        gl, ql = gl + 1, ql + s
    return gl, ql, len(sizes) - gl


# name: (sizes, baseline columns, (gl, ql, gh)) -- what each covers:
SHAPES = {
    "one_group": ([4], 2, (1, 4, 0)),                       # no pair; the matrix is [[phi_0]]
    "all_low": ([1, 2, 3], 0, (3, 6, 0)),                   # one unit, low-low pairs only
    "no_low_group": ([7, 8], 0, (0, 0, 2)),                 # a single live lane, one high-high pair
    "baseline": ([2, 5, 1, 3, 4], 2, (3, 6, 2)),            # all three pair kinds beside a baseline
    "8_groups_of_3": ([3] * 8, 0, (2, 6, 6)),               # 15 high-high pairs
    "12_groups_of_5_p64": ([5] * 12, 4, (1, 5, 11)),        # p = 64; 55 high-high pairs, two waves keep high-low sums
    "16_groups_of_3": ([3] * 16, 0, (2, 6, 14)),            # 91 high-high pairs
}


def shape_problem(shape):
    sizes, nb, _ = SHAPES[shape]
    labels = labels_of(sizes, nb, seed=len(sizes))
    return labels, problem(len(labels), seed=200 + len(labels))


@lru_cache(maxsize=None)
def oracle(shape, reg):
    """(phi, raw index) of the shape's seeded problem from one table of all 2^g group values, computed once."""
    labels, d = shape_problem(shape)
    ng = len(SHAPES[shape][0])
    u, size = group_table(*gram_problem(*d, reg=reg), labels)
    phi, raw = shapley_of_table(u, ng), interactions_of_table(u, size, ng)
    for a in (phi, raw):
        a.setflags(write=False)
    return phi, raw


# ---- against the CPU oracle ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reg", [0.0, 0.1])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_against_the_cpu_oracle(engine, shape, reg):
    sizes, nb, lay = SHAPES[shape]
    assert layout_of(sizes) == lay, "the case no longer covers its edge"
    ng = len(sizes)
    labels, d = shape_problem(shape)
    want_phi, want_raw = oracle(shape, reg)
    engine.load_data(*d, reg)
    phi, raw, info = engine.groups_interactions(labels)
    phi_only, info0 = engine.groups_shapley(labels)
    assert info == info0 == 0
    print(f"{shape} reg={reg}: max |I - oracle| = {np.abs(raw - want_raw).max():.2e}, "
          f"max |phi - oracle| = {np.abs(phi - want_phi).max():.2e}")
    assert raw.shape == (ng, ng) and phi.shape == (ng,)
    np.testing.assert_allclose(raw, want_raw, **ORACLE_TOL)
    np.testing.assert_allclose(phi, want_phi, **ORACLE_TOL)
    np.testing.assert_array_equal(raw, raw.T)
    np.testing.assert_array_equal(np.diag(raw), np.zeros(ng))
    np.testing.assert_array_equal(phi, phi_only)
    res = ls_spa_interactions(*d, reg=reg, groups=labels)
    assert isinstance(res, InteractionResults)
    assert res.interactions.shape == (ng, ng) and res.theta.shape == (len(labels),)
    np.testing.assert_array_equal(res.interactions, shap_matrix(raw, phi))
    np.testing.assert_array_equal(res.attribution, phi)
    if ng == 1:
        np.testing.assert_array_equal(res.interactions, phi.reshape(1, 1))
    else:
        assert np.abs(want_raw).max() > 1e-5


# ---- two different kernels, one answer ---------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [12, 24])
def test_singletons_equal_the_ungrouped_interactions(engine, p):
    engine.load_data(*problem(p, seed=300 + p), 0.0)
    phi_s, raw_s, info_s = engine.subsets_interactions()
    phi, raw, info = engine.groups_interactions(np.arange(p))
    assert info == info_s == 0
    np.testing.assert_allclose(raw, raw_s, rtol=0, atol=1e-12)
    np.testing.assert_allclose(phi, phi_s, rtol=0, atol=1e-12)
    assert np.abs(raw_s).max() > 1e-5


# ---- g = 20, p = 64: beyond the oracle ---------------------------------------------------------------------------------
def test_identities_at_g20_p64_and_launch_bound(engine):
    """Several units and launches in play.  Exact symmetry, rows summing to the phi of groups_shapley, the total equal to
    u(all) - u(none), a permutation of the columns with their labels changing nothing, a renumbering of the groups
    permuting the matrix, two calls bitwise equal, the table accumulated over at least two launches and none of them
    longer than 0.2 s (the bound of test_gpu_groups' fact 4)."""
    labels = labels_of(MIXED20, 4, seed=20)
    p, ng = len(labels), len(MIXED20)
    assert p == 64
    Xa, Xe, ya, ye = problem(p, seed=264)
    engine.load_data(Xa, Xe, ya, ye, 0.0)
    _, r2, _ = engine.full_fit()
    phi_only, info0 = engine.groups_shapley(labels)
    phi, raw, info = engine.groups_interactions(labels)
    kernels, longest, launches = engine.groups_timing()
    print(f"g = 20, p = 64 interactions: kernels {kernels:.3f} s in {launches} launches, longest {longest * 1e3:.1f} ms")
    assert info0 == info == 0
    assert launches >= 2 and 0 < longest <= 0.2
    np.testing.assert_array_equal(phi, phi_only)
    np.testing.assert_array_equal(raw, raw.T)
    np.testing.assert_array_equal(np.diag(raw), np.zeros(ng))
    assert np.abs(raw).max() > 1e-5
    Phi = shap_matrix(raw, phi)
    np.testing.assert_allclose(Phi.sum(axis=1), phi_only, **ORACLE_TOL)
    base = value(*gram_problem(Xa, Xe, ya, ye), np.nonzero(labels == -1)[0])
    assert abs(Phi.sum() - (r2 - base)) <= 1e-11
    phi2, raw2, _ = engine.groups_interactions(labels)
    np.testing.assert_array_equal(raw2, raw)
    np.testing.assert_array_equal(phi2, phi)
    renum = np.random.default_rng(22).permutation(ng)       # group k becomes group renum[k]
    relab = np.where(labels < 0, -1, renum[np.maximum(labels, 0)])
    _, raw_r, info_r = engine.groups_interactions(relab)
    np.testing.assert_allclose(raw_r[np.ix_(renum, renum)], raw, **ORACLE_TOL)
    perm = np.random.default_rng(23).permutation(p)
    engine.load_data(Xa[:, perm], Xe[:, perm], ya, ye, 0.0)
    phi_p, raw_p, info_p = engine.groups_interactions(labels[perm])
    assert info_r == info_p == 0
    np.testing.assert_allclose(raw_p, raw, **ORACLE_TOL)
    np.testing.assert_allclose(phi_p, phi, **ORACLE_TOL)


# ---- block games over groups -------------------------------------------------------------------------------------------
def block_game(counts, size, seed):
    """A reduced problem whose G and H are block diagonal after a permutation of the columns, with counts[b] groups of
    `size` columns inside block b (the groups numbered in a seeded order): the group game is a sum of games on the
    blocks, so the index vanishes between blocks and inside a block is that of the block's own game.  Returns the
    problem, the labels and the expected raw index."""
    rng = np.random.default_rng(seed)
    ng = sum(counts)
    p = ng * size
    G, H, g, h = np.zeros((p, p)), np.zeros((p, p)), rng.standard_normal(p), rng.standard_normal(p)
    want = np.zeros((ng, ng))
    perm, gperm = rng.permutation(p), rng.permutation(ng)
    labels = np.empty(p, dtype=np.int64)
    yy = 8.0 * p
    at = gat = 0
    for nb in counts:
        idx = np.sort(perm[at:at + nb * size])
        grp = gperm[gat:gat + nb]
        at, gat = at + nb * size, gat + nb
        local = np.repeat(np.arange(nb), size)            # the block's own labels 0 .. nb-1 ...
        labels[idx] = grp[local]                          # ... and the game's
        b = len(idx)
        A, B = rng.standard_normal((3 * b + 5, b)), rng.standard_normal((3 * b + 5, b))
        sub = np.ix_(idx, idx)
        G[sub] = A.T @ A / len(A)
        H[sub] = B.T @ B
        want[np.ix_(grp, grp)] = group_interactions(G[sub], g[idx], H[sub], h[idx], yy, local)
    return (G, g, H, h, yy), labels, want


# (8, 8) x 3: g = 16, 91 pairs of high groups; (7, 7, 6) x 3: g = 20, p = 60, several launches; (9, 9, 9) x 2: g = 27 with
# 24 high groups, 276 pairs of them -- the first layout of two-column groups past the 256 pairs of a thread's first slot
@pytest.mark.parametrize("counts, size, gh", [((8, 8), 3, 14), ((7, 7, 6), 3, 18), ((9, 9, 9), 2, 24)],
                         ids=["g16", "g20", "g27_second_slot"])
def test_block_games_beyond_the_oracle(engine, counts, size, gh):
    assert layout_of([size] * sum(counts))[2] == gh
    (G, g, H, h, yy), labels, want = block_game(counts, size, seed=sum(counts))
    engine.load_reduced(G, g, float(g @ np.linalg.solve(G, g)) + 1.0, yy, H=H, h=h)
    phi, raw, info = engine.groups_interactions(labels)
    assert info == 0
    print(f"block game {counts} x {size}: max |I - blocks' oracle| = {np.abs(raw - want).max():.2e}, "
          f"kernels {engine.groups_timing()[0]:.3f} s")
    np.testing.assert_allclose(raw, want, **ORACLE_TOL)
    np.testing.assert_array_equal(raw, raw.T)
    assert np.abs(want).max() > 1e-5
    assert (want == 0).sum() >= 2 * counts[0] * counts[1]        # the pairs across blocks are asserted to vanish


# ---- accuracy under ill-conditioning, against a long-double truth --------------------------------------------------------
def truth_group_interactions(ref, labels):
    """The raw index from the long-double values of all 2^g group masks (tests/hp_ref.py), by the definition."""
    ng = int(np.max(labels)) + 1
    tab = np.array([ref.group_value(m, labels) for m in range(1 << ng)], dtype=np.longdouble)
    masks = np.arange(1 << ng, dtype=np.int64)
    size = np.array([bin(m).count("1") for m in range(1 << ng)])
    w2 = np.array([np.longdouble(1) / np.longdouble((ng - 1) * comb(ng - 2, s)) for s in range(ng - 1)])
    out = np.zeros((ng, ng))
    for k in range(ng):
        for l in range(k + 1, ng):
            bk, bl = 1 << k, 1 << l
            S_ = masks[(masks & (bk | bl)) == 0]
            out[k, l] = out[l, k] = float(np.sum(w2[size[S_]] * (tab[S_ | bk | bl] - tab[S_ | bk] - tab[S_ | bl] + tab[S_])))
    return out


@pytest.mark.parametrize("kappa", KAPPAS)
def test_sweep_groups_interactions_g10_p24(kappa):
    labels = labels_of([2] * 10, 4, seed=10)

    def call(eng):
        _, raw, info = eng.groups_interactions(labels)
        return raw, info
    values_case("groups_interactions", 24, kappa, call, lambda ref: truth_group_interactions(ref, labels),
                lambda prob: group_interactions(*prob, labels))


# ---- a failed pivot, rect mode, engine state, refusals ---------------------------------------------------------------------
@pytest.mark.parametrize("src, dup", [(3, 9), (8, 10), (1, 4)])
def test_duplicate_column_sets_the_info_bit(engine, src, dup):
    """The placements of test_duplicate_column_in_the_exact_enumerations, groups of 3 columns (two low, two high)."""
    labels = labels_of([3, 3, 3, 3], 0)
    assert labels[src] != labels[dup]
    engine.load_data(*duplicated(12, dup, src, seed=12), 0.0)
    assert engine.groups_interactions(labels)[2] & 1


def test_fewer_test_rows_than_columns(golden):
    g = golden("edge")                       # p = 12, M = 8: the test factor itself is kept (rect mode)
    d = [g[k] for k in ("X_train", "X_test", "y_train", "y_test")]
    labels = np.arange(12) // 3
    res = ls_spa_interactions(*d, groups=labels)
    u, size = group_table(*gram_problem(*d), labels)
    np.testing.assert_allclose(res.interactions,
                               shap_matrix(interactions_of_table(u, size, 4), shapley_of_table(u, 4)), **ORACLE_TOL)
    assert abs(res.interactions.sum() - res.r_squared) < 1e-11


def test_engine_state_untouched(engine):
    """The running statistics, the info word, the ungrouped enumeration's timing and result and a following sampling
    batch are what they are without a groups_interactions call in between."""
    d = data(14, n=200, m=100, seed=14)
    engine.load_data(*d, 0.0)
    engine.full_fit()
    plain, _ = engine.subsets_shapley()
    timing = engine.subsets_timing()
    perms = np.array([np.random.default_rng(s).permutation(14) for s in range(32)], dtype=np.int32)
    engine.reset_stats()
    engine.run_batch(perms[:16], False, accumulate=2)
    n0, m0, c0 = engine.stats()
    info0 = engine.info()
    engine.groups_interactions(np.arange(14) // 2)
    n1, m1, c1 = engine.stats()
    assert n0 == n1 and np.array_equal(m0, m1) and np.array_equal(c0, c1)
    assert engine.info() == info0
    assert engine.subsets_timing() == timing
    engine.run_batch(perms[16:], False, accumulate=2)
    with_call = engine.stats()
    np.testing.assert_array_equal(engine.subsets_shapley()[0], plain)
    engine.reset_stats()
    engine.run_batch(perms[:16], False, accumulate=2)
    engine.run_batch(perms[16:], False, accumulate=2)
    without = engine.stats()
    assert with_call[0] == without[0]
    np.testing.assert_array_equal(with_call[1], without[1])
    np.testing.assert_array_equal(with_call[2], without[2])


def test_kept_engine_sampling_unchanged_by_a_group_interactions_call():
    d = data(12, n=200, m=100, seed=12)
    kw = dict(method="argsort", seed=7, max_samples=512, batch_size=128, tolerance=0.0)
    before = ls_spa(*d, **kw)
    ls_spa_interactions(*d, groups=np.arange(12) // 3)
    after = ls_spa(*d, **kw)
    np.testing.assert_array_equal(before.attribution, after.attribution)
    np.testing.assert_array_equal(before.error_history, after.error_history)


@pytest.mark.parametrize("p, labels, text", [
    (40, np.minimum(np.arange(40), 32), "at most g = 32"),
    (65, np.arange(65) % 8, "at most p = 64"),
    (6, np.array([0, 0, 2, 2, -1, -1]), "no column"),
])
def test_refused_by_the_library(engine, p, labels, text):
    engine.load_data(*data(p, n=2 * p + 20, m=p + 20, seed=33), 0.0)
    with pytest.raises(ValueError, match=text):
        engine.groups_interactions(labels)
