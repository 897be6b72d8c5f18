"""ls_spa_multi(groups=labels) on the MI355X: the exact attribution of many responses over groups of columns
(csrc/k_multi_groups.hip) against the batched CPU oracle of tests/test_multi_groups_host.py, against the one-response
grouped kernel and the ungrouped many-response kernel, and the bitwise facts that make a response's row independent of
its place, its neighbours and the way a run is cut."""
import functools
import warnings

import numpy as np
import pytest

from ls_spa import MultiGroupResults, ls_spa, ls_spa_multi
from ls_spa._engine import HipEngine
from test_groups_host import group_values, labels_of
from test_multi_groups_host import baseline_r_squared, multi_group_oracle
from test_multi_host import multi_fit, multi_gram_problem, with_responses
from test_subsets_host import data

pytestmark = pytest.mark.gpu

ORACLE_TOL = dict(rtol=0, atol=1e-11)     # tests/test_gpu_subsets.py, tests/test_gpu_groups.py
RB = HipEngine.MULTI_RB

MIXED20 = [1, 2, 3, 4, 4, 3, 2, 1, 4, 4, 3, 3, 2, 4, 4, 1, 4, 4, 3, 4]      # 20 groups, 60 columns (test_gpu_groups.py)
SHAPES = {                                  # sizes, baseline columns, responses
    "sizes_1_2_3_one_response": ([1, 2, 3], 0, 1),                 # every group low, gh = 0
    "8_groups_of_3_one_chunk": ([3] * 8, 0, 8),                    # gl = 2, ql = 6, one full chunk
    "no_low_group": ([7, 8, 9], 2, 3),                             # ql = 0
    "p36_chunk_edge": ([5] * 7, 1, 9),                             # p = 36 > 32, 8 + 1 responses
    "p54_two_chunks": ([5] * 10, 4, 11),
    "singletons_p12_three_chunks": ([1] * 12, 0, 17),
}


def problem(labels, m, seed):
    p = len(labels)
    return with_responses(*data(p, n=4 * p + 8, m=3 * p + 5, seed=seed), m, seed)


@functools.lru_cache(maxsize=None)
def _case(shape, reg):
    """Labels, data and the oracle's (phi, theta, r2, baseline r2) of a shape, computed once and left unchanged."""
    sizes, nb, m = SHAPES[shape]
    labels = labels_of(sizes, nb, seed=len(sizes))
    d = problem(labels, m, seed=600 + len(labels))
    want = (multi_group_oracle(*d, labels, reg=reg), *multi_fit(*d, reg=reg), baseline_r_squared(*d, labels, reg=reg))
    for a in (labels,) + d + want:
        a.setflags(write=False)
    return labels, d, want


# ---- 1. against the batched oracle -------------------------------------------------------------------------------------
@pytest.mark.parametrize("reg", [0.0, 0.1])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_against_the_batched_oracle(shape, reg):
    labels, d, (phi, theta, r2, base) = _case(shape, reg)
    sizes, nb, m = SHAPES[shape]
    res = ls_spa_multi(*d, reg, groups=labels)
    print(f"{shape} reg={reg}: max |phi - oracle| = {np.abs(res.attribution - phi).max():.3e}, max |sum - (r2 - base)| = "
          f"{np.abs(res.attribution.sum(axis=1) - (res.r_squared - res.baseline_r_squared)).max():.3e}")
    assert isinstance(res, MultiGroupResults)
    assert res.attribution.shape == (m, len(sizes)) and res.theta.shape == (m, len(labels))
    np.testing.assert_allclose(res.attribution, phi, **ORACLE_TOL)
    np.testing.assert_allclose(res.theta, theta, **ORACLE_TOL)
    np.testing.assert_allclose(res.r_squared, r2, **ORACLE_TOL)
    np.testing.assert_allclose(res.baseline_r_squared, base, **ORACLE_TOL)
    assert np.all(res.baseline_r_squared == 0.0) == (nb == 0)
    np.testing.assert_allclose(res.attribution.sum(axis=1), res.r_squared - res.baseline_r_squared, rtol=0, atol=1e-12)


# ---- 2. g = 20, p = 64 -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reg", [0.0, 0.1])
def test_20_mixed_groups_values_and_efficiency(engine, reg):
    """g = 20, p = 64, m = 9: the oracle of all 2^20 group subsets takes minutes, so the enumeration's own device code is
    compared on seeded masks (the empty one, the singletons, their complements and 512 random ones) with the per-column
    oracle, and phi by its sums."""
    labels = labels_of(MIXED20, 4, seed=20)
    p, ng, m = len(labels), len(MIXED20), 9
    assert p == 64
    d = problem(labels, m, seed=264)
    G, g, H, h, yy = multi_gram_problem(*d, reg)
    full = (1 << ng) - 1
    small = [0] + [1 << i for i in range(ng)]
    masks = np.array(small + [full ^ mk for mk in small] + list(np.random.default_rng(21).integers(0, 1 << ng, 512)),
                     dtype=np.uint64)
    engine.multi_load(*d, reg)
    got = engine.multi_group_values(labels, masks)
    phi, info = engine.multi_groups_shapley(labels)
    timing = engine.multi_timing()
    engine.multi_free()
    want = np.stack([group_values(G, g[r], H, h[r], yy[r], labels, masks) for r in range(m)], axis=1)
    print(f"g=20 reg={reg}: max |u - oracle| = {np.abs(got - want).max():.3e}, max |sum phi - (u(all) - u(none))| = "
          f"{np.abs(phi.sum(axis=1) - (want[len(small)] - want[0])).max():.3e}; enumeration "
          f"{timing['enumeration'] * 1e3:.1f} ms in {timing['launches']} launches, longest "
          f"{timing['max_launch'] * 1e3:.1f} ms")
    assert got.shape == (len(masks), m) and phi.shape == (m, ng) and info == 0
    np.testing.assert_allclose(got, want, **ORACLE_TOL)
    np.testing.assert_allclose(phi.sum(axis=1), want[len(small)] - want[0], rtol=0, atol=1e-12)   # u(all) - u(none)
    assert 0 < timing["max_launch"] <= 0.2


# ---- 3. rows against the one-response kernel ---------------------------------------------------------------------------
@pytest.mark.parametrize("sizes, nb", [([5] * 12, 4), ([3] * 16, 0)])
def test_rows_against_the_one_response_kernel(sizes, nb):
    labels = labels_of(sizes, nb, seed=len(sizes))
    d = problem(labels, 9, seed=700 + len(labels))
    res = ls_spa_multi(*d, groups=labels)
    for r in range(9):
        one = ls_spa(d[0], d[1], d[2][:, r], d[3][:, r], method="subsets", groups=labels)
        np.testing.assert_allclose(res.attribution[r], one.attribution, **ORACLE_TOL)
        np.testing.assert_allclose(res.theta[r], one.theta, **ORACLE_TOL)
        assert abs(res.r_squared[r] - one.r_squared) < 1e-11


# ---- 4. singletons -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [12, 24])
def test_singletons_equal_the_ungrouped_call(p):
    d = problem(np.arange(p), 9, seed=300 + p)
    grouped = ls_spa_multi(*d, groups=np.arange(p))
    plain = ls_spa_multi(*d)
    np.testing.assert_allclose(grouped.attribution, plain.attribution, **ORACLE_TOL)
    np.testing.assert_array_equal(grouped.theta, plain.theta)
    np.testing.assert_array_equal(grouped.r_squared, plain.r_squared)
    assert np.all(grouped.baseline_r_squared == 0.0)


# ---- 5. bitwise facts --------------------------------------------------------------------------------------------------
SIZES14 = [1, 2, 3, 4, 2, 3, 3, 2, 4, 3, 2, 3, 3, 2]      # 14 groups, 37 columns


@pytest.fixture(scope="module")
def wide():
    labels = labels_of(SIZES14, 3, seed=14)
    assert len(labels) == 40
    d = problem(labels, 11, seed=814)
    return labels, d, ls_spa_multi(*d, groups=labels).attribution


def test_two_calls_agree(wide):
    labels, d, phi = wide
    np.testing.assert_array_equal(ls_spa_multi(*d, groups=labels).attribution, phi)
    assert np.abs(phi).max() > 1e-3


def test_a_row_is_the_same_alone_and_with_the_columns_reversed(wide):
    labels, d, phi = wide
    alone = ls_spa_multi(d[0], d[1], d[2][:, 5:6], d[3][:, 5:6], groups=labels).attribution      # slot 0 of 1
    np.testing.assert_array_equal(alone[0], phi[5])
    rev = ls_spa_multi(d[0], d[1], d[2][:, ::-1], d[3][:, ::-1], groups=labels).attribution
    np.testing.assert_array_equal(rev, phi[::-1])


def test_identical_columns_give_identical_rows(wide):
    labels, d, phi = wide
    cols = [0, 4, 0, 1, 2, 3, 5, 6, 7, 8, 4]              # 0 and 4 twice, in other slots and another chunk
    res = ls_spa_multi(d[0], d[1], d[2][:, cols], d[3][:, cols], groups=labels).attribution
    np.testing.assert_array_equal(res[2], res[0])
    np.testing.assert_array_equal(res[10], res[1])
    np.testing.assert_array_equal(res, phi[cols])


def test_block_and_cut_do_not_change_a_bit(wide, engine):
    labels, d, phi = wide
    engine.multi_load(*d, 0.0)
    blocks = [engine.multi_groups_shapley(labels, block=b) for b in (0, RB, 2 * RB, 1)]
    head, _ = engine.multi_groups_shapley(labels, first=0, count=3)
    tail, _ = engine.multi_groups_shapley(labels, first=3, count=8)
    engine.multi_free()
    for got, info in blocks:
        assert info == 0
        np.testing.assert_array_equal(got, phi)
    np.testing.assert_array_equal(np.vstack([head, tail]), phi)


def test_a_column_scaled_by_four_gives_the_same_row(wide):
    labels, d, phi = wide
    Ya, Ye = d[2].copy(), d[3].copy()
    Ya[:, 2] *= 4.0
    Ye[:, 2] *= 4.0
    np.testing.assert_array_equal(ls_spa_multi(d[0], d[1], Ya, Ye, groups=labels).attribution, phi)


# ---- 6. relabelling ----------------------------------------------------------------------------------------------------
def test_relabelling_permutes_the_columns(wide):
    labels, d, phi = wide
    renum = np.random.default_rng(22).permutation(len(SIZES14))       # group k becomes group renum[k]
    relab = np.where(labels < 0, -1, renum[np.maximum(labels, 0)])
    got = ls_spa_multi(*d, groups=relab).attribution
    np.testing.assert_allclose(got[:, renum], phi, rtol=0, atol=1e-12)


# ---- 7. M < p ----------------------------------------------------------------------------------------------------------
def test_fewer_test_rows_than_columns():
    labels = labels_of([5] * 7, 1, seed=7)
    d = with_responses(*data(36, n=200, m=20, seed=736), 4, 736)
    res = ls_spa_multi(*d, reg=0.05, groups=labels)
    np.testing.assert_allclose(res.attribution, multi_group_oracle(*d, labels, reg=0.05), **ORACLE_TOL)
    np.testing.assert_allclose(res.attribution.sum(axis=1), res.r_squared - res.baseline_r_squared, rtol=0, atol=1e-12)


# ---- 8. the Gram form --------------------------------------------------------------------------------------------------
def test_the_gram_form(engine):
    labels = labels_of([5] * 7, 1, seed=8)
    d = with_responses(*data(36, n=400, m=300, seed=836), RB + 2, 836)
    engine.multi_load(*d, 0.01)
    from_data, info_d = engine.multi_groups_shapley(labels)
    prob = multi_gram_problem(*d, 0.01)
    engine.multi_load_reduced(*prob)
    from_gram, info_g = engine.multi_groups_shapley(labels)
    back = engine.multi_gram()
    engine.multi_free()
    assert info_d == info_g == 0
    print(f"Gram form: max |phi - phi(data form)| = {np.abs(from_gram - from_data).max():.3e}")
    np.testing.assert_allclose(from_gram, from_data, rtol=0, atol=1e-12)
    for got, want in zip(back, prob):
        np.testing.assert_array_equal(got, want)


# ---- 9. engine state ---------------------------------------------------------------------------------------------------
def test_engine_state_untouched(engine):
    glab = np.arange(14) // 2
    d1 = data(14, n=200, m=100, seed=14)
    engine.load_data(*d1, 0.0)
    engine.full_fit()
    plain, _ = engine.subsets_shapley()
    grouped, _ = engine.groups_shapley(glab)
    gram_before = engine.gram()
    timings = engine.subsets_timing(), engine.groups_timing()
    labels = labels_of([5] * 7, 1, seed=9)
    other = with_responses(*data(36, n=160, m=120, seed=936), RB + 1, 936)
    engine.multi_load(*other, 0.1)
    phi, _ = engine.multi_groups_shapley(labels)
    assert phi.shape == (RB + 1, 7)
    for a, b in zip(engine.gram(), gram_before):
        np.testing.assert_array_equal(a, b)
    assert (engine.subsets_timing(), engine.groups_timing()) == timings
    np.testing.assert_array_equal(engine.subsets_shapley()[0], plain)
    np.testing.assert_array_equal(engine.groups_shapley(glab)[0], grouped)
    engine.multi_free()
    np.testing.assert_array_equal(engine.subsets_shapley()[0], plain)
    np.testing.assert_array_equal(engine.groups_shapley(glab)[0], grouped)


# ---- 10. errors --------------------------------------------------------------------------------------------------------
def test_errors_of_the_engine(engine):
    labels = labels_of([5] * 7, 1, seed=10)
    engine.multi_free()
    with pytest.raises(Exception, match="comes first"):      # LSSPA_ERR_STATE before a load
        engine.multi_groups_shapley(labels)
    with pytest.raises(Exception, match="comes first"):
        engine.multi_group_values(labels, np.zeros(1, dtype=np.uint64))
    d = with_responses(*data(36, n=160, m=120, seed=1036), 4, 1036)
    engine.multi_load(*d, 0.0)
    try:
        for first, count in ((-1, 2), (0, 5), (3, 2), (4, 1), (0, 0)):
            with pytest.raises(ValueError, match="must lie inside"):
                engine.multi_groups_shapley(labels, first=first, count=count)
        with pytest.raises(ValueError, match="beyond g"):
            engine.multi_group_values(labels, np.array([1 << 7], dtype=np.uint64))
        with pytest.raises(ValueError, match="at most p = 32"):      # p = 36 is loaded for the grouped call alone
            engine.multi_shapley()
        with pytest.raises(ValueError, match="at most p = 32"):
            engine.multi_values(np.zeros(1, dtype=np.uint64))
        with pytest.raises(ValueError, match="no column"):
            engine.multi_groups_shapley(np.where(labels == 3, 4, labels))
        with pytest.raises(ValueError, match="at most g = 32"):
            engine.multi_groups_shapley(np.minimum(np.arange(36), 32))
        with pytest.raises(ValueError, match="length p = 36"):
            engine.multi_groups_shapley(labels[:-1])
        phi, info = engine.multi_groups_shapley(labels)              # the refusals left the responses loaded
        assert info == 0 and phi.shape == (4, 7)
    finally:
        engine.multi_free()


def test_singular_gram_warns_once():
    """Two identical columns inside a group: the verdict of ls_spa(method='subsets', groups=) for one y, once for all."""
    labels = labels_of([5] * 7, 1, seed=11)
    Xa, Xe, Ya, Ye = with_responses(*data(36, n=160, m=120, seed=1136), 3, 1136)
    a, b = np.nonzero(labels == 2)[0][:2]
    Xa[:, b], Xe[:, b] = Xa[:, a], Xe[:, a]
    with pytest.warns(RuntimeWarning, match="not numerically positive definite"):
        ls_spa(Xa, Xe, Ya[:, 0], Ye[:, 0], method="subsets", groups=labels)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        res = ls_spa_multi(Xa, Xe, Ya, Ye, groups=labels)
    assert len([w for w in seen if "not numerically positive definite" in str(w.message)]) == 1
    assert res.attribution.shape == (3, 7) and np.isfinite(res.theta).all()


def test_a_zero_test_column_is_refused_naming_it():
    labels = labels_of([5] * 7, 1, seed=12)
    Xa, Xe, Ya, Ye = with_responses(*data(36, n=160, m=120, seed=1236), 3, 1236)
    Ye[:, 1] = 0.0
    with pytest.raises(ValueError, match="column 1 of Y_test is identically zero"):
        ls_spa_multi(Xa, Xe, Ya, Ye, groups=labels)
