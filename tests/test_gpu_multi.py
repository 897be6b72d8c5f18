"""ls_spa_multi on the MI355X (csrc/k_multi.hip, lsspa_multi_* of include/lsspa.h): the attribution of many responses
against the CPU oracle of tests/test_multi_host.py at every chunk edge, per column against the one-response kernel, the
value hook over all subsets, and -- bitwise -- that a response's row does not depend on its place, on the other
responses or on how a run is cut."""
import functools

import numpy as np
import pytest

from ls_spa import ls_spa, ls_spa_multi
from ls_spa._engine import HipEngine
from test_multi_host import (multi_data, multi_fit, multi_gram_problem, multi_oracle_batched, multi_subset_values)
from test_subsets_host import exact_shapley

pytestmark = pytest.mark.gpu

ORACLE_TOL = dict(rtol=0, atol=1e-11)      # that of tests/test_gpu_subsets.py
RB = HipEngine.MULTI_RB
M_MAX = 2 * RB + 3


@functools.lru_cache(maxsize=None)
def _case(p, reg):
    """The data with M_MAX responses and their oracle, computed once; fewer responses are its first columns."""
    d = multi_data(p, M_MAX, n=max(60, 3 * p), rows=max(40, 2 * p), seed=100 + p)
    want = multi_oracle_batched(*d, reg=reg), *multi_fit(*d, reg=reg)
    for a in d + want:
        a.setflags(write=False)
    return d, want


def _first(d, m):
    return d[0], d[1], d[2][:, :m], d[3][:, :m]


@pytest.mark.parametrize("reg", [0.0, 0.1])
@pytest.mark.parametrize("m", [1, RB - 1, RB, RB + 1, M_MAX])
@pytest.mark.parametrize("p", [1, 2, 5, 6, 7, 12, 16])
def test_against_the_cpu_oracle(p, m, reg):
    d, (phi, theta, r2) = _case(p, reg)
    res = ls_spa_multi(*_first(d, m), reg)
    print(f"p={p} m={m} reg={reg}: max |phi - oracle| = {np.abs(res.attribution - phi[:m]).max():.3e}, "
          f"max |sum - r2| = {np.abs(res.attribution.sum(axis=1) - res.r_squared).max():.3e}")
    np.testing.assert_allclose(res.attribution, phi[:m], **ORACLE_TOL)
    np.testing.assert_allclose(res.r_squared, r2[:m], **ORACLE_TOL)
    np.testing.assert_allclose(res.theta, theta[:m], **ORACLE_TOL)
    np.testing.assert_allclose(res.attribution.sum(axis=1), res.r_squared, rtol=0, atol=1e-12)


def test_p20_every_phi_against_the_cpu_oracle():
    """Several high subsets per unit: every phi of every response, not only the sums."""
    d = multi_data(20, RB + 1, n=300, rows=150, seed=120)
    res = ls_spa_multi(*d, 0.05)
    want = multi_oracle_batched(*d, reg=0.05)
    print(f"p=20: max |phi - oracle| = {np.abs(res.attribution - want).max():.3e}")
    np.testing.assert_allclose(res.attribution, want, **ORACLE_TOL)


def test_p27_several_launches_and_column_permutation(engine):
    """Several launches into the unit table: permuting the features permutes every row; rows sum to the oracle's R^2."""
    p, m = 27, 3
    Xa, Xe, Ya, Ye = multi_data(p, m, n=400, rows=200, seed=270)
    perm = np.random.default_rng(27).permutation(p)
    engine.multi_load(Xa, Xe, Ya, Ye, 0.0)
    phi, info = engine.multi_shapley()
    assert engine.multi_timing()["launches"] > 1
    engine.multi_load(Xa[:, perm], Xe[:, perm], Ya, Ye, 0.0)
    phi_p, info_p = engine.multi_shapley()
    engine.multi_free()
    assert info == info_p == 0
    print(f"p=27: max |phi_perm - phi[perm]| = {np.abs(phi_p - phi[:, perm]).max():.3e}")
    np.testing.assert_allclose(phi_p, phi[:, perm], rtol=0, atol=1e-12)
    np.testing.assert_allclose(phi.sum(axis=1), multi_fit(Xa, Xe, Ya, Ye)[1], **ORACLE_TOL)
    assert np.abs(phi).max() > 1e-3


def test_rows_against_the_one_response_kernel():
    p, m = 12, 5
    d = multi_data(p, m, seed=112)
    res = ls_spa_multi(*d, 0.0)
    for r in range(m):
        one = ls_spa(d[0], d[1], d[2][:, r], d[3][:, r], method="subsets")
        np.testing.assert_allclose(res.attribution[r], one.attribution, **ORACLE_TOL)
        np.testing.assert_allclose(res.theta[r], one.theta, **ORACLE_TOL)
        assert abs(res.r_squared[r] - one.r_squared) < 1e-11


def test_values_of_all_subsets(engine):
    p, m = 9, RB + 1
    d = multi_data(p, m, seed=109)
    engine.multi_load(*d, 0.0)
    masks = np.arange(1 << p, dtype=np.uint64)
    got = engine.multi_values(masks)
    engine.multi_free()
    want = multi_subset_values(*multi_gram_problem(*d), masks)
    assert got.shape == (1 << p, m)
    np.testing.assert_allclose(got, want, **ORACLE_TOL)
    assert np.all(got[0] == 0.0)


# ---- independence and determinism, bitwise ---------------------------------------------------------------------------
P_IND = 13


@pytest.fixture(scope="module")
def wide():
    d = multi_data(P_IND, M_MAX, n=90, rows=50, seed=213)
    return d, ls_spa_multi(*d).attribution


def test_two_calls_agree(wide):
    d, phi = wide
    np.testing.assert_array_equal(ls_spa_multi(*d).attribution, phi)


def test_a_row_does_not_depend_on_the_columns_behind_it(wide):
    d, phi = wide
    np.testing.assert_array_equal(ls_spa_multi(*_first(d, 3)).attribution, phi[:3])


def test_reversed_columns_reverse_the_rows(wide):
    d, phi = wide
    rev = ls_spa_multi(d[0], d[1], d[2][:, ::-1], d[3][:, ::-1]).attribution
    np.testing.assert_array_equal(rev, phi[::-1])


def test_identical_columns_give_identical_rows(wide):
    d, phi = wide
    cols = [0, 4, 0, 1, 2, 3, 5, 6, 7, 8, 4]              # 0 and 4 twice, in other slots and another chunk
    res = ls_spa_multi(d[0], d[1], d[2][:, cols], d[3][:, cols]).attribution
    np.testing.assert_array_equal(res[2], res[0])
    np.testing.assert_array_equal(res[10], res[1])
    np.testing.assert_array_equal(res, phi[cols])


def test_block_and_cut_do_not_change_a_bit(wide, engine):
    d, phi = wide
    engine.multi_load(*d, 0.0)
    whole, info = engine.multi_shapley(block=0)
    one_by_one, _ = engine.multi_shapley(block=1)
    chunked, _ = engine.multi_shapley(block=RB)
    head, _ = engine.multi_shapley(first=0, count=5)
    tail, _ = engine.multi_shapley(first=5)
    engine.multi_free()
    assert info == 0
    np.testing.assert_array_equal(whole, phi)
    np.testing.assert_array_equal(one_by_one, phi)
    np.testing.assert_array_equal(chunked, phi)
    np.testing.assert_array_equal(np.vstack([head, tail]), phi)


def test_a_column_scaled_by_four_gives_the_same_row(wide):
    d, phi = wide
    Ya, Ye = d[2].copy(), d[3].copy()
    Ya[:, 2] *= 4.0
    Ye[:, 2] *= 4.0
    np.testing.assert_array_equal(ls_spa_multi(d[0], d[1], Ya, Ye).attribution, phi)


# ---- other checks ------------------------------------------------------------------------------------------------------
def test_fewer_test_rows_than_features():
    d = multi_data(8, 4, n=60, rows=5, seed=85)
    res = ls_spa_multi(*d)
    np.testing.assert_allclose(res.attribution, multi_oracle_batched(*d), **ORACLE_TOL)
    np.testing.assert_allclose(res.attribution.sum(axis=1), res.r_squared, rtol=0, atol=1e-12)


def test_the_gram_form(engine):
    rng = np.random.default_rng(41)
    p, m = 10, RB + 2
    A, B = rng.standard_normal((200, p)), rng.standard_normal((150, p))
    G, H = A.T @ A / 200 + 0.01 * np.eye(p), B.T @ B
    g, yt = rng.standard_normal((m, 200)) @ A / 200, rng.standard_normal((m, 150))
    h, yy = yt @ B, np.einsum("ri,ri->r", yt, yt)
    engine.multi_load_reduced(G, g, H, h, yy)
    phi, info = engine.multi_shapley()
    back = engine.multi_gram()
    engine.multi_free()
    assert info == 0
    for r in range(m):
        np.testing.assert_allclose(phi[r], exact_shapley(G, g[r], H, h[r], yy[r]), **ORACLE_TOL)
    for got, want in zip(back, (G, g, H, h, yy)):
        np.testing.assert_array_equal(got, want)


def test_the_loaded_problem_is_left_alone(engine):
    p = 11
    d = multi_data(p, 5, seed=111)
    engine.load_data(d[0], d[1], d[2][:, 0], d[3][:, 0], 0.0)
    before, _ = engine.subsets_shapley()
    gram_before = engine.gram()
    other = multi_data(7, RB + 1, seed=77)                # another p, other rows
    engine.multi_load(*other, 0.1)
    phi, _ = engine.multi_shapley()
    assert phi.shape == (RB + 1, 7)
    for a, b in zip(engine.gram(), gram_before):
        np.testing.assert_array_equal(a, b)
    after, _ = engine.subsets_shapley()
    engine.multi_free()
    again, _ = engine.subsets_shapley()
    np.testing.assert_array_equal(after, before)
    np.testing.assert_array_equal(again, before)


def test_errors_of_the_engine(engine):
    with pytest.raises(Exception, match="comes first"):      # LSSPA_ERR_STATE before a load
        engine.multi_shapley()
    d = multi_data(6, 4, seed=66)
    engine.multi_load(*d, 0.0)
    for first, count in ((-1, 2), (0, 5), (3, 2), (4, 1), (0, 0)):
        with pytest.raises(ValueError, match="must lie inside"):
            engine.multi_shapley(first=first, count=count)
    with pytest.raises(ValueError, match="beyond p"):
        engine.multi_values(np.array([1 << 6], dtype=np.uint64))
    engine.multi_free()


def test_singular_gram_warns_for_all_responses():
    """The verdict of ls_spa(method='subsets') for one y: a RuntimeWarning, theta of minimal norm."""
    Xa, Xe, Ya, Ye = multi_data(8, 3, seed=88)
    Xa[:, 7], Xe[:, 7] = Xa[:, 1], Xe[:, 1]
    with pytest.warns(RuntimeWarning, match="not numerically positive definite"):
        ls_spa(Xa, Xe, Ya[:, 0], Ye[:, 0], method="subsets")
    with pytest.warns(RuntimeWarning, match="not numerically positive definite"):
        res = ls_spa_multi(Xa, Xe, Ya, Ye)
    assert res.attribution.shape == (3, 8) and np.isfinite(res.theta).all()
    np.testing.assert_allclose(res.theta[:, 7], res.theta[:, 1], rtol=0, atol=1e-9)


def test_a_zero_test_column_is_refused_like_a_zero_y():
    Xa, Xe, Ya, Ye = multi_data(5, 3, seed=55)
    Ye[:, 1] = 0.0
    with pytest.raises(ValueError, match="identically zero"):
        ls_spa(Xa, Xe, Ya[:, 1], Ye[:, 1], method="subsets")
    with pytest.raises(ValueError, match="column 1 of Y_test is identically zero"):
        ls_spa_multi(Xa, Xe, Ya, Ye)
