"""ls_spa_permutation_test on the MI355X (csrc/k_perm.hip, lsspa_perm_* of include/lsspa.h): the gathered X^T y[pi] of
every replicate against a long-double truth at every slice, block and column-block edge (tests/perm_ref.py has the
cases, tests/test_permutation_host.py proves which edges they reach), the null rows against the explicit construction
through ls_spa_multi, and -- bitwise -- that a replicate does not depend on how a run is cut."""
import functools
import warnings

import numpy as np
import pytest
import torch

import perm_ref
from ls_spa import ls_spa, ls_spa_multi, ls_spa_permutation_test
from test_subsets_host import data

pytestmark = pytest.mark.gpu

ORACLE_TOL = dict(rtol=0, atol=1e-11)      # that of tests/test_gpu_multi.py, for the same enumeration kernels
U = 2.0 ** -53                             # tests/test_gpu_gram_exact.py
SEED = 20240607
LD = np.longdouble


def _truth(X, y, seed, first, R, side):
    """(sums [R][p] in long double, magnitudes [R][p]): X^T y[pi_r] and sum_i |x_ij| |y[pi_r(i)]|."""
    Xl, yl = X.astype(LD), y.astype(LD)
    idx = [perm_ref.indices(seed, r, side, len(y)) for r in range(first, first + R)]
    return (np.stack([Xl.T @ yl[a] for a in idx]), np.stack([np.abs(Xl).T @ np.abs(yl[a]) for a in idx]))


@functools.lru_cache(maxsize=None)
def _case_data(N, M, p, integer):
    rng = np.random.default_rng([N, M, p, int(integer)])
    if integer:
        return tuple(rng.integers(-8, 9, size=s).astype(np.float64) for s in ((N, p), (M, p), (N,), (M,)))
    scale = 1.7 * 2.0 ** rng.integers(-6, 7, size=p)
    Xa, Xe = (1.0 + rng.standard_normal((N, p))) * scale, (1.0 + rng.standard_normal((M, p))) * scale
    return Xa, Xe, 3.0 + rng.standard_normal(N), 3.0 + rng.standard_normal(M)


@pytest.mark.parametrize("integer", [False, True], ids=["real", "integer"])
@pytest.mark.parametrize("case", perm_ref.XTY_CASES, ids=["N%d_M%d_p%d_g%d_R%d_b%d" % c for c in perm_ref.XTY_CASES])
def test_xty_of_every_replicate_against_the_truth(engine, case, integer):
    """|C - truth| <= gamma_n sum_i |x_ij| |y_pi(i)|, gamma_n = n u / (1 - n u): the bound of a sum of n products in any
    order (tests/test_gpu_gram_exact.py), so it covers slices and the matrix instruction's own order.  The training side
    is then multiplied by a rounded 1 / N: two more roundings relative to the value.  On small integers every sum is
    exact, and so is the comparison."""
    N, M, p, g, R, block = case
    Xa, Xe, ya, ye = _case_data(N, M, p, integer)
    labels = perm_ref.case_labels(p, g)
    ye = ye if np.any(ye) else ye + 1.0
    try:
        engine.perm_load(Xa, Xe, ya, ye, 1.0)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            phi, gp, hp, info = engine.perm_run(R, SEED, labels, block=block)
    finally:
        engine.perm_free()
    assert gp.shape == hp.shape == (R, p) and np.isfinite(phi).all()
    for got, X, y, side, rows in ((gp, Xa, ya, 0, N), (hp, Xe, ye, 1, M)):
        want, mag = _truth(X, y, SEED, 0, R, side)
        if integer:
            want = want.astype(np.float64) * (1.0 / N) if side == 0 else want.astype(np.float64)
            np.testing.assert_array_equal(got, want)
            continue
        gamma = LD(rows * U) / (1 - LD(rows * U))
        bound = gamma * mag
        if side == 0:
            want, bound = want / N, (bound + 2 * U * np.abs(want)) / N
        ratio = np.abs(got.astype(LD) - want) / np.maximum(bound, LD(1e-300))
        print(f"PERMACC {case} side {side}: worst err/bound {float(ratio.max()):.4f}")
        assert float(ratio.max()) <= 1.0


# ---- null rows against the explicit construction --------------------------------------------------------------------
LABELS = np.array([0, 1, -1, 1, 2, 0, 2, 1, -1])


@pytest.mark.parametrize("groups", [None, LABELS], ids=["features", "groups"])
@pytest.mark.parametrize("permute", [("train", "test"), "train", "test"])
def test_null_rows_equal_ls_spa_multi_on_the_permuted_responses(groups, permute):
    R, p = 19, 9
    Xa, Xe, ya, ye = data(p, n=90, m=50, seed=31)
    res = ls_spa_permutation_test(Xa, Xe, ya, ye, 0.05, n_perm=R, seed=SEED, groups=groups, permute=permute)
    Ya = perm_ref.permuted_responses(ya, SEED, range(R), 0) if "train" in permute else np.repeat(ya[:, None], R, axis=1)
    Ye = perm_ref.permuted_responses(ye, SEED, range(R), 1) if "test" in permute else np.repeat(ye[:, None], R, axis=1)
    want = ls_spa_multi(Xa, Xe, Ya, Ye, 0.05, groups=groups)
    one = ls_spa(Xa, Xe, ya, ye, 0.05, method="subsets", groups=groups)
    print(f"max |null - multi| = {np.abs(res.null_attribution - want.attribution).max():.3e}, "
          f"max |observed - ls_spa| = {np.abs(res.attribution - one.attribution).max():.3e}")
    np.testing.assert_allclose(res.null_attribution, want.attribution, **ORACLE_TOL)
    np.testing.assert_allclose(res.null_r_squared, want.r_squared, **ORACLE_TOL)
    np.testing.assert_allclose(res.attribution, one.attribution, **ORACLE_TOL)
    np.testing.assert_allclose(res.theta, one.theta, **ORACLE_TOL)
    assert abs(res.r_squared - one.r_squared) < 1e-11
    if groups is not None:
        np.testing.assert_allclose(res.null_baseline_r_squared, want.baseline_r_squared, **ORACLE_TOL)
        np.testing.assert_allclose(res.null_attribution.sum(axis=1), res.null_r_squared - res.null_baseline_r_squared,
                                   rtol=0, atol=1e-9)
    else:
        np.testing.assert_allclose(res.null_attribution.sum(axis=1), res.null_r_squared, rtol=0, atol=1e-9)
    assert res.n_failed == 0 and res.n_perm == R


def test_m_smaller_than_p():
    Xa, Xe, ya, ye = data(8, n=60, m=5, seed=32)
    res = ls_spa_permutation_test(Xa, Xe, ya, ye, n_perm=9, seed=SEED)
    one = ls_spa(Xa, Xe, ya, ye, method="subsets")
    np.testing.assert_allclose(res.attribution, one.attribution, **ORACLE_TOL)
    Ya, Ye = perm_ref.permuted_responses(ya, SEED, range(9), 0), perm_ref.permuted_responses(ye, SEED, range(9), 1)
    np.testing.assert_allclose(res.null_attribution, ls_spa_multi(Xa, Xe, Ya, Ye).attribution, **ORACLE_TOL)


# ---- bitwise independence -------------------------------------------------------------------------------------------
IND = dict(p=9, n=300, m=70, seed=33)


def test_a_replicate_does_not_depend_on_n_perm_and_two_calls_agree():
    d = data(**IND)
    a = ls_spa_permutation_test(*d, n_perm=37, seed=SEED)
    b = ls_spa_permutation_test(*d, n_perm=5, seed=SEED)
    c = ls_spa_permutation_test(*d, n_perm=37, seed=SEED)
    np.testing.assert_array_equal(a.null_attribution[:5], b.null_attribution)
    np.testing.assert_array_equal(a.null_r_squared[:5], b.null_r_squared)
    for f in ("attribution", "null_attribution", "null_r_squared", "p_values", "p_values_adjusted"):
        np.testing.assert_array_equal(getattr(a, f), getattr(c, f))
    assert a.r_squared_p_value == c.r_squared_p_value
    assert not np.array_equal(a.null_attribution, ls_spa_permutation_test(*d, n_perm=37, seed=SEED + 1).null_attribution)


def test_a_replicate_does_not_depend_on_block_first_or_groups(engine):
    d = data(**IND)
    labels = (np.arange(IND["p"]) % 4).astype(np.int32)
    try:
        engine.perm_load(*d, 0.0)
        whole = engine.perm_run(37, SEED)
        for block in (8, 16):
            cut = engine.perm_run(37, SEED, block=block)
            for x, y in zip(whole[:3], cut[:3]):
                np.testing.assert_array_equal(x, y)
        lo, hi = engine.perm_run(20, SEED, first=0), engine.perm_run(17, SEED, first=20, block=8)
        for k in range(3):
            np.testing.assert_array_equal(whole[k], np.concatenate([lo[k], hi[k]]))
        grouped = engine.perm_run(37, SEED, labels)
        np.testing.assert_array_equal(grouped[1], whole[1])
        np.testing.assert_array_equal(grouped[2], whole[2])
        assert grouped[0].shape == (37, 4)
        train_only = engine.perm_run(5, SEED, sides=1)
        _, g, _, h, _ = engine.perm_gram()
        np.testing.assert_array_equal(train_only[1], whole[1][:5])
        np.testing.assert_array_equal(train_only[2], np.repeat(h[None], 5, axis=0))
        t = engine.perm_timing()
        assert set(t) == {"draw", "upload", "xty", "enumeration"} and all(v >= 0 for v in t.values())
    finally:
        engine.perm_free()


# ---- isolation --------------------------------------------------------------------------------------------------------
def test_other_states_keep_their_bits_and_the_memory_comes_back(engine):
    Xa, Xe, ya, ye = data(7, n=80, m=40, seed=34)
    Ya, Ye = np.stack([ya, ya ** 2], axis=1), np.stack([ye, ye ** 2], axis=1)

    def others():
        return (engine.subsets_shapley()[0], engine.boot_run(4, 5)[0], engine.multi_shapley()[0])

    try:
        engine.load_data(Xa, Xe, ya, ye, 0.0)
        engine.boot_load(Xa, Xe, ya, ye, 0.0)
        engine.multi_load(Xa, Xe, Ya, Ye, 0.0)
        before = others()
        first = ls_spa_permutation_test(Xa, Xe, ya, ye, n_perm=20, seed=SEED, _engine=engine)
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        again = ls_spa_permutation_test(Xa, Xe, ya, ye, n_perm=20, seed=SEED, _engine=engine)
        torch.cuda.synchronize()
        free1 = torch.cuda.mem_get_info()[0]
        after = others()
    finally:
        engine.boot_free()
        engine.multi_free()
    for x, y in zip(before, after):
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(first.null_attribution, again.null_attribution)
    assert free1 == free0, (free0, free1)
    assert getattr(engine, "_perm_dims", None) is None


# ---- not positive definite -----------------------------------------------------------------------------------------------
def test_a_duplicated_column_warns_and_does_not_raise():
    Xa, Xe, ya, ye = data(5, n=60, m=40, seed=35)
    Xa[:, 4], Xe[:, 4] = Xa[:, 3], Xe[:, 3]
    with pytest.warns(RuntimeWarning, match="not numerically positive definite"):
        res = ls_spa_permutation_test(Xa, Xe, ya, ye, n_perm=9, seed=SEED)
    assert res.n_failed in (0, 9) and res.null_attribution.shape == (9, 5)
