"""ls_spa_best_subsets(groups=) on the MI355X: the best set of groups of every size over all 2^g group subsets
(csrc/k_groups.hip, groups_best_kernel) against the brute-force truth of tests/group_best_ref.py, against the device's
own values, on exact ties under two numberings, against a planted additive truth where brute force cannot go (g = 20
over several launches; g = 28, per = 512), against the column call on singletons, its determinism and isolation, a Gram
matrix that is not positive definite, and the public call."""
import warnings

import numpy as np
import pytest

import best_ref as B
import group_best_ref as R
from ls_spa import BestGroupSubsetsResults, ls_spa, ls_spa_best_subsets
from ls_spa._engine import debug_groups_best_plan
from test_subsets_host import data, gram_problem

pytestmark = pytest.mark.gpu

ORACLE_TOL = dict(rtol=0, atol=1e-11)      # the project's bound for these enumerations (tests/test_gpu_groups.py)
NAMES = [n for n in R.CASES if n not in R.RECT]


def popcount(masks):
    return np.array([bin(int(m)).count("1") for m in masks])


def check_against_truth(got, u_all, g):
    u, masks, found, info = got
    best, want_masks, want_found, _ = B.best_truth(u_all, g)
    print("max |u - truth|", np.nanmax(np.abs(u - best)), "masks", [hex(int(m)) for m in masks])
    assert info == 0 and u.shape == (g + 1,) and masks.dtype == np.uint32
    np.testing.assert_array_equal(found, want_found)
    np.testing.assert_array_equal(masks, want_masks)
    np.testing.assert_allclose(u, best, **ORACLE_TOL)
    assert abs(u[0] - u_all[0]) <= 1e-11 and masks[0] == 0 and masks[g] == (1 << g) - 1


# ---- 1. brute force ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reg", R.REGS)
@pytest.mark.parametrize("name", NAMES)
def test_against_brute_force(engine, name, reg):
    d, labels, u_all = R.brute_case(name, reg)
    engine.load_data(*d, reg)
    assert engine.tri
    got = engine.groups_best(labels)
    check_against_truth(got, u_all, int(labels.max()) + 1)
    if not (labels < 0).any():
        assert got[0][0] == 0.0


def test_against_brute_force_in_rect_mode(engine):
    d, labels, u_all = R.brute_case(R.RECT[0], 0.0)
    engine.load_data(*d, 0.0)
    assert not engine.tri
    check_against_truth(engine.groups_best(labels), u_all, int(labels.max()) + 1)


# ---- 2. the device's own values ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["g12p64", "gl0"])
def test_winners_carry_the_devices_own_values(engine, name):
    d, labels, _ = R.brute_case(name, 0.0)
    engine.load_data(*d, 0.0)
    u, masks, found, info = engine.groups_best(labels)
    assert info == 0 and found.all()
    np.testing.assert_array_equal(u, engine.debug_group_values(labels, masks.astype(np.uint64)))


@pytest.mark.parametrize("name", list(R.CASES))
def test_winners_are_the_best_of_the_devices_own_table(engine, name):
    d, labels, _ = R.brute_case(name, 0.0)
    g = int(labels.max()) + 1
    engine.load_data(*d, 0.0)
    u, masks, found, info = engine.groups_best(labels)
    table = engine.debug_group_values(labels, np.arange(1 << g, dtype=np.uint64))
    best, want_masks, want_found, _ = B.best_truth(table, g)
    assert info == 0
    np.testing.assert_array_equal(found, want_found)
    np.testing.assert_array_equal(masks, want_masks)
    np.testing.assert_array_equal(u, best)


# ---- 3. ties -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("run", list(R.TIE_RUNS))
def test_exact_ties_go_to_the_smallest_caller_mask(engine, run):
    d, labels, u_all = R.tie_case(run)
    engine.load_data(*d, 0.0)
    u, masks, found, info = engine.groups_best(labels)
    print(run, "masks", list(masks), "u", list(u))
    assert info == 0 and found.all()
    assert list(masks[1:4]) == R.tie_winners(run) and (u[:4] == 0.0).all()
    np.testing.assert_array_equal(masks, B.best_truth(u_all, 5)[1])
    np.testing.assert_allclose(u, B.best_truth(u_all, 5)[0], **ORACLE_TOL)


# ---- 4. planted truth --------------------------------------------------------------------------------------------------
def planted(labels, seed):
    """Orthonormal columns on both sides (planted() of tests/test_gpu_best_subsets.py): G = I / N and H = I to
    rounding, so v(K) = sum_{j in K} d_j with d_j = (2 a_j b_j - a_j^2) / ||y_test||^2, a = X_train^T y_train,
    b = X_test^T y_test -- additive over the columns, hence u over the groups, with d_k = the sum over group k's
    columns.  With a_j = 1 and b_j = (1 + t_j) / 2, d_j = t_j / ||y_test||^2: every column of group k gets the same
    t_k, g values from -1 to 1.5 in a shuffled order, so the d_k are of both signs and far more than 1e-6 apart."""
    rng = np.random.default_rng(seed)
    p, g = len(labels), int(labels.max()) + 1
    n = 2 * p + 8
    Qa = np.linalg.qr(rng.standard_normal((n, p)))[0]
    Qe = np.linalg.qr(rng.standard_normal((n, p)))[0]
    t = np.linspace(-1.0, 1.5, g)[rng.permutation(g)][labels]
    noise = rng.standard_normal(n)
    noise -= Qe @ (Qe.T @ noise)
    ya, ye = Qa @ np.ones(p), Qe @ ((1.0 + t) / 2.0) + noise
    a, b, yy = Qa.T @ ya, Qe.T @ ye, float(ye @ ye)
    dj = (2.0 * a * b - a * a) / yy
    dk = np.array([dj[labels == k].sum() for k in range(g)])
    assert np.diff(np.sort(dk)).min() > 1e-6 and (dk > 0).any() and (dk < 0).any()
    return (Qa, Qe, ya, ye), dk


def check_planted(engine, labels, seed):
    """The winner of size s is the s best groups, its value their sum."""
    d, dk = planted(labels, seed)
    engine.load_data(*d, 0.0)
    u, masks, found, info = engine.groups_best(labels)
    order = np.argsort(-dk)
    want_u = np.concatenate([[0.0], np.cumsum(dk[order])])
    want_masks = np.concatenate([np.zeros(1, dtype=np.uint64),
                                 np.cumsum(np.uint64(1) << order.astype(np.uint64))]).astype(np.uint32)
    print("max |u - planted|", np.abs(u - want_u).max(), "winners", [hex(int(m)) for m in masks])
    assert info == 0 and found.all()
    np.testing.assert_array_equal(masks, want_masks)
    np.testing.assert_allclose(u, want_u, **ORACLE_TOL)        # additivity holds to a few p eps: G, H diagonal to rounding
    assert int(np.argmax(u)) == int((dk > 0).sum())
    return masks


@pytest.mark.parametrize("name, seed", [("g20x3", 6000), ("g28", 2800)])
def test_planted_truth_over_several_launches(engine, name, seed):
    labels, plan = R.PLANTED[name]
    masks = check_planted(engine, labels, seed)
    assert engine.groups_timing()[2] == plan["launches"] > 1
    # equal sizes: the low groups are labels 0 .. gl-1, the high ones follow in order, so hi = mask >> gl; a unit's
    # steps are the low bits of hi: early and late launches both win, and many units
    per_bits = plan["per"].bit_length() - 1
    hi = masks.astype(np.int64) >> plan["gl"]
    step, units = hi & (plan["per"] - 1), hi >> per_bits
    assert len(np.unique(units)) > 8 and step.min() < plan["per"] // 4 and step.max() >= 3 * plan["per"] // 4
    assert len(np.unique(popcount(step))) >= per_bits          # the size classes of a unit, up to the deepest


# ---- 5. all singletons --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [9, 12])
def test_singletons_select_what_the_column_call_selects(engine, p):
    d, _ = B.brute_case(p, 0.0)
    engine.load_data(*d, 0.0)
    v, cmasks, cfound, _ = engine.subsets_best()
    u, masks, found, info = engine.groups_best(np.arange(p))
    assert info == 0 and found.all() and cfound.all()
    np.testing.assert_array_equal(masks, cmasks)
    np.testing.assert_allclose(u, v, **ORACLE_TOL)             # (another arithmetic: not bitwise)
    res = ls_spa_best_subsets(*d, groups=np.arange(p))
    ref = ls_spa_best_subsets(*d)
    np.testing.assert_array_equal(res.group_subsets, ref.subsets)
    np.testing.assert_array_equal(res.subsets, ref.subsets)
    np.testing.assert_allclose(res.r_squared, ref.r_squared, **ORACLE_TOL)


# ---- 6. determinism and isolation -----------------------------------------------------------------------------------------
def test_two_calls_agree_and_the_attributions_are_untouched(engine):
    d, labels, _ = R.brute_case("g12p64", 0.0)
    d32 = data(16, n=200, m=120, seed=716)
    engine.load_data(*d, 0.0)
    phi0, _ = engine.groups_shapley(labels)
    first = engine.groups_best(labels)
    timing = engine.groups_timing()
    assert timing[2] >= 1 and timing[0] > 0
    again = engine.groups_best(labels)
    phi1, _ = engine.groups_shapley(labels)
    for a, b in zip(first, again):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(phi0, phi1)
    engine.load_data(*d32, 0.0)
    sub0, _ = engine.subsets_shapley()
    engine.groups_best(np.arange(16) // 2)
    np.testing.assert_array_equal(engine.subsets_shapley()[0], sub0)


def test_kept_engine_sampling_unchanged_by_a_grouped_best_subsets_call():
    d = data(12, n=200, m=100, seed=12)
    kw = dict(method="argsort", seed=7, max_samples=512, batch_size=128, tolerance=0.0)
    before = ls_spa(*d, **kw)
    ls_spa_best_subsets(*d, groups=np.arange(12) // 3)
    after = ls_spa(*d, **kw)
    np.testing.assert_array_equal(before.attribution, after.attribution)
    np.testing.assert_array_equal(before.error_history, after.error_history)
    np.testing.assert_array_equal(before.attribution_errors, after.attribution_errors)


# ---- 7. not positive definite ---------------------------------------------------------------------------------------------
# sizes 1, 2, 2 are low (5 columns), 4 and 4 high; the copy of a column of group a replaces a column of group b
@pytest.mark.parametrize("a, b", [(0, 1), (3, 4), (2, 3)])       # both low, both high (the workgroup's pivot), one of each
def test_duplicate_column(engine, a, b):
    labels = np.repeat(np.arange(5), [1, 2, 2, 4, 4])
    g, p = 5, 13
    plan = debug_groups_best_plan(labels)
    assert plan["gl"] == 3 and plan["gh"] == 2
    Xa, Xe, ya, ye = data(p, seed=81)
    ja, jb = np.nonzero(labels == a)[0][0], np.nonzero(labels == b)[0][-1]
    Xa[:, jb], Xe[:, jb] = Xa[:, ja], Xe[:, ja]
    engine.load_data(Xa, Xe, ya, ye, 0.0)
    u, masks, found, info = engine.groups_best(labels)
    both = (1 << a) | (1 << b)
    assert info & 1
    assert found[:g].all() and not found[g] and np.isnan(u[g]) and masks[g] == 0
    assert ((masks[:g] & both) != both).all()
    np.testing.assert_array_equal(popcount(masks[:g]), np.arange(g))
    with pytest.warns(RuntimeWarning, match="not numerically positive definite"):
        res = ls_spa_best_subsets(Xa, Xe, ya, ye, groups=labels)
    assert np.isnan(res.r_squared[g]) and np.isnan(res.theta[g]).all() and 0 <= res.best_size < g
    assert np.isfinite(res.theta[:g]).all()


# ---- 8. the public call ---------------------------------------------------------------------------------------------------
def test_public_call():
    reg = 0.1
    d, labels, u_all = R.brute_case("nine", reg)
    g, p = int(labels.max()) + 1, len(labels)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        res = ls_spa_best_subsets(*d, reg=reg, groups=labels)
        full = ls_spa(*d, reg=reg, method="subsets", groups=labels)
    assert isinstance(res, BestGroupSubsetsResults)
    best, masks, found, _ = B.best_truth(u_all, g)
    assert res.sizes.tolist() == list(range(g + 1))
    assert res.group_subsets.shape == (g + 1, g) and res.subsets.shape == (g + 1, p) and res.theta.shape == (g + 1, p)
    np.testing.assert_allclose(res.r_squared, best, **ORACLE_TOL)
    G, gv, H, h, yy = gram_problem(*d, reg=reg)
    for k in range(g + 1):
        assert B.mask_of(np.nonzero(res.group_subsets[k])[0]) == masks[k]
        np.testing.assert_array_equal(res.subsets[k], R.columns_of(labels, masks[k]))
        cols = np.nonzero(res.subsets[k])[0]
        assert res.n_columns[k] == len(cols) and (res.theta[k, ~res.subsets[k]] == 0.0).all()
        np.testing.assert_allclose(res.theta[k, cols], np.linalg.solve(G[np.ix_(cols, cols)], gv[cols]), rtol=1e-9,
                                   atol=1e-12)
    assert res.best_size == int(np.argmax(best))
    np.testing.assert_array_equal(res.best_group_subset, res.group_subsets[res.best_size])
    np.testing.assert_array_equal(res.best_subset, res.subsets[res.best_size])
    assert res.baseline_r_squared == res.r_squared[0] and abs(res.baseline_r_squared - u_all[0]) <= 1e-11
    assert res.full_r_squared == full.r_squared
    assert abs(res.r_squared[-1] - full.r_squared) < 1e-11
    np.testing.assert_allclose(res.theta[-1], full.theta, rtol=1e-9, atol=1e-12)


def test_refused_by_the_library(engine):
    engine.load_data(*data(9, seed=1), 0.0)
    with pytest.raises(ValueError, match="no column"):
        engine.groups_best([0, 0, 0, 2, 2, 2, 3, 3, 3])
    with pytest.raises(ValueError, match="outside -1 .. g-1"):
        engine.groups_best([0, 0, 0, 1, 1, 1, -2, 2, 2])
    with pytest.raises(ValueError, match="length p = 9"):
        engine.groups_best([0, 1])
