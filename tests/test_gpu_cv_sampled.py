"""ls_spa_cv_sampled on the MI355X (the fold launch of csrc/k_small.hip, cv_lift_fold_kernel of csrc/k_cv.hip,
lsspa_cv_lift_* of include/lsspa.h): the folds' lift vectors and their sum against the long-double truth of
tests/cv_sampled_ref.py at every edge of the kernels' layout, the fold problems against long-double Grams and the exact
CV load, fold f against the one-response kernels, the bitwise contracts of the header, groups, the running statistics,
the public call against ls_spa_cv, flags, isolation, errors and memory.

Tolerance: the project's rule, tol = max(1e-10, 8 e_plain) with e_plain the error of NumPy / LAPACK on the same case
(tests/test_gpu_multi_sampled.py).  No case here may be flagged NOT_PD: for exactly these data (seed 7000 + p) the
smallest relative pivot of any fold's G_f or H_f over the three orderings is at least 1e6 x the threshold 16 p eps."""
import functools

import numpy as np
import pytest

import cv_sampled_ref as ref
import hp_ref
from ls_spa import ls_spa_cv, ls_spa_cv_sampled
from ls_spa._engine import debug_cv_lift_plan, debug_expand_groups

pytestmark = pytest.mark.gpu

T0, MG = 1e-10, 8


@functools.lru_cache(maxsize=None)
def case(p, K, kappa):
    """(X, y, ids, orderings, fold problems, scale); computed once and left unchanged."""
    n = K * (2 * p + 6) + 1
    Xa, _, ya, _ = hp_ref.gen(p, n, 1, kappa, 7000 + p)
    ids = (np.arange(n) % K).astype(np.int32)
    orders = hp_ref.orderings(p, 7000 + p, count=1)            # identity, reversed, one seeded
    for a in (Xa, ya, ids, orders):
        a.setflags(write=False)
    probs, scale = ref.fold_problems(Xa, ya, ids, K)
    return Xa, ya, ids, orders, probs, scale


@functools.lru_cache(maxsize=None)
def truth(p, K, kappa, anti):
    """(fold [3][K][p], total [3][p], e_plain of either)"""
    Xa, ya, ids, orders, probs, scale = case(p, K, kappa)
    fold, tot = ref.truth_lifts(probs, scale, orders, anti)
    pf, pt = ref.plain_lifts(Xa, ya, ids, K, 0.0, orders, anti)
    e_plain = float(max(np.nanmax(np.abs(pf - fold)), np.nanmax(np.abs(pt - tot))))
    fold.setflags(write=False)
    tot.setflags(write=False)
    return fold, tot, (e_plain if np.isfinite(e_plain) else 0.0)


def lifts_of(engine, p, K, kappa, orders, anti, accumulate=False):
    Xa, ya, ids = case(p, K, kappa)[:3]
    engine.cv_lift_load(Xa, ya, ids, K, 0.0)
    fold, tot = engine.cv_lift_batch(orders, anti, want_lifts=True, accumulate=accumulate)
    return fold, tot, engine.cv_lift_info()


def judge(name, got, want, e_plain):
    assert np.all(np.isfinite(got)), f"{name}: non-finite result"
    err, tol = float(np.abs(got - want).max()), max(T0, MG * e_plain)
    print(f"CVLIFT {name}: err {err:.3e} e_plain {e_plain:.3e} tol {tol:.3e}")
    assert err <= tol, f"{name}: |got - truth| = {err:.3e} > {tol:.3e} (e_plain {e_plain:.3e})"


# ---- truth -----------------------------------------------------------------------------------------------------------------
# (15, 2): p + 1 fills one block; (16, 3): the augmented row opens a block; (40, 32): the K limit; (111, 2): the last
# register-resident shape; (112, 2): the first LDS shape; (127, 2): the limit
TRUTH = [(9, 5), (15, 2), (16, 3), (40, 32), (111, 2), (112, 2), (127, 2)]


@pytest.mark.parametrize("kappa", [1e1, 1e4])
@pytest.mark.parametrize("p, K", TRUTH)
def test_fold_lifts_and_the_sum_against_the_long_double_truth(engine, p, K, kappa):
    orders = case(p, K, kappa)[3]
    try:
        for anti in (False, True):
            fold, tot, info = lifts_of(engine, p, K, kappa, orders, anti)
            assert fold.shape == (len(orders), K, p) and tot.shape == (len(orders), p)
            assert not info.any(), f"p={p} K={K} kappa={kappa:g}: flagged {info} (no case here may be)"
            want_fold, want_tot, e_plain = truth(p, K, kappa, anti)
            judge(f"folds p={p} K={K} kappa={kappa:g} anti={int(anti)}", fold, want_fold, e_plain)
            judge(f"sum   p={p} K={K} kappa={kappa:g} anti={int(anti)}", tot, want_tot, e_plain)
    finally:
        engine.cv_lift_free()


# ---- fold problems ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p, K", [(9, 5), (16, 3), (32, 4), (40, 32), (112, 2), (127, 2)])
def test_fold_problems_against_long_double_grams(engine, p, K):
    if (p, K) == (32, 4):
        n = K * (2 * p + 6) + 1
        Xa, _, ya, _ = hp_ref.gen(p, n, 1, 1e1, 7000 + p)
        ids = (np.arange(n) % K).astype(np.int32)
    else:
        Xa, ya, ids = case(p, K, 1e1)[:3]
    n = len(ya)
    Xl, yl = np.asarray(Xa, dtype=np.longdouble), np.asarray(ya, dtype=np.longdouble)
    yy = (yl * yl).sum()
    try:
        engine.cv_lift_load(Xa, ya, ids, K, 0.25)
        got = [engine.cv_lift_problem(f) for f in range(K)]
        exact = None
        if p <= 32:
            engine.cv_load(Xa, ya, ids, K, 0.25)
            exact = [engine.cv_get_problem(f) for f in range(K)]
    finally:
        engine.cv_lift_free()
        engine.cv_free()
    for f in range(K):
        tr, te = ids != f, ids == f
        nt = int(tr.sum())
        want = (Xl[tr].T @ Xl[tr] / nt + np.longdouble(0.25) * np.eye(p), Xl[tr].T @ yl[tr] / nt, Xl[te].T @ Xl[te],
                Xl[te].T @ yl[te], 1 / yy)
        for name, a, b in zip("GgHhy", got[f], want):
            b = np.asarray(b, dtype=np.float64)
            assert np.abs(np.asarray(a) - b).max() <= 1e-13 * np.abs(b).max(), f"{name} of fold {f}"
        if exact is not None:
            for name, a, b in zip("GgHhy", got[f], exact[f]):
                assert np.abs(np.asarray(a) - np.asarray(b)).max() <= 1e-13 * np.abs(np.asarray(b)).max(), \
                    f"{name} of fold {f} against lsspa_cv_get_problem"


# ---- against the one-response path -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [40, 112])
def test_a_folds_lifts_against_the_one_response_kernels(engine, p):
    K, kappa = (32, 1e1) if p == 40 else (2, 1e1)
    Xa, ya, ids, orders = case(p, K, kappa)[:4]
    yy = float(ya @ ya)
    try:
        for anti in (False, True):
            fold, _, info = lifts_of(engine, p, K, kappa, orders, anti)
            assert not info.any()
            _, _, e_plain = truth(p, K, kappa, anti)
            for f in ((0, 13, 31) if K == 32 else range(K)):
                tr, te = ids != f, ids == f
                engine.load_data(Xa[tr], Xa[te], ya[tr], ya[te], 0.0)
                one = engine.run_batch(orders, anti, want_lifts=True, accumulate=False)
                assert engine.info() & 1 == 0
                one = one * (float(ya[te] @ ya[te]) / yy)
                err, tol = float(np.abs(fold[:, f] - one).max()), max(T0, MG * e_plain)
                print(f"CVLIFT one-response p={p} anti={int(anti)} f={f}: |cv - one| {err:.3e} tol {tol:.3e}")
                assert err <= tol
    finally:
        engine.cv_lift_free()


# ---- bitwise ---------------------------------------------------------------------------------------------------------------
BITS = [(9, 3), (112, 2)]


@functools.lru_cache(maxsize=None)
def bit_orders(p):
    rng = np.random.default_rng(99 + p)
    o = np.array([rng.permutation(p) for _ in range(7)], dtype=np.int32)
    o.setflags(write=False)
    return o


@pytest.mark.parametrize("p, K", BITS)
def test_bitwise_contracts(engine, p, K):
    orders = bit_orders(p)
    try:
        out = {anti: lifts_of(engine, p, K, 1e1, orders, anti)[:2] for anti in (False, True)}
        for anti in (False, True):
            fold, tot = out[anti]
            # two calls agree
            again = engine.cv_lift_batch(orders, anti, want_lifts=True, accumulate=False)
            np.testing.assert_array_equal(again[0], fold)
            np.testing.assert_array_equal(again[1], tot)
            # a batch cut in two; a sample placed inside another batch
            a = engine.cv_lift_batch(orders[:3], anti, want_lifts=True, accumulate=False)
            b = engine.cv_lift_batch(orders[3:], anti, want_lifts=True, accumulate=False)
            np.testing.assert_array_equal(np.concatenate([a[0], b[0]]), fold)
            np.testing.assert_array_equal(np.concatenate([a[1], b[1]]), tot)
            mixed = engine.cv_lift_batch(orders[[5, 2, 6, 2, 0]], anti, want_lifts=True, accumulate=False)
            np.testing.assert_array_equal(mixed[0][1], fold[2])
            np.testing.assert_array_equal(mixed[0][3], fold[2])
            np.testing.assert_array_equal(mixed[1][1], tot[2])
            # the sum is the ascending fold sum
            s = fold[:, 0].copy()
            for f in range(1, K):
                s = s + fold[:, f]
            np.testing.assert_array_equal(tot, s)
            # accumulate on or off
            acc = engine.cv_lift_batch(orders, anti, want_lifts=True, accumulate=True)
            np.testing.assert_array_equal(acc[0], fold)
            np.testing.assert_array_equal(acc[1], tot)
        # the antithetical pair is 0.5 a + 0.5 b of the two orderings run as plain samples
        rev = engine.cv_lift_batch(np.ascontiguousarray(orders[:, ::-1]), False, want_lifts=True, accumulate=False)
        np.testing.assert_array_equal(out[True][0], 0.5 * out[False][0] + 0.5 * rev[0])
    finally:
        engine.cv_lift_free()


@pytest.mark.parametrize("p, K", BITS)
def test_a_batch_of_two_launches_equals_its_halves(engine, p, K):
    anti = True
    S = debug_cv_lift_plan(p, p, K, 1 << 20, anti)["samples_per_launch"]
    B = S + 3
    plan = debug_cv_lift_plan(p, p, K, B, anti)
    assert plan["launches"] == 2 and plan["samples_per_launch"] == S
    rng = np.random.default_rng(5 + p)
    base = np.array([rng.permutation(p) for _ in range(16)], dtype=np.int32)
    orders = np.ascontiguousarray(base[rng.integers(0, 16, size=B)])
    Xa, ya, ids = case(p, K, 1e1)[:3]
    try:
        engine.cv_lift_load(Xa, ya, ids, K, 0.0)
        fold, tot = engine.cv_lift_batch(orders, anti, want_lifts=True, accumulate=False)
        h = B // 2
        a = engine.cv_lift_batch(orders[:h], anti, want_lifts=True, accumulate=False)
        b = engine.cv_lift_batch(orders[h:], anti, want_lifts=True, accumulate=False)
    finally:
        engine.cv_lift_free()
    np.testing.assert_array_equal(np.concatenate([a[0], b[0]]), fold)
    np.testing.assert_array_equal(np.concatenate([a[1], b[1]]), tot)


# ---- groups ------------------------------------------------------------------------------------------------------------------
def group_case(p):
    if p == 20:
        labels = np.array([-1, 0, 1, 2, 0, 3, 4, 5, 1, -1, 2, 3, 4, 5, 0, 1, 2, 3, 4, 5], dtype=np.int32)
        return labels, 6, 3
    labels = (np.arange(p) * 7 % 5).astype(np.int32)
    return labels, 5, 2


def expanded_rows(labels, gperms, anti):
    """The column orderings of the header: the baseline first, every group's columns contiguous and ascending; a pair's
    second row is the expansion of the reversed group ordering (lsspa_debug_expand_groups' own pair reads the forward
    row backwards when there is no baseline, the one-response path's layout: the rows are expanded one by one here)."""
    fwd = debug_expand_groups(labels, gperms, False)
    if not anti:
        return fwd
    rev = debug_expand_groups(labels, np.ascontiguousarray(gperms[:, ::-1]), False)
    return np.ascontiguousarray(np.stack([fwd, rev], axis=1).reshape(2 * len(gperms), -1))


@pytest.mark.parametrize("p", [20, 112])
def test_group_lifts_are_the_fold_of_the_column_call_and_the_truth(engine, p):
    labels, g, K = group_case(p)
    Xa, ya, ids, _, probs, scale = case(p, K, 1e1)
    rng = np.random.default_rng(p)
    gperms = np.array([np.arange(g), np.arange(g)[::-1], rng.permutation(g)], dtype=np.int32)
    try:
        engine.cv_lift_load(Xa, ya, ids, K, 0.0)
        for anti in (False, True):
            rows = expanded_rows(labels, gperms, anti)
            engine.cv_lift_clear_players()
            col = engine.cv_lift_batch(rows, False, want_lifts=True, accumulate=False)[0]      # [B per][K][p]
            engine.cv_lift_set_players(labels)
            fold, tot = engine.cv_lift_batch(gperms, anti, want_lifts=True, accumulate=False)
            assert fold.shape == (3, K, g) and tot.shape == (3, g) and not engine.cv_lift_info().any()
            want = ref.group_fold(col, labels)
            if anti:
                want = 0.5 * want[0::2] + 0.5 * want[1::2]
            assert np.array_equal(fold, want)
            s = want[:, 0].copy()
            for f in range(1, K):
                s = s + want[:, f]
            assert np.array_equal(tot, s)
            # the truth: the long-double column lifts of the expanded rows, folded
            tf, _ = ref.truth_lifts(probs, scale, rows, False)
            pf, _ = ref.plain_lifts(Xa, ya, ids, K, 0.0, rows, False)
            tg, pg = ref.group_fold(tf, labels), ref.group_fold(pf, labels)
            if anti:
                tg, pg = 0.5 * tg[0::2] + 0.5 * tg[1::2], 0.5 * pg[0::2] + 0.5 * pg[1::2]
            judge(f"groups p={p} anti={int(anti)}", fold, tg, float(np.abs(pg - tg).max()))
    finally:
        engine.cv_lift_free()


# ---- running statistics --------------------------------------------------------------------------------------------------------
def test_running_statistics_against_numpy(engine):
    p, K = 16, 3
    Xa, ya, ids = case(p, K, 1e1)[:3]
    rng = np.random.default_rng(24)
    batches = [np.array([rng.permutation(p) for _ in range(b)], dtype=np.int32) for b in (5, 1, 6)]
    try:
        engine.cv_lift_load(Xa, ya, ids, K, 0.0)
        n0, mean0, m20 = engine.cv_lift_get()
        assert n0 == 0 and not mean0.any() and not m20.any()
        outs = [engine.cv_lift_batch(b, True, want_lifts=True, accumulate=True) for b in batches]
        x = np.concatenate([np.concatenate([f, t[:, None]], axis=1) for f, t in outs])      # [12][K + 1][p]
        n, mean, m2 = engine.cv_lift_get()
        assert n == 12 and mean.shape == (K + 1, p) and m2.shape == (K + 1, p)
        want_mean = x.mean(axis=0)
        want_m2 = ((x - want_mean) ** 2).sum(axis=0)
        print(f"CVLIFT stats: mean {np.abs(mean - want_mean).max():.3e}, M2 rel {np.abs(m2 / want_m2 - 1).max():.3e}")
        np.testing.assert_allclose(mean, want_mean, rtol=0, atol=1e-14)
        np.testing.assert_allclose(m2, want_m2, rtol=1e-12, atol=0)
        engine.cv_lift_batch(batches[0], True, accumulate=False)      # accumulate = 0 leaves the state alone
        n_b, mean_b, m2_b = engine.cv_lift_get()
        assert n_b == n
        np.testing.assert_array_equal(mean_b, mean)
        np.testing.assert_array_equal(m2_b, m2)
        engine.cv_lift_reset()
        assert engine.cv_lift_get()[0] == 0
    finally:
        engine.cv_lift_free()


# ---- the public call -----------------------------------------------------------------------------------------------------------
def test_public_call_with_all_orderings_is_ls_spa_cv():
    p, K = 6, 3
    Xa, _, ya, _ = hp_ref.gen(p, 61, 1, 1e1, 606)
    res = ls_spa_cv_sampled(Xa, ya, 0.1, K, method="exact", antithetical=False, max_samples=1000)
    want = ls_spa_cv(Xa, ya, 0.1, K)
    assert res.n_samples == 720
    np.testing.assert_array_equal(res.fold_ids, want.fold_ids)
    np.testing.assert_allclose(res.attribution, want.attribution, rtol=0, atol=1e-10)
    np.testing.assert_allclose(res.fold_attribution, want.fold_attribution, rtol=0, atol=1e-10)
    np.testing.assert_allclose(res.fold_r_squared, want.fold_r_squared, rtol=0, atol=1e-10)
    assert abs(res.r_squared - want.r_squared) <= 1e-10
    np.testing.assert_allclose(res.theta, want.theta, rtol=1e-9, atol=1e-12)


def test_public_call_over_groups_is_ls_spa_cv_over_groups():
    p, K = 12, 3
    labels = np.array([-1, 0, 1, 2, 3, 4, 0, 1, 2, 3, 4, 0])
    Xa, _, ya, _ = hp_ref.gen(p, 100, 1, 1e1, 1212)
    res = ls_spa_cv_sampled(Xa, ya, 0.0, K, groups=labels, method="exact", antithetical=False, max_samples=1000)
    want = ls_spa_cv(Xa, ya, 0.0, K, groups=labels)
    assert res.n_samples == 120 and res.attribution.shape == (5,)
    np.testing.assert_allclose(res.attribution, want.attribution, rtol=0, atol=1e-10)
    np.testing.assert_allclose(res.fold_attribution, want.fold_attribution, rtol=0, atol=1e-10)
    np.testing.assert_allclose(res.fold_r_squared, want.fold_r_squared, rtol=0, atol=1e-10)
    np.testing.assert_allclose(res.fold_baseline_r_squared, want.fold_baseline_r_squared, rtol=0, atol=1e-10)
    assert abs(res.r_squared - want.r_squared) <= 1e-10
    assert abs(res.baseline_r_squared - want.baseline_r_squared) <= 1e-10


def test_public_call_sums_repeats_and_stops():
    p, K = 60, 5
    Xa, _, ya, _ = hp_ref.gen(p, K * (2 * p + 6) + 1, 1, 1e1, 6060)
    res = ls_spa_cv_sampled(Xa, ya, 0.0, K, max_samples=64, batch_size=32)
    assert res.n_samples == 64 and res.attribution.shape == (p,) and res.fold_attribution.shape == (K, p)
    assert res.attribution_errors.shape == (p,) and res.fold_attribution_errors.shape == (K, p)
    print(f"CVLIFT public: |sum - R^2| {abs(res.attribution.sum() - res.r_squared):.3e}, |folds - sum| "
          f"{np.abs(res.fold_attribution.sum(axis=0) - res.attribution).max():.3e}")
    assert abs(res.attribution.sum() - res.r_squared) <= 1e-12
    np.testing.assert_allclose(res.fold_attribution.sum(axis=0), res.attribution, rtol=0, atol=1e-12)
    again = ls_spa_cv_sampled(Xa, ya, 0.0, K, max_samples=64, batch_size=32)
    np.testing.assert_array_equal(again.attribution, res.attribution)
    np.testing.assert_array_equal(again.fold_attribution, res.fold_attribution)
    np.testing.assert_array_equal(again.attribution_errors, res.attribution_errors)
    early = ls_spa_cv_sampled(Xa, ya, 0.0, K, max_samples=4096, batch_size=32, tolerance=1.0)
    assert early.n_samples == 32 and early.attribution_errors.max() <= 1.0


# ---- flags and isolation -------------------------------------------------------------------------------------------------------
def test_a_duplicated_column_raises_the_warning_that_names_folds():
    p, K = 8, 3
    Xa, _, ya, _ = hp_ref.gen(p, 91, 1, 1e1, 88)
    Xa = Xa.copy()
    Xa[:, 5] = Xa[:, 2]
    with pytest.warns(RuntimeWarning, match=r"fold\(s\) 0, 1, 2"):
        ls_spa_cv_sampled(Xa, ya, 0.0, K, max_samples=8, batch_size=8)


def test_the_other_stores_are_left_alone(engine):
    p = 12
    one = hp_ref.gen(p, 60, 40, 1e1, 12)
    o1 = hp_ref.orderings(p, 12)
    engine.load_data(*one, 0.0)
    engine.full_fit()
    before = engine.run_batch(o1, True, want_lifts=True, accumulate=True)
    stats_before, info_before, gram_before = engine.stats(), engine.info(), engine.gram()
    Xc, _, yc, _ = hp_ref.gen(6, 61, 1, 1e1, 6)
    idc = (np.arange(61) % 3).astype(np.int32)
    engine.cv_load(Xc, yc, idc, 3, 0.0)
    cv_before = engine.cv_shapley()
    Ym = np.stack([one[2], one[2] ** 2], axis=1), np.stack([one[3], one[3] ** 2], axis=1)
    engine.multi_lift_load(one[0], one[1], Ym[0], Ym[1], 0.0)
    ml_before = engine.multi_lift_batch(o1, True, want_lifts=True, accumulate=True)
    ml_state = engine.multi_lift_get()
    try:
        fold, tot, info = lifts_of(engine, 16, 3, 1e1, case(16, 3, 1e1)[3], True, accumulate=True)
        assert not info.any() and fold.shape == (3, 3, 16)
    finally:
        engine.cv_lift_free()
    assert engine.info() == info_before
    for a, b in zip(engine.stats(), stats_before):
        np.testing.assert_array_equal(a, b)
    for a, b in zip(engine.gram(), gram_before):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(engine.run_batch(o1, True, want_lifts=True, accumulate=False), before)
    for a, b in zip(engine.cv_shapley(), cv_before):
        np.testing.assert_array_equal(a, b)
    engine.cv_free()
    for a, b in zip(engine.multi_lift_get(), ml_state):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(engine.multi_lift_batch(o1, True, want_lifts=True, accumulate=False), ml_before)
    engine.multi_lift_free()


# ---- engine errors -----------------------------------------------------------------------------------------------------------
def test_errors_of_the_engine(engine):
    engine.cv_lift_free()
    for call in (lambda: engine.cv_lift_batch(np.arange(4, dtype=np.int32)[None], False), engine.cv_lift_get,
                 engine.cv_lift_info, engine.cv_lift_reset, lambda: engine.cv_lift_problem(0),
                 lambda: engine.cv_lift_set_players(np.zeros(4, dtype=np.int32))):
        with pytest.raises(Exception, match="comes first") as e:      # LSSPA_ERR_STATE before a load
            call()
        assert not isinstance(e.value, ValueError)
    z = np.zeros
    ids2 = lambda n, K: (np.arange(n) % K).astype(np.int32)      # noqa: E731
    with pytest.raises(ValueError, match="at most p = 127"):
        engine.cv_lift_load(z((400, 128)), z(400), ids2(400, 2), 2, 0.0)
    for K in (1, 33):
        with pytest.raises(ValueError, match="2 .. 32 folds"):
            engine.cv_lift_load(z((400, 4)), z(400), ids2(400, 2), K, 0.0)
    Xa, ya, ids, orders = case(9, 3, 1e1)[:4]
    short = np.concatenate([ids[ids != 1], np.ones(8, dtype=np.int32)])      # fold 1 with p - 1 rows
    with pytest.raises(ValueError, match="fold 1 of 3 has 8 rows, fewer than p = 9"):
        engine.cv_lift_load(Xa[:len(short)], ya[:len(short)], short, 3, 0.0)
    with pytest.raises(Exception, match="comes first"):              # a refused load leaves nothing loaded
        engine.cv_lift_get()
    engine.cv_lift_load(Xa, ya, ids, 3, 0.0)
    try:
        bad = orders.copy()
        bad[1, 3] = bad[1, 4]
        with pytest.raises(ValueError, match="not a permutation"):
            engine.cv_lift_batch(bad, False)
        with pytest.raises(ValueError, match="perms is NULL"):
            engine.cv_lift_batch(orders[:0], False)
        assert engine.cv_lift_get()[0] == 0                          # none of them ran
        t = engine.cv_lift_timing()
        assert set(t) == {"gram", "batch", "stats"} and t["gram"] > 0
    finally:
        engine.cv_lift_free()


def test_repeated_load_and_free_leaves_free_memory_where_it_was(engine):
    import torch
    Xa, ya, ids = case(16, 3, 1e1)[:3]

    def cycle():
        engine.cv_lift_load(Xa, ya, ids, 3, 0.0)
        engine.cv_lift_set_players((np.arange(16) % 4).astype(np.int32))
        engine.cv_lift_batch(np.array([[0, 1, 2, 3], [3, 1, 0, 2]], dtype=np.int32), True)
        engine.cv_lift_free()

    cycle()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(3):
        cycle()
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    assert free1 == free0, (free0, free1)
    assert getattr(engine, "_cv_lift_dims", None) is None
