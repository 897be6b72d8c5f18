"""ls_spa_multi_sampled on the MI355X (csrc/k_small_multi.hip, lsspa_multi_lift_* of include/lsspa.h): every response's
lift vectors against the long-double truth of tests/hp_ref.py at every edge of the augmented rows' layout, against the
one-response kernels, and -- bitwise -- that a response's lifts do not depend on the other responses, on the batch or on
how it is cut; the running statistics against NumPy; the pivot flag; that nothing else of the context is touched.

Tolerance: the rule of tests/test_gpu_accuracy.py, tol = max(1e-10, 8 e_plain) with e_plain the error of NumPy / LAPACK
(hp_ref.plain_lifts) on the same case; a case the engine flags NOT_PD is excused only if the truth's smallest relative
pivot is within 100 x of the engine's threshold 16 p eps."""
import functools
import warnings

import numpy as np
import pytest

import hp_ref
from ls_spa import ls_spa, ls_spa_multi_sampled
from ls_spa._engine import HipEngine
from test_multi_host import with_responses

pytestmark = pytest.mark.gpu

EPS = 2.220446049250313e-16
T0, MG, EXCUSE = 1e-10, 8, 100
M_MAX = 11
MAX_P = HipEngine.MULTI_LIFT_MAX_P


def threshold(p):
    return 16 * p * EPS


@functools.lru_cache(maxsize=None)
def case(p, kappa, m=M_MAX):
    """(data with m responses, orderings, per response the long-double problem); fewer responses are the first columns.
    Computed once and left unchanged."""
    Xa, Xe, ya, ye = hp_ref.gen(p, 3 * p + 5, p + 3, kappa, 9000 + p)
    d = with_responses(Xa, Xe, ya, ye, m, 9000 + p)
    orders = hp_ref.orderings(p, 9000 + p, count=1)            # identity, reversed, one seeded
    for a in d + (orders,):
        a.setflags(write=False)
    refs = [hp_ref.Problem(d[0], d[1], d[2][:, r], d[3][:, r]) for r in range(m)]
    return d, orders, refs


@functools.lru_cache(maxsize=None)
def truth(p, kappa, r, anti):
    """(long-double lifts [3][p], e_plain, true smallest pivot / threshold) of response r."""
    d, orders, refs = case(p, kappa)
    want = refs[r].lifts(orders, anti)
    plain = hp_ref.plain_lifts(d[0], d[1], d[2][:, r], d[3][:, r], 0.0, orders, anti)
    e_plain = float(np.nanmax(np.abs(plain - want)))
    want.setflags(write=False)
    return want, (e_plain if np.isfinite(e_plain) else 0.0), min(refs[r].min_pivot, refs[r].min_pivot_test) / threshold(p)


def first(d, m):
    return d[0], d[1], d[2][:, :m], d[3][:, :m]


def judge(name, got, want, e_plain, not_pd, ratio):
    if ratio >= EXCUSE:
        assert not not_pd, f"{name}: NOT_PD with the true smallest pivot {ratio:.3g} x the threshold"
    if not_pd:
        print(f"MLIFT {name}: NOT_PD (true pivot / threshold = {ratio:.3g}): excused")
        return
    assert np.all(np.isfinite(got)), f"{name}: non-finite result without NOT_PD"
    err, tol = float(np.abs(got - want).max()), max(T0, MG * e_plain)
    print(f"MLIFT {name}: err {err:.3e} e_plain {e_plain:.3e} tol {tol:.3e} pivot/threshold {ratio:.3g}")
    assert err <= tol, f"{name}: |got - truth| = {err:.3e} > {tol:.3e} (e_plain {e_plain:.3e})"


def lifts_of(engine, d, orders, anti):
    engine.multi_lift_load(*d, 0.0)
    out = engine.multi_lift_batch(orders, anti, want_lifts=True, accumulate=False)
    return out, engine.multi_lift_info()


# ---- truth ---------------------------------------------------------------------------------------------------------------
# p = 7: p + 8 = 15, one block with identity padding inside; 8: fills the block; 9: the augmented rows straddle blocks 0 and
# 1; 16: they start a block; 104: p + 8 = 112 fills the seven block rows.  m = 9: one response in a second chunk; m = 1:
# seven padded slots.
TRUTH = [(7, 9), (8, 11), (9, 1), (9, 8), (9, 9), (9, 11), (16, 9), (24, 11), (40, 9), (100, 11),
         (104, 1), (104, 8), (104, 9), (104, 11)]


@pytest.mark.parametrize("kappa", [1e1, 1e4])
@pytest.mark.parametrize("p, m", TRUTH)
def test_lifts_against_the_long_double_truth(engine, p, m, kappa):
    d, orders, _ = case(p, kappa)
    try:
        for anti in (False, True):
            got, info = lifts_of(engine, first(d, m), orders, anti)
            assert got.shape == (len(orders), m, p)
            for r in range(m):
                want, e_plain, ratio = truth(p, kappa, r, anti)
                judge(f"p={p} m={m} kappa={kappa:g} anti={int(anti)} r={r}", got[:, r], want, e_plain, info & 1, ratio)
            assert info & ~1 == 0
    finally:
        engine.multi_lift_free()


# ---- against the one-response path -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [40, 100])
def test_rows_against_the_one_response_kernels(engine, p):
    kappa, m = 1e1, 9
    d, orders, _ = case(p, kappa)
    try:
        for anti in (False, True):
            got, info = lifts_of(engine, first(d, m), orders, anti)
            assert info == 0
            for r in range(m):
                engine.load_data(d[0], d[1], d[2][:, r], d[3][:, r], 0.0)
                one = engine.run_batch(orders, anti, want_lifts=True, accumulate=False)
                assert engine.info() & 1 == 0
                _, e_plain, _ = truth(p, kappa, r, anti)
                err, tol = float(np.abs(got[:, r] - one).max()), max(T0, MG * e_plain)
                print(f"MLIFT one-response p={p} anti={int(anti)} r={r}: |multi - one| {err:.3e} tol {tol:.3e}")
                assert err <= tol
    finally:
        engine.multi_lift_free()


# ---- bitwise ---------------------------------------------------------------------------------------------------------------
P_BIT, KAPPA_BIT = 9, 1e1


@pytest.fixture(scope="module")
def bits(engine):
    d, _, _ = case(P_BIT, KAPPA_BIT)
    rng = np.random.default_rng(99)
    orders = np.array([rng.permutation(P_BIT) for _ in range(7)], dtype=np.int32)
    out = {anti: lifts_of(engine, d, orders, anti)[0] for anti in (False, True)}
    engine.multi_lift_free()
    return d, orders, out


@pytest.mark.parametrize("anti", [False, True])
def test_two_calls_agree(engine, bits, anti):
    d, orders, out = bits
    got, _ = lifts_of(engine, d, orders, anti)
    engine.multi_lift_free()
    np.testing.assert_array_equal(got, out[anti])


@pytest.mark.parametrize("r", [2, 9])
def test_the_other_responses_do_not_change_a_bit(engine, bits, r):
    d, orders, out = bits
    rng = np.random.default_rng(5 + r)
    Ya, Ye = rng.standard_normal(d[2].shape) * 3.0, rng.standard_normal(d[3].shape) * 3.0
    Ya[:, r], Ye[:, r] = d[2][:, r], d[3][:, r]
    for anti in (False, True):
        got, _ = lifts_of(engine, (d[0], d[1], Ya, Ye), orders, anti)
        np.testing.assert_array_equal(got[:, r], out[anti][:, r])
        assert np.abs(got[:, (r + 1) % M_MAX] - out[anti][:, (r + 1) % M_MAX]).max() > 1e-6
    engine.multi_lift_free()


def test_fewer_responses_behind_it_do_not_change_a_bit(engine, bits):
    d, orders, out = bits
    got, _ = lifts_of(engine, first(d, 3), orders, True)
    engine.multi_lift_free()
    np.testing.assert_array_equal(got, out[True][:, :3])


@pytest.mark.parametrize("anti", [False, True])
def test_a_batch_cut_in_two_and_a_sample_inside_another_batch(engine, bits, anti):
    d, orders, out = bits
    engine.multi_lift_load(*d, 0.0)
    head = engine.multi_lift_batch(orders[:3], anti, want_lifts=True, accumulate=False)
    tail = engine.multi_lift_batch(orders[3:], anti, want_lifts=True, accumulate=False)
    rng = np.random.default_rng(17)
    other = np.array([rng.permutation(P_BIT) for _ in range(5)], dtype=np.int32)
    other[2] = orders[4]
    mid = engine.multi_lift_batch(other, anti, want_lifts=True, accumulate=False)
    engine.multi_lift_free()
    np.testing.assert_array_equal(np.concatenate([head, tail]), out[anti])
    np.testing.assert_array_equal(mid[2], out[anti][4])


def test_another_slot_agrees_to_the_tolerance(engine):
    """Independence of the slot is not promised (the augmented rows may straddle a block edge): to the tolerance."""
    d, orders, _ = case(P_BIT, KAPPA_BIT)
    r = 3
    alone = (d[0], d[1], d[2][:, [r]], d[3][:, [r]])
    cols = [0, 1, 2, 4, 5, r]                                   # response r in slot 5
    moved = (d[0], d[1], d[2][:, cols], d[3][:, cols])
    try:
        for anti in (False, True):
            a, _ = lifts_of(engine, alone, orders, anti)
            b, _ = lifts_of(engine, moved, orders, anti)
            _, e_plain, _ = truth(P_BIT, KAPPA_BIT, r, anti)
            err, tol = float(np.abs(a[:, 0] - b[:, 5]).max()), max(T0, MG * e_plain)
            print(f"MLIFT slots 0 and 5, anti={int(anti)}: {err:.3e} tol {tol:.3e}")
            assert err <= tol
    finally:
        engine.multi_lift_free()


# ---- statistics --------------------------------------------------------------------------------------------------------------
def test_running_statistics_against_numpy(engine):
    p, m = 24, 11
    d, _, _ = case(p, 1e1)
    rng = np.random.default_rng(24)
    batches = [np.array([rng.permutation(p) for _ in range(b)], dtype=np.int32) for b in (5, 1, 6)]
    try:
        engine.multi_lift_load(*first(d, m), 0.0)
        n0, mean0, m20 = engine.multi_lift_get()
        assert n0 == 0 and not mean0.any() and not m20.any()

        def run():
            return [engine.multi_lift_batch(b, True, want_lifts=True, accumulate=True) for b in batches]

        x = np.concatenate(run())
        n, mean, m2 = engine.multi_lift_get()
        assert n == 12 and mean.shape == (m, p) and m2.shape == (m, p)
        want_mean = x.mean(axis=0)
        want_m2 = ((x - want_mean) ** 2).sum(axis=0)
        print(f"MLIFT stats: mean {np.abs(mean - want_mean).max():.3e}, M2 rel {np.abs(m2 / want_m2 - 1).max():.3e}")
        np.testing.assert_allclose(mean, want_mean, rtol=0, atol=1e-14)
        np.testing.assert_allclose(m2, want_m2, rtol=1e-12, atol=0)
        # accumulate = 0 leaves the state alone
        engine.multi_lift_batch(batches[0], True, want_lifts=False, accumulate=False)
        n_b, mean_b, m2_b = engine.multi_lift_get()
        assert n_b == n
        np.testing.assert_array_equal(mean_b, mean)
        np.testing.assert_array_equal(m2_b, m2)
        # the same batches again after a reset: the same bits
        engine.multi_lift_reset()
        assert engine.multi_lift_get()[0] == 0
        np.testing.assert_array_equal(np.concatenate(run()), x)
        n_c, mean_c, m2_c = engine.multi_lift_get()
        assert n_c == n
        np.testing.assert_array_equal(mean_c, mean)
        np.testing.assert_array_equal(m2_c, m2)
    finally:
        engine.multi_lift_free()


# ---- the pivot flag ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [9, 24])
def test_a_response_in_the_span_of_x_is_not_flagged(engine, p):
    """The Schur complement of its augmented row is exactly zero in both matrices: only the pivots j < p count."""
    d, orders, _ = case(p, 1e1)
    m = 9
    Xa, Xe, Ya, Ye = (a.copy() for a in first(d, m))
    w = np.random.default_rng(p).integers(-3, 4, p).astype(np.float64)
    for r in (1, 8):
        Ya[:, r], Ye[:, r] = Xa @ w, Xe @ w
    try:
        for anti in (False, True):
            got, info = lifts_of(engine, (Xa, Xe, Ya, Ye), orders, anti)
            assert info == 0
            assert np.all(np.isfinite(got))
            np.testing.assert_allclose(got[:, [1, 8]].sum(axis=2), 1.0, rtol=0, atol=1e-9)     # R^2 = 1
            for r in (0, 2, 7):                                  # the neighbours are the truth's as ever
                want, e_plain, ratio = truth(p, 1e1, r, anti)
                judge(f"span p={p} anti={int(anti)} r={r}", got[:, r], want, e_plain, 0, ratio)
    finally:
        engine.multi_lift_free()


def test_a_duplicated_column_is_flagged_and_the_driver_warns(engine):
    p, m = 16, 9
    d, orders, _ = case(p, 1e1)
    Xa, Xe, Ya, Ye = (a.copy() for a in first(d, m))
    Xa[:, 11], Xe[:, 11] = Xa[:, 4], Xe[:, 4]
    try:
        _, info = lifts_of(engine, (Xa, Xe, Ya, Ye), orders, False)
        assert info & 1
    finally:
        engine.multi_lift_free()
    with pytest.warns(RuntimeWarning, match="not numerically positive definite"):
        res = ls_spa_multi_sampled(Xa, Xe, Ya, Ye, perms=orders)
    assert res.attribution.shape == (m, p) and np.isfinite(res.theta).all()


# ---- isolation -----------------------------------------------------------------------------------------------------------------
def test_the_loaded_problem_and_the_exact_state_are_left_alone(engine):
    p = 12
    d, orders, _ = case(16, 1e1)
    one = hp_ref.gen(p, 60, 40, 1e1, 12)
    o1 = hp_ref.orderings(p, 12)
    engine.load_data(*one, 0.0)
    engine.full_fit()
    before = engine.run_batch(o1, True, want_lifts=True, accumulate=True)
    stats_before, info_before, gram_before = engine.stats(), engine.info(), engine.gram()
    small = with_responses(*hp_ref.gen(6, 40, 20, 1e1, 6), 3, 6)
    engine.multi_load(*small, 0.0)
    phi_before, _ = engine.multi_shapley()
    try:
        got, info = lifts_of(engine, first(d, 9), orders, True)
        engine.multi_lift_batch(orders, True, accumulate=True)
        assert info == 0 and got.shape == (len(orders), 9, 16)
    finally:
        engine.multi_lift_free()
    assert engine.info() == info_before
    for a, b in zip(engine.stats(), stats_before):
        np.testing.assert_array_equal(a, b)
    for a, b in zip(engine.gram(), gram_before):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(engine.run_batch(o1, True, want_lifts=True, accumulate=False), before)
    phi_after, _ = engine.multi_shapley()
    engine.multi_free()
    np.testing.assert_array_equal(phi_after, phi_before)


# ---- engine errors -----------------------------------------------------------------------------------------------------------
def test_errors_of_the_engine(engine):
    import ctypes as C
    engine.multi_lift_free()
    for call in (lambda: engine.multi_lift_batch(np.arange(4, dtype=np.int32)[None], False), engine.multi_lift_get,
                 engine.multi_lift_info, engine.multi_lift_reset, engine.multi_lift_gram):
        with pytest.raises(Exception, match="comes first") as e:      # LSSPA_ERR_STATE before a load
            call()
        assert not isinstance(e.value, ValueError)
    z = np.zeros
    with pytest.raises(ValueError, match=f"1 <= p <= {MAX_P}"):
        engine.multi_lift_load(z((400, MAX_P + 1)), z((200, MAX_P + 1)), z((400, 2)), z((200, 2)), 0.0)
    with pytest.raises(ValueError, match="M >= p test rows"):
        engine.multi_lift_load(z((40, 10)), z((9, 10)), z((40, 2)), z((9, 2)), 0.0)
    with pytest.raises(ValueError, match="p \\+ m <= 32767"):
        engine.multi_lift_load(z((10, 4)), z((10, 4)), z((10, 32764)), z((10, 32764)), 0.0)
    d, orders, _ = case(9, 1e1)
    Ye = d[3][:, :3].copy()
    Ye[:, 1] = 0.0
    with pytest.raises(ValueError, match="column 1 of Y_test is identically zero"):
        engine.multi_lift_load(d[0], d[1], d[2][:, :3], Ye, 0.0)
    with pytest.raises(Exception, match="comes first"):              # a refused load leaves nothing loaded
        engine.multi_lift_get()
    engine.multi_lift_load(*first(d, 3), 0.0)
    try:
        bad = orders.copy()
        bad[1, 3] = bad[1, 4]
        with pytest.raises(ValueError, match="not a permutation"):
            engine.multi_lift_batch(bad, False)
        with pytest.raises(ValueError, match="perms is NULL"):
            engine._check(engine._lib.lsspa_multi_lift_batch(engine._h, None, 3, 0, None, 0))
        with pytest.raises(ValueError, match="perms is NULL"):
            engine.multi_lift_batch(orders[:0], False)
        assert engine.multi_lift_get()[0] == 0                       # none of them ran
        t = engine.multi_lift_timing()
        assert set(t) == {"gram", "batch", "stats"} and t["gram"] > 0
    finally:
        engine.multi_lift_free()


def test_the_gram_form(engine):
    p, m = 16, 9
    d, orders, _ = case(p, 1e1)
    Xa, Xe, Ya, Ye = first(d, m)
    try:
        got, _ = lifts_of(engine, (Xa, Xe, Ya, Ye), orders, True)
        gram = engine.multi_lift_gram()
        engine.multi_lift_load_reduced(*gram)
        again = engine.multi_lift_batch(orders, True, want_lifts=True, accumulate=False)
        for a, b in zip(engine.multi_lift_gram(), gram):
            np.testing.assert_array_equal(a, b)
    finally:
        engine.multi_lift_free()
    np.testing.assert_array_equal(again, got)
    n = Xa.shape[0]
    np.testing.assert_allclose(gram[0], Xa.T @ Xa / n, rtol=0, atol=1e-12 * np.abs(gram[0]).max())
    np.testing.assert_allclose(gram[3], (Xe.T @ Ye).T, rtol=0, atol=1e-12 * np.abs(gram[3]).max())


# ---- the public call -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("anti", [False, True])
def test_public_call_against_ls_spa_per_response(anti):
    p, m, kappa = 40, 11, 1e1
    d, orders, _ = case(p, kappa)
    res = ls_spa_multi_sampled(*d, perms=orders, antithetical=anti)
    assert res.n_samples == len(orders) and res.attribution.shape == (m, p)
    np.testing.assert_allclose(res.attribution.sum(axis=1), res.r_squared, rtol=0, atol=1e-9)
    for r in range(m):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            one = ls_spa(d[0], d[1], d[2][:, r], d[3][:, r], perms=orders, antithetical=anti, tolerance=0.0)
        want, e_plain, _ = truth(p, kappa, r, anti)
        tol = max(T0, MG * e_plain)
        print(f"MLIFT public p={p} anti={int(anti)} r={r}: |multi - ls_spa| "
              f"{np.abs(res.attribution[r] - one.attribution).max():.3e} tol {tol:.3e}")
        assert np.abs(res.attribution[r] - one.attribution).max() <= tol
        assert np.abs(res.attribution[r] - want.mean(axis=0)).max() <= tol
        assert abs(res.r_squared[r] - one.r_squared) <= 1e-10
        np.testing.assert_allclose(res.theta[r], one.theta, rtol=1e-9, atol=1e-12)
