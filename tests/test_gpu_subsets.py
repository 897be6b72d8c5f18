"""ls_spa(method='subsets') on the MI355X: the exact attribution over all 2^p feature subsets (csrc/k_subsets.hip)
against the reference's exact results, the CPU oracle of tests/test_subsets_host.py, its own efficiency and
determinism -- and, with it as the truth, the sampling estimator's error bound at a size where sampling is used."""
import time

import numpy as np
import pytest

from ls_spa import ls_spa, workloads
from test_subsets_host import data, exact_shapley, gram_problem, mask_bits, subset_values

pytestmark = pytest.mark.gpu

LIFT_TOL = dict(rtol=0, atol=1e-10)
ORACLE_TOL = dict(rtol=0, atol=1e-11)


def _arrays(g):
    return [g[k] for k in ("X_train", "X_test", "y_train", "y_test")]


@pytest.mark.parametrize("name", ["toy", "exact_p4", "exact_p8"])
def test_reference_exact_fixtures(golden, name):
    g = golden(name)
    res = ls_spa(*_arrays(g), method="subsets")
    np.testing.assert_allclose(res.attribution, g["attribution"], **LIFT_TOL)
    np.testing.assert_allclose(res.theta, g["theta"], rtol=1e-9, atol=1e-12)
    assert abs(res.r_squared - float(g["r_squared"])) < 1e-12
    assert res.overall_error == 0.0 and res.error_history.shape == (0,) and res.attribution_history is None
    np.testing.assert_array_equal(res.attribution_errors, np.zeros(len(res.attribution)))


def test_p8_equals_the_ordering_mean(golden):
    d = _arrays(golden("exact_p8"))
    sub = ls_spa(*d, method="subsets")
    ex = ls_spa(*d, method="exact")
    np.testing.assert_allclose(sub.attribution, ex.attribution, rtol=0, atol=1e-12)
    np.testing.assert_array_equal(sub.theta, ex.theta)


@pytest.mark.parametrize("reg", [0.0, 0.1])
@pytest.mark.parametrize("p", [1, 2, 5, 9, 12, 16])
def test_against_the_cpu_oracle(p, reg):
    d = data(p, n=max(60, 3 * p), m=max(40, 2 * p), seed=100 + p)
    res = ls_spa(*d, reg=reg, method="subsets")
    phi = exact_shapley(*gram_problem(*d, reg=reg))
    np.testing.assert_allclose(res.attribution, phi, **ORACLE_TOL)
    assert abs(res.attribution.sum() - res.r_squared) < 1e-12


def test_p20_per_feature_against_the_cpu_oracle():
    """Several high subsets per unit (p >= 19): every phi_j, not only their sum."""
    d = data(20, n=300, m=150, seed=120)
    res = ls_spa(*d, reg=0.05, method="subsets")
    np.testing.assert_allclose(res.attribution, exact_shapley(*gram_problem(*d, reg=0.05)), **ORACLE_TOL)


def test_p28_column_permutation_permutes_phi(engine):
    """Several launches accumulating into the unit table (p >= 27): permuting the features permutes phi."""
    Xa, Xe, ya, ye = data(28, n=400, m=200, seed=280)
    perm = np.random.default_rng(28).permutation(28)
    engine.load_data(Xa, Xe, ya, ye, 0.0)
    phi, info = engine.subsets_shapley()
    assert engine.subsets_timing()[2] > 1
    engine.load_data(Xa[:, perm], Xe[:, perm], ya, ye, 0.0)
    phi_p, info_p = engine.subsets_shapley()
    assert info == info_p == 0
    np.testing.assert_allclose(phi_p, phi[perm], rtol=0, atol=1e-12)
    assert np.abs(phi).max() > 1e-3


def test_reduced_problem_with_many_test_columns(engine):
    """lsspa_set_reduced in rect mode with a long test factor (m = 3000 >> p): H = Ft Ft^T formed on the device."""
    rng = np.random.default_rng(31)
    p, m = 10, 3000
    A = rng.standard_normal((200, p))
    G = A.T @ A / 200 + 0.01 * np.eye(p)
    g = A.T @ rng.standard_normal(200) / 200
    Ft = rng.standard_normal((p, m))
    ytil = Ft.T @ rng.standard_normal(p) + rng.standard_normal(m)
    yy = float(ytil @ ytil)
    engine.load_reduced(G, g, float(g @ np.linalg.solve(G, g)) + 1.0, yy, Ft=Ft, ytil=ytil)
    phi, info = engine.subsets_shapley()
    assert info == 0
    np.testing.assert_allclose(phi, exact_shapley(G, g, Ft @ Ft.T, Ft @ ytil, yy), **ORACLE_TOL)


def test_kept_engine_float32_then_subsets():
    """A float32 sampling call leaves its precision on the kept engine; a subsets call after it still gives the fp64
    theta and r_squared of a fresh engine, and phi sums to that r_squared."""
    from ls_spa._engine import HipEngine
    d = data(14, n=300, m=150, seed=140)
    ls_spa(*d, method="argsort", seed=1, max_samples=256, batch_size=128, tolerance=0.0, precision="float32")
    after = ls_spa(*d, method="subsets")
    fresh_engine = HipEngine(0)
    try:
        fresh = ls_spa(*d, method="subsets", _engine=fresh_engine)
    finally:
        fresh_engine.close()
    np.testing.assert_array_equal(after.theta, fresh.theta)
    assert after.r_squared == fresh.r_squared
    np.testing.assert_array_equal(after.attribution, fresh.attribution)
    assert abs(after.attribution.sum() - after.r_squared) <= 1e-12


def test_fewer_test_rows_than_features(golden):
    g = golden("edge")                       # p = 12, M = 8: the test factor itself is kept (rect mode)
    d = _arrays(g)
    res = ls_spa(*d, method="subsets")
    np.testing.assert_allclose(res.attribution, exact_shapley(*gram_problem(*d)), **ORACLE_TOL)
    assert abs(res.attribution.sum() - res.r_squared) < 1e-12


def test_float32_inputs():
    d = [a.astype(np.float32) for a in data(11, seed=9)]
    res = ls_spa(*d, method="subsets", precision="float32")
    np.testing.assert_allclose(res.attribution, exact_shapley(*gram_problem(*d)), **ORACLE_TOL)


def test_subset_values_on_a_correlated_workload(engine):
    p = 20
    Xa, Xe, ya, ye, _, _ = workloads.correlated(np.random.default_rng(4), p, 400, 200)
    engine.load_data(Xa, Xe, ya, ye, 0.0)
    rng = np.random.default_rng(5)
    full = (1 << p) - 1
    small = [0] + [1 << i for i in range(p)] + [(1 << i) | (1 << j) for i in range(p) for j in range(i + 1, p)]
    masks = np.array(small + [full ^ m for m in small] + list(rng.integers(0, 1 << p, 4096)), dtype=np.uint64)
    assert mask_bits(masks, p).sum(axis=1).max() == p
    got = engine.debug_subset_values(masks)
    want = subset_values(*gram_problem(Xa, Xe, ya, ye), masks)
    np.testing.assert_allclose(got, want, **ORACLE_TOL)
    assert got[0] == 0.0


def test_efficiency_p24_and_determinism(engine):
    d = data(24, n=300, m=200, seed=24)
    engine.load_data(*d, 0.0)
    _, r2, _ = engine.full_fit()
    phi, info = engine.subsets_shapley()
    again, _ = engine.subsets_shapley()
    assert info == 0
    assert abs(phi.sum() - r2) <= 1e-12
    np.testing.assert_array_equal(phi, again)
    _, longest, launches = engine.subsets_timing()
    assert launches >= 1 and 0 < longest < 0.2


def test_kept_engine_sampling_unchanged_by_a_subsets_call():
    d = data(12, n=200, m=100, seed=12)
    kw = dict(method="argsort", seed=7, max_samples=512, batch_size=128, tolerance=0.0)
    before = ls_spa(*d, **kw)
    ls_spa(*d, method="subsets")
    after = ls_spa(*d, **kw)
    np.testing.assert_array_equal(before.attribution, after.attribution)
    np.testing.assert_array_equal(before.error_history, after.error_history)
    np.testing.assert_array_equal(before.attribution_errors, after.attribution_errors)


def test_engine_state_untouched(engine):
    """The running statistics of a sampling batch survive a subsets call on the same context."""
    d = data(14, n=200, m=100, seed=14)
    engine.load_data(*d, 0.0)
    engine.full_fit()
    perms = np.array([np.random.default_rng(s).permutation(14) for s in range(32)], dtype=np.int32)
    engine.reset_stats()
    engine.run_batch(perms[:16], False, accumulate=2)
    n0, m0, c0 = engine.stats()
    engine.subsets_shapley()
    n1, m1, c1 = engine.stats()
    assert n0 == n1 and np.array_equal(m0, m1) and np.array_equal(c0, c1)
    engine.run_batch(perms[16:], False, accumulate=2)
    with_sub = engine.stats()
    engine.reset_stats()
    engine.run_batch(perms[:16], False, accumulate=2)
    engine.run_batch(perms[16:], False, accumulate=2)
    without = engine.stats()
    assert with_sub[0] == without[0]
    np.testing.assert_array_equal(with_sub[1], without[1])
    np.testing.assert_array_equal(with_sub[2], without[2])


def test_sampling_estimator_error_bound_against_the_truth():
    """The first check of the estimator's error bound at a size where sampling is used: at p = 20 the exact
    attribution is known, so the argsort estimate's actual error must stay inside twice its reported overall error."""
    p = 20
    Xa, Xe, ya, ye, _, _ = workloads.correlated(np.random.default_rng(20), p, 400, 200)
    truth = ls_spa(Xa, Xe, ya, ye, method="subsets")
    est = ls_spa(Xa, Xe, ya, ye, method="argsort", seed=3, max_samples=2 ** 14, batch_size=2 ** 10, tolerance=0.0)
    err = float(np.linalg.norm(est.attribution - truth.attribution))
    assert 0.0 < est.overall_error
    assert err <= 2.0 * est.overall_error, (err, est.overall_error)


def test_p28_in_one_call(engine):
    d = data(28, n=400, m=200, seed=28)
    engine.load_data(*d, 0.0)
    _, r2, _ = engine.full_fit()
    t = time.perf_counter()
    phi, info = engine.subsets_shapley()
    t = time.perf_counter() - t
    kernel, longest, launches = engine.subsets_timing()
    print(f"p = 28: call {t:.3f} s, kernels {kernel:.3f} s in {launches} launches (longest {longest * 1e3:.1f} ms)")
    assert info == 0 and abs(phi.sum() - r2) <= 1e-12


def test_p33_refused_by_the_library(engine):
    d = data(33, n=80, m=60, seed=33)
    engine.load_data(*d, 0.0)
    with pytest.raises(ValueError, match="at most p = 32"):
        engine.subsets_shapley()
