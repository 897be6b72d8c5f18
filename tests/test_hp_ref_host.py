"""tests/hp_ref.py has to earn its trust before the GPU tests lean on it (tests/test_gpu_accuracy.py): its long-double
path against mpmath at 50 digits, its algorithm against the fixtures made from the real reference and against the QR
oracle, and its values of column sets against the two host oracles of the exact paths."""
import numpy as np
import pytest

import hp_ref
import lsspa_oracle as O
from test_groups_host import group_values, labels_of
from test_subsets_host import data, gram_problem, subset_values

DATA = ("X_train", "X_test", "y_train", "y_test")


def test_long_double_is_wider_than_double():
    assert np.finfo(np.longdouble).eps < 1e-18


def _orders(p, seed, count):
    return hp_ref.orderings(p, seed, count)


@pytest.mark.parametrize("mode", ["tri", "rect"])
@pytest.mark.parametrize("kappa", [1.0, 1e3, 1e6])
@pytest.mark.parametrize("p", [8, 16, 24])
def test_long_double_against_mpmath(p, kappa, mode):
    """The long-double lifts are at least 256 times closer to the 50-digit ones than LAPACK fp64 is on the same case
    (8 of long double's 11 extra bits), or within 1e-17 where both sit at round-off."""
    d = hp_ref.gen(p, 4 * p + 50, 3 * p + 40 if mode == "tri" else p - 3, kappa, seed=1000 + p)
    orders = _orders(p, p, 1)                                 # identity, reversed, one seeded; both anti values below
    mp = hp_ref.MP(50)
    exact, ld = hp_ref.Problem(*d, ar=mp), hp_ref.Problem(*d)
    assert ld.tri == (mode == "tri")
    for anti in (False, True):
        want = exact.lifts(orders, anti, raw=True)
        got = ld.lifts(orders, anti, raw=True)
        e_ld = max(abs(float(mp.exact(a) - b)) for a, b in zip(got.ravel(), want.ravel()))
        e_plain = np.abs(hp_ref.plain_lifts(*d, 0.0, orders, anti) - mp.to_float(want)).max()
        print(f"p={p} kappa={kappa:g} {mode} anti={anti}: long double {e_ld:.2e}, plain fp64 {e_plain:.2e}")
        assert e_ld <= max(e_plain / 256, 1e-17)
    assert ld.min_pivot == pytest.approx(exact.min_pivot, rel=1e-6)


@pytest.mark.parametrize("kappa", [1.0, 1e6])
def test_long_double_values_and_shapley_against_mpmath(kappa):
    p = 6
    d = hp_ref.gen(p, 80, 60, kappa, seed=6)
    mp = hp_ref.MP(50)
    exact, ld = hp_ref.Problem(*d, ar=mp), hp_ref.Problem(*d)
    labels = np.array([0, 1, -1, 2, 1, 0])
    prob = gram_problem(*d)
    for phi_ld, phi_mp, phi_plain in [
            (ld.shapley(raw=True), exact.shapley(raw=True),
             _shapley_fp64(lambda m: subset_values(*prob, np.array([m], dtype=np.uint64))[0], p)),
            (ld.shapley(labels, raw=True), exact.shapley(labels, raw=True),
             _shapley_fp64(lambda m: group_values(*prob, labels, [m])[0], 3))]:
        e_ld = max(abs(float(mp.exact(a) - b)) for a, b in zip(phi_ld, phi_mp))
        e_plain = np.abs(phi_plain - mp.to_float(phi_mp)).max()
        print(f"kappa={kappa:g}: long double {e_ld:.2e}, plain fp64 {e_plain:.2e}")
        assert e_ld <= max(e_plain / 256, 1e-17)


def _shapley_fp64(value, ng):
    from test_groups_host import shapley_of_table
    return shapley_of_table(np.array([value(m) for m in range(1 << ng)]), ng)


# ---- against what the real reference produced ---------------------------------------------------------------------------
@pytest.mark.parametrize("tag,reg", [("r0", 0.0), ("r1", 0.1)])
def test_reference_lifts_p12(golden, tag, reg):
    g = golden("p12")
    ref = hp_ref.Problem(*(g[k] for k in DATA), reg=reg)
    np.testing.assert_allclose(ref.lifts(g["orders"], False), g[f"{tag}_lifts"], rtol=0, atol=1e-12)


def test_reference_lifts_corr_p100(golden):
    g = golden("corr_p100")
    d = O.correlated_workload(np.random.default_rng(int(g["seed"])), 100, int(g["N"]), int(g["M"]))
    ref = hp_ref.Problem(*d)
    assert float(ref.yy) == pytest.approx(float(g["y_norm_sq"]), rel=1e-14)
    np.testing.assert_allclose(ref.lifts(g["orders"][:6], False), g["lifts"][:6], rtol=0, atol=1e-12)


def test_reference_edge_fewer_test_rows_than_features(golden):
    g = golden("edge")                                         # M = 8 < p = 12: the rect form
    ref = hp_ref.Problem(*(g[k] for k in DATA))
    assert not ref.tri
    np.testing.assert_allclose(ref.lifts(g["perms"], True).mean(axis=0), g["mltp_attribution"], rtol=0, atol=1e-12)


def test_reference_exact_p8_by_brute_force_shapley(golden):
    g = golden("exact_p8")
    ref = hp_ref.Problem(*(g[k] for k in DATA))
    phi = ref.shapley()
    np.testing.assert_allclose(phi, g["attribution"], rtol=0, atol=1e-12)
    assert abs(phi.sum() - float(g["r_squared"])) < 1e-12


@pytest.mark.parametrize("p", [40, 130])
def test_against_the_qr_oracle_on_gaussian_data(p):
    d = O.gaussian_workload(p, 4 * p + 50, 3 * p + 40, seed=p)
    red = O.reduce(*d, 0.0)
    yy = float(np.linalg.norm(d[3]) ** 2)
    ref = hp_ref.Problem(*d)
    orders = _orders(p, p, 2)
    want = np.array([O.ordering_lift(*red, yy, o) for o in orders])
    np.testing.assert_allclose(ref.lifts(orders, False), want, rtol=0, atol=1e-13)
    np.testing.assert_allclose(hp_ref.plain_lifts(*d, 0.0, orders, False), want, rtol=0, atol=1e-13)


@pytest.mark.parametrize("mode", ["tri", "rect"])
@pytest.mark.parametrize("kappa", [1.0, 1e3, 1e6])
def test_efficiency(kappa, mode):
    """Every ordering's lifts telescope to the R^2 of the full model, to long double's round-off times kappa(G)."""
    p = 40
    d = hp_ref.gen(p, 4 * p + 50, 3 * p + 40 if mode == "tri" else 25, kappa, seed=77)
    ref = hp_ref.Problem(*d)
    r2 = ref.subset_value(np.arange(p))
    cond = np.linalg.cond(ref.to_float(ref.G))
    # the generator's promise, kappa(G) ~ 1.3 kappa_X^2, up to the sampling spread of Z^T Z / n at p / n = 0.19
    # (Marchenko-Pastur: its own condition number is ((1 + sqrt(0.19)) / (1 - sqrt(0.19)))^2 = 6.5)
    assert 0.3 * kappa ** 2 <= cond <= 10 * kappa ** 2
    for lift in ref.lifts(_orders(p, 5, 3), False, raw=True):
        assert abs(float(lift.sum() - r2)) <= 1e-16 * cond


def test_the_generator_gives_the_condition_number_it_is_asked_for():
    p = 30
    Xa = hp_ref.gen(p, 400, 200, 1e4, seed=3)[0]
    c = np.linalg.cond(Xa)
    assert 0.3e4 <= c <= 3e4


def test_subset_and_group_values_against_the_host_oracles():
    p = 12
    d = data(p, n=100, m=70, seed=12)
    prob = gram_problem(*d, reg=0.05)
    ref = hp_ref.Problem(*d, reg=0.05)
    masks = np.random.default_rng(1).integers(0, 1 << p, 64).astype(np.uint64)
    got = np.array([float(ref.mask_value(m)) for m in masks])
    np.testing.assert_allclose(got, subset_values(*prob, masks), rtol=0, atol=1e-13)
    labels = labels_of([2, 3, 1, 2], 4, seed=4)
    gm = np.arange(16)
    got = np.array([float(ref.group_value(m, labels)) for m in gm])
    np.testing.assert_allclose(got, group_values(*prob, labels, gm), rtol=0, atol=1e-13)
    assert float(ref.group_value(0, labels)) > 0.0               # the baseline is in every value
