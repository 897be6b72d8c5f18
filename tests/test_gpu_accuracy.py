"""How accurate the kernels are where Gaussian data do not look: under ill-conditioning, column scaling and collinearity.

Every case compares the device with tests/hp_ref.py (long double from the fp64 inputs on, validated against mpmath and
the real reference's fixtures in tests/test_hp_ref_host.py), never with fp64 code of the project's own precision.

    tol(case) = max(T0, MG * e_plain(case))

T0 is the stated tolerance (1e-10 fp64, 1e-4 fp32 work), e_plain the error of NumPy / LAPACK on the same route at the
same precision against the same truth (hp_ref.plain_lifts; the fp64 host oracles for the exact paths), and MG the
margin between two correct implementations of one c p eps kappa bound.  MG = 4 x the worst measured
r = err_kernel / max(e_plain, 4 eps) on the MI355X, rounded up to a power of two; the table is in DESIGN.md, Numerics.

A case whose pivots the engine calls non-positive (LSSPA_INFO_NOT_PD) is excused from the tolerance -- but only a case
whose TRUE smallest relative pivot is within 100 x of the engine's threshold 16 p eps may be."""
import warnings
from functools import lru_cache

import numpy as np
import pytest

import hp_ref
from ls_spa import ls_spa, ls_spa_groups
from ls_spa._engine import HipEngine, debug_expand_groups
from ls_spa._native import LSSPANativeError
from test_groups_host import group_shapley, group_values, labels_of
from test_subsets_host import data, exact_shapley, gram_problem, subset_values

pytestmark = pytest.mark.gpu

EPS = {"float64": 2.220446049250313e-16, "float32": 1.1920929e-07}
T0 = {"float64": 1e-10, "float32": 1e-4}
MG = 8            # worst measured r: 1.68 (rect p = 150, kappa_X = 1e3)
KAPPAS = [1.0, 1e2, 1e3, 1e4, 1e5, 1e6, 3e6]
KAPPAS32 = [1.0, 10.0, 100.0, 1000.0]


def threshold(p, dtype="float64"):
    return 16 * p * EPS[dtype]


def shape(p, m=None):
    return 4 * p + 50, (3 * p + 40 if m is None else m)


@lru_cache(maxsize=4)
def truth_of(p, n, m, kappa, seed):
    """(data, long-double problem, orderings): shared by the cases that differ in engine flags or precision only."""
    d = hp_ref.gen(p, n, m, kappa, seed)
    return d, hp_ref.Problem(*d), hp_ref.orderings(p, seed)


def judge(name, got, want, e_plain, not_pd, ratio, dtype="float64"):
    """The three assertions of a case; returns r = err / max(e_plain, 4 eps) (nan for an excused case)."""
    if ratio >= 100:
        assert not not_pd, f"{name}: NOT_PD with the true smallest pivot {ratio:.3g} x the threshold"
    if not_pd:
        print(f"ACC {name}: NOT_PD (true pivot / threshold = {ratio:.3g}): excused")
        return float("nan")
    assert np.all(np.isfinite(got)), f"{name}: non-finite result without NOT_PD"
    err = float(np.abs(np.asarray(got) - want).max())
    tol = max(T0[dtype], MG * e_plain)
    r = err / max(e_plain, 4 * EPS[dtype])
    print(f"ACC {name}: err {err:.3e} e_plain {e_plain:.3e} r {r:.2f} tol {tol:.3e} pivot/threshold {ratio:.3g}")
    assert err <= tol, f"{name}: |got - truth| = {err:.3e} > {tol:.3e} (e_plain {e_plain:.3e})"
    return r


def lift_sweep_case(path, p, m, kappa, dtype="float64", flags=0):
    n, m = shape(p, m)
    d, ref, orders = truth_of(p, n, m, kappa, 7000 + p)
    eng = HipEngine(0)
    try:
        eng.set_flags(flags)
        eng.set_precision(dtype)
        eng.load_data(*d, 0.0)
        assert eng.tri == (m >= p)
        eng.full_fit()                   # from here on every batch's sums are checked too
        for anti in (False, True):
            got = eng.run_batch(orders, anti, want_lifts=True, accumulate=False)
            info = eng.info()
            want = ref.lifts(orders, anti)
            e_plain = float(np.nanmax(np.abs(hp_ref.plain_lifts(*d, 0.0, orders, anti, np.dtype(dtype).type) - want)))
            ratio = min(ref.min_pivot, ref.min_pivot_test) / threshold(p, dtype)
            name = f"{path} p={p} kappa={kappa:g} {dtype} flags={flags} anti={int(anti)} info={info}"
            judge(name, got, want, e_plain if np.isfinite(e_plain) else 0.0, info & 1, ratio, dtype)
            if not info & 1:
                # ill-conditioned but positive definite: neither a hand-over timed out nor do the sums count as a fault
                assert info & 12 == 0, f"{name}: sum deviation {eng.sum_deviation():.3e}"
    finally:
        eng.close()


# ---- a. conditioning sweep, fp64 -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kappa", KAPPAS)
def test_sweep_register_fused_p40(kappa):
    lift_sweep_case("register", 40, None, kappa)


@pytest.mark.parametrize("kappa", KAPPAS)
def test_sweep_lds_fused_p120(kappa):
    lift_sweep_case("lds", 120, None, kappa)


@pytest.mark.slow
@pytest.mark.parametrize("flags", [0, 128, 512])
@pytest.mark.parametrize("kappa", KAPPAS)
def test_sweep_general_tri_p300(kappa, flags):
    lift_sweep_case("general", 300, None, kappa, flags=flags)


@pytest.mark.parametrize("kappa", KAPPAS)
def test_sweep_general_rect_p150_m100(kappa):
    lift_sweep_case("rect", 150, 100, kappa)


def masks_of(ng, n_random, seed):
    """The masks of test_subset_values_on_a_correlated_workload: the small sets, their complements, random ones."""
    full = (1 << ng) - 1
    small = [0] + [1 << i for i in range(ng)] + [(1 << i) | (1 << j) for i in range(ng) for j in range(i + 1, ng)]
    rnd = list(np.random.default_rng(seed).integers(0, 1 << ng, n_random))
    return np.array(small + [full ^ s for s in small] + rnd, dtype=np.uint64)


def values_case(name, p, kappa, call, want_of, plain_of):
    d = hp_ref.gen(p, *shape(p), kappa, 7100 + p)
    ref = hp_ref.Problem(*d)
    eng = HipEngine(0)
    try:
        eng.load_data(*d, 0.0)
        try:
            got, not_pd = call(eng)
        except LSSPANativeError as e:            # the test hooks report a failed pivot as an error
            assert "positive definite" in str(e), e
            got, not_pd = None, 1
    finally:
        eng.close()
    want = want_of(ref)
    e_plain = float(np.abs(plain_of(gram_problem(*d)) - want).max())
    judge(f"{name} p={p} kappa={kappa:g}", got, want, e_plain, not_pd, ref.min_pivot / threshold(p))


@pytest.mark.parametrize("kappa", KAPPAS)
def test_sweep_subset_values_p20(kappa):
    masks = masks_of(20, 512, 5)
    values_case("subset_values", 20, kappa, lambda eng: (eng.debug_subset_values(masks), 0),
                lambda ref: np.array([float(ref.mask_value(m)) for m in masks]),
                lambda prob: subset_values(*prob, masks))


@pytest.mark.parametrize("kappa", KAPPAS)
def test_sweep_group_values_g12_p40(kappa):
    labels = labels_of([3] * 12, 4, seed=12)
    masks = masks_of(12, 256, 6)
    values_case("group_values", 40, kappa, lambda eng: (eng.debug_group_values(labels, masks), 0),
                lambda ref: np.array([float(ref.group_value(m, labels)) for m in masks]),
                lambda prob: group_values(*prob, labels, masks))


@pytest.mark.parametrize("kappa", KAPPAS)
def test_sweep_subsets_shapley_p10(kappa):
    values_case("subsets_shapley", 10, kappa, lambda eng: eng.subsets_shapley(), lambda ref: ref.shapley(),
                lambda prob: exact_shapley(*prob))


@pytest.mark.parametrize("kappa", KAPPAS)
def test_sweep_groups_shapley_g10_p24(kappa):
    labels = labels_of([2] * 10, 4, seed=10)
    values_case("groups_shapley", 24, kappa, lambda eng: eng.groups_shapley(labels), lambda ref: ref.shapley(labels),
                lambda prob: group_shapley(*prob, labels))


# ---- b. conditioning sweep, fp32 work matrices -----------------------------------------------------------------------
@pytest.mark.slow
@pytest.mark.parametrize("kappa", KAPPAS32)
@pytest.mark.parametrize("p", [300, 257])
def test_sweep_float32_general(p, kappa):
    lift_sweep_case("general", p, None, kappa, dtype="float32")


# ---- a'. the pivots' reciprocal square root, isolated ------------------------------------------------------------------
# The sweeps above cannot see the factorisation's own round-off: forming G in fp64 costs kappa^2 before any kernel runs,
# for LAPACK and the kernels alike.  These cases take the engine's own fp64 G, g, H, h (lsspa_get_gram) as exact inputs
# and look at the first pivot of an ordering, where nothing has been accumulated yet: every quantity is a handful of
# roundings (u = eps / 2 each) away from its long-double value, so a reciprocal square root that is not faithfully
# rounded (one Newton step leaves 4e-15 = 37 u, csrc/tiles.h) shows at once.  Every feature takes the first position.
def first_orderings(p):
    return np.array([[j] + [k for k in range(p) if k != j] for j in range(p)], dtype=np.int32)


@pytest.mark.parametrize("p", [40, 120, 300], ids=["register_p40", "lds_p120", "general_p300"])
def test_first_lift_of_every_feature_to_a_few_ulp(p):
    """lift of the first feature j = (g_j / G_jj) (2 h_j - g_j H_jj / G_jj) / yy.  The engine computes it as
    z V (2 yt - z V) / yy with r = rsqrt(G_jj), rt = rsqrt(H_jj), z = g_j r, V = (H_jj rt) r, yt = h_j rt.  With r, rt
    faithful (2 u): z 3 u, H_jj rt 3 u, V 6 u, N = z V 10 u, yt 3 u, 2 yt - N <= 11 u of |2 yt| + |N|, the product
    21 u, the division 22 u -- and nothing else enters (V[0, k > 0] = 0 exactly).  Bound: 16 eps = 32 u of the terms'
    magnitudes.  One Newton step (37 u in r and rt) gives up to 4 x 37 u on top."""
    d = hp_ref.gen(p, *shape(p), 10.0, 7400 + p)
    orders = first_orderings(p)
    eng = HipEngine(0)
    try:
        eng.load_data(*d, 0.0)
        G, g, H, h = (np.asarray(a, dtype=np.longdouble) for a in eng.gram())
        yy = np.longdouble(eng.y_norm_sq)
        got = eng.run_batch(orders, False, want_lifts=True, accumulate=False)
        assert eng.info() == 0
    finally:
        eng.close()
    Gd, Hd = np.diag(G), np.diag(H)
    want = (g / Gd) * (2 * h - g * Hd / Gd) / yy
    scale = np.abs(g / Gd) * (2 * np.abs(h) + np.abs(g) * Hd / Gd) / yy
    first = np.asarray(got[np.arange(p), np.arange(p)], dtype=np.longdouble)
    rel = np.asarray(np.abs(first - want) / scale, dtype=np.float64) / EPS["float64"]
    print(f"ACC first lift p={p}: max {rel.max():.2f} eps, mean {rel.mean():.2f} eps")
    assert rel.max() <= 16


@pytest.mark.parametrize("p", [40, 300])
def test_first_column_of_the_factor_to_a_few_ulp(p):
    """The factors the general path leaves in its work matrices (lsspa_debug_factor), first column, both matrices:
    L_00 = fl(G_00 r) and L_i0 = fl(G_i0 r) (or via the block's inverse: one more rounding each) with r faithful are
    each within 4 u of their values, so L_i0 L_00 is within 8 u = 4 eps of G_i0, and the carried row z_0 L_00 of g_0."""
    d = hp_ref.gen(p, *shape(p), 10.0, 7500 + p)
    engine = HipEngine(0)
    try:
        engine.load_data(*d, 0.0)
        G, g, H, h = (np.asarray(a, dtype=np.longdouble) for a in engine.gram())
        worst = 0.0
        for j in np.random.default_rng(p).choice(p, 24, replace=False):
            o = first_orderings(p)[j]
            L, Lt, _ = engine.debug_factor(o)
            for F, S, s in ((L, G, g), (Lt, H, h)):
                col = np.asarray(F[:p + 1, 0], dtype=np.longdouble)
                ref = np.concatenate([S[o, j], [s[j]]])
                rel = np.abs(col * col[0] - ref) / (np.abs(col) * col[0])
                worst = max(worst, float(rel.max()) / EPS["float64"])
        assert engine.info() == 0
    finally:
        engine.close()
    print(f"ACC first column p={p}: max {worst:.2f} eps")
    assert worst <= 4


# ---- c. scaling ------------------------------------------------------------------------------------------------------
def run_lifts(d, orders, dtype):
    eng = HipEngine(0)
    try:
        eng.set_precision(dtype)
        eng.load_data(*d, 0.0)
        eng.full_fit()
        return eng.run_batch(orders, False, want_lifts=True, accumulate=False), eng.info()
    finally:
        eng.close()


@pytest.mark.parametrize("yexp", [30, -30])
@pytest.mark.parametrize("dtype, kmax", [("float64", 40), ("float32", 12)])
@pytest.mark.parametrize("p, m", [(40, None), (120, None), pytest.param(300, None, marks=pytest.mark.slow), (150, 100)])
def test_column_and_target_scaling(p, m, dtype, kmax, yexp):
    """Columns scaled by 2^k_j, y by 2^yexp (both sets alike): the lifts are those of the unscaled data, the relative
    pivot test sees the same ratios, and nothing may be reported."""
    n, m = shape(p, m)
    Xa, Xe, ya, ye = hp_ref.gen(p, n, m, 10.0, 7200 + p)
    orders = hp_ref.orderings(p, p, 1)
    c = np.ldexp(1.0, np.random.default_rng(p + kmax).integers(-kmax, kmax + 1, p))
    s = np.ldexp(1.0, yexp)
    scaled = (Xa * c, Xe * c, ya * s, ye * s)
    want = hp_ref.Problem(*scaled).lifts(orders, False)
    e_plain = float(np.abs(hp_ref.plain_lifts(*scaled, 0.0, orders, False, np.dtype(dtype).type) - want).max())
    got, info = run_lifts(scaled, orders, dtype)
    base, info0 = run_lifts((Xa, Xe, ya, ye), orders, dtype)
    name = f"scaling p={p} m={m} {dtype} y*2^{yexp}"
    judge(name, got, want, e_plain, 0, float("inf"), dtype)
    print(f"ACC {name}: max |scaled - unscaled| = {np.abs(got - base).max():.3e}, bit-equal: {np.array_equal(got, base)}")
    if dtype == "float64":
        np.testing.assert_allclose(got, base, rtol=0, atol=1e-12)
    assert info == 0 and info0 == 0, (info, info0)


@pytest.mark.parametrize("k", [70, -70])
def test_float32_columns_outside_the_float32_range(k):
    """Two columns scaled by 2^k: their G_jj = 2^(2k) leaves the fp32 range.  Right within tol, or reported."""
    p = 150
    Xa, Xe, ya, ye = hp_ref.gen(p, *shape(p), 10.0, 7300)
    orders = hp_ref.orderings(p, 3, 1)
    c = np.ones(p)
    c[[11, 140]] = np.ldexp(1.0, k)
    scaled = (Xa * c, Xe * c, ya, ye)
    want = hp_ref.Problem(*scaled).lifts(orders, False)
    with np.errstate(all="ignore"):
        e_plain = np.abs(hp_ref.plain_lifts(*scaled, 0.0, orders, False, np.float32) - want)
    e_plain = float(np.nanmax(e_plain)) if np.isfinite(e_plain).any() else 0.0
    try:
        got, info = run_lifts(scaled, orders, "float32")
    except (LSSPANativeError, ValueError) as e:
        print(f"ACC fp32 range k={k}: reported by exception: {e}")
        return
    print(f"ACC fp32 range k={k}: info = {info}")
    if info == 0:
        judge(f"fp32 range k={k}", got, want, e_plain if np.isfinite(e_plain) else 0.0, 0, float("inf"), "float32")


# ---- d. NOT_PD on every path and pivot position ----------------------------------------------------------------------
def duplicated(p, dup, src, seed, train=True):
    Xa, Xe, ya, ye = data(p, *shape(p), seed=seed)
    Xa, Xe = Xa.copy(), Xe.copy()
    if train:
        Xa[:, dup] = Xa[:, src]
    Xe[:, dup] = Xe[:, src]
    return Xa, Xe, ya, ye


def not_pd_bits(d, order, dtype="float64"):
    eng = HipEngine(0)
    try:
        eng.set_precision(dtype)
        eng.load_data(*d, 0.0)
        eng.run_batch(np.asarray(order, dtype=np.int32)[None, :], False, want_lifts=True, accumulate=False)
        return eng.info()
    finally:
        eng.close()


NOT_PD_CASES = [
    ("register_p20_last_block", 20, 19, "float64"),
    ("register_p100_last_block", 100, 99, "float64"),
    ("lds_p120_col119", 120, 119, "float64"),
    ("general_p300_first_block", 300, 40, "float64"),
    ("general_p300_second_block_of_the_diagonal_launch", 300, 70, "float64"),
    ("general_p300_panel", 300, 130, "float64"),
    ("general_p300_ragged_last_block", 300, 299, "float64"),
    ("general_p300_first_block_f32", 300, 40, "float32"),
    ("general_p300_second_block_of_the_diagonal_launch_f32", 300, 70, "float32"),
    ("general_p300_panel_f32", 300, 130, "float32"),
    ("general_p300_ragged_last_block_f32", 300, 299, "float32"),
]


@pytest.mark.parametrize("name, p, dup, dtype", NOT_PD_CASES, ids=[c[0] for c in NOT_PD_CASES])
@pytest.mark.parametrize("train", [True, False], ids=["both_sets", "test_set_only"])
def test_duplicate_column_is_flagged(name, p, dup, dtype, train):
    """An exact duplicate of column 3 at column `dup`: under the identity ordering the pivot at position `dup` is zero
    up to round-off (<= 1.3e-16 G_jj with LAPACK), in G and H or -- test_set_only -- in H alone.  Also under a seeded
    ordering, where the zero pivot falls wherever the later of the two columns does."""
    d = duplicated(p, dup, 3, seed=p + dup, train=train)
    assert not_pd_bits(d, np.arange(p), dtype) & 1
    assert not_pd_bits(d, np.random.default_rng(dup).permutation(p), dtype) & 1


def test_the_truth_sees_the_duplicate_far_under_the_threshold():
    d = duplicated(20, 19, 3, seed=39)
    ref = hp_ref.Problem(*d)
    with np.errstate(all="ignore"):
        ref.ordering_lift(np.arange(20))
    assert ref.min_pivot < 1e-3 * threshold(20) and ref.min_pivot_test < 1e-3 * threshold(20)


@pytest.mark.parametrize("src, dup", [(3, 9), (8, 10), (1, 4)])
def test_duplicate_column_in_the_exact_enumerations(engine, src, dup):
    """Each enumeration has two pivot tests: the elimination of a unit's high features / groups and the per-lane
    Cholesky of the low ones (the first 6 features; the smallest groups while their columns total <= 6).  The three
    pairs put the duplicate low-high, high-high and low-low, so each test is the only one that can see one of them."""
    d = duplicated(12, dup, src, seed=12)
    engine.load_data(*d, 0.0)
    assert engine.subsets_shapley()[1] & 1
    labels = labels_of([3, 3, 3, 3], 0)                 # groups of 3 columns: two of them low, two high
    assert labels[src] != labels[dup]
    assert engine.groups_shapley(labels)[1] & 1


@pytest.mark.parametrize("src, dup", [(6, 9), (0, 3), (3, 9)])
def test_duplicate_column_across_high_and_low_groups(engine, src, dup):
    """Groups {0,1,2} .. {9,10,11}: whichever two the host makes the low ones, the pairs cover high-high, low-low and
    (3, 9) a mixed pair."""
    d = duplicated(12, dup, src, seed=21)
    engine.load_data(*d, 0.0)
    assert engine.groups_shapley(labels_of([3, 3, 3, 3], 0))[1] & 1


def test_duplicate_column_warns_through_the_public_calls():
    d = duplicated(12, 9, 3, seed=12)
    perms = hp_ref.orderings(12, 1)
    with pytest.warns(RuntimeWarning, match="positive definite"):
        ls_spa(*d, perms=perms, batch_size=8, tolerance=0.0)
    with pytest.warns(RuntimeWarning, match="positive definite"):
        ls_spa(*d, method="subsets")


# ---- e. the public call on ill-conditioned but positive-definite data ------------------------------------------------
def quiet_call(fn, *a, **kw):
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        res = fn(*a, **kw)                       # an LSSPANativeError fails the test here
    texts = [str(w.message) for w in seen]
    print("ACC warnings:", texts)
    assert not any("engine fault" in t or "repeated" in t for t in texts), texts
    return res


@pytest.mark.parametrize("p, kappa", [(40, 1e6), (120, 3e5), pytest.param(300, 1e6, marks=pytest.mark.slow)])
def test_public_call_on_ill_conditioned_data(p, kappa):
    """kappa(G) ~ 1e12: the lifts' sums leave R^2 by more than the 1e-9 of well-conditioned data while every pivot is
    hundreds of times above the NOT_PD threshold.  That is the input's conditioning, not an engine fault: the call
    returns, does not repeat itself, and its attribution is the long-double mean of the same orderings within tol."""
    n, m = shape(p)
    d, ref, orders = truth_of(p, n, m, kappa, 7000 + p)
    res = quiet_call(ls_spa, *d, perms=orders, batch_size=len(orders), tolerance=0.0)
    want = ref.lifts(orders, True).mean(axis=0)
    e_plain = float(np.abs(hp_ref.plain_lifts(*d, 0.0, orders, True).mean(axis=0) - want).max())
    ratio = min(ref.min_pivot, ref.min_pivot_test) / threshold(p)
    assert ratio >= 100
    judge(f"ls_spa p={p} kappa={kappa:g}", res.attribution, want, e_plain, 0, ratio)
    # an ordering source that could be drawn again is where a false fault made the driver repeat the whole run
    quiet_call(ls_spa, *d, seed=3, max_samples=32, batch_size=16, tolerance=0.0)


def test_public_grouped_call_on_ill_conditioned_data():
    p, kappa = 120, 3e5
    n, m = shape(p)
    d, ref, _ = truth_of(p, n, m, kappa, 7000 + p)
    labels = labels_of([10] * 11 + [6], 4, seed=120)
    rng = np.random.default_rng(12)
    gperms = np.array([rng.permutation(12) for _ in range(4)], dtype=np.int32)
    res = quiet_call(ls_spa_groups, *d, labels, perms=gperms, batch_size=4, tolerance=0.0)
    cols = debug_expand_groups(labels, gperms, True)                     # the column orderings the kernels are given
    fold = lambda lift: np.array([lift[labels == k].sum() for k in range(12)])
    want = np.mean([fold(ref.to_float(ref.ordering_lift(o))) for o in cols], axis=0)
    plain = np.mean([fold(v) for v in hp_ref.plain_lifts(*d, 0.0, cols, False)], axis=0)
    ratio = min(ref.min_pivot, ref.min_pivot_test) / threshold(p)
    judge(f"ls_spa_groups p={p} kappa={kappa:g}", res.attribution, want, float(np.abs(plain - want).max()), 0, ratio)
