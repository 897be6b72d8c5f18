"""The exact enumerations at the top of their ranges on the MI355X -- p = 29 .. 32 features, g = 24 and 28 groups over
p <= 64 columns, 22 players of an Owen game, subset values at p = 32 and g = 32 -- against a per-player truth.

Above p = 20 / g = 20 no CPU can enumerate the game, so the data are SEPARABLE (tests/separable_ref.py): every block of
columns has rows of its own, the game is a sum of block games of at most 10 players, and phi, the interaction index and
the Owen value of every player are known in long double from 2^10 solves at most.  tests/test_separable_host.py pins
that truth to the fp64 oracles of whole problems and proves that the cases below reach the last pair slot of the
interactions kernel, the last entry slot of the sweep matrix, 8192 units x 8192 high subsets and the grouped layouts
their comments name.  Every result is held to ORACLE_TOL, the tolerance of the project's enumeration tests on
well-conditioned data, and every call must return info == 0.  The subset values at the top use correlated data and the
rule of tests/test_gpu_accuracy.py instead."""
import time
import warnings
from functools import lru_cache

import numpy as np
import pytest

import hp_ref
import separable_ref as SR
from ls_spa import ls_spa, ls_spa_interactions, ls_spa_multi, ls_spa_owen
from owen_ref import BIG_CASE
from test_gpu_accuracy import judge, shape, threshold, values_case
from test_groups_host import group_values
from test_interactions_host import shap_matrix
from test_multi_groups_host import multi_group_values
from test_multi_host import multi_gram_problem, multi_subset_values
from test_subsets_host import subset_values

pytestmark = pytest.mark.gpu

ORACLE_TOL = dict(rtol=0, atol=1e-11)      # that of tests/test_gpu_subsets.py
WORST = {}                                 # entry point -> worst |got - truth|, for DESIGN.md (Numerics)
phi_case = lru_cache(maxsize=None)(SR.phi_case)
inter_case = lru_cache(maxsize=None)(SR.inter_case)
group_case = lru_cache(maxsize=None)(SR.group_case)


def held(entry, case, got, want):
    """|got - truth| <= 1e-11 for every entry; the worst of the entry point is kept for the report."""
    err = float(np.abs(np.asarray(got) - want).max())
    WORST[entry] = max(WORST.get(entry, 0.0), err)
    print(f"SEPTOP {entry} {case}: max |got - truth| = {err:.3e}")
    np.testing.assert_allclose(got, want, **ORACLE_TOL)


def public(fn, *a, **kw):
    """A public call whose NOT_PD warning (info != 0) is an error."""
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        return fn(*a, **kw)


# ---- phi, one response -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", sorted(SR.PHI_SIZES))
def test_phi_of_every_feature(engine, p):
    sep = phi_case(p)
    engine.load_data(*sep.data(), 0.0)
    _, r2, _ = engine.full_fit()
    phi, info = engine.subsets_shapley()
    assert info == 0
    held("subsets_shapley", f"p={p}", phi, sep.phi())
    assert abs(phi.sum() - sep.total()) <= 1e-11 and abs(phi.sum() - r2) <= 1e-12
    if p == 32:
        assert engine.subsets_timing()[2] == 64
    assert np.abs(sep.phi()).min() > 1e-7 and np.abs(sep.phi()).max() > 1e-3


@pytest.mark.parametrize("p", sorted(SR.PHI_SIZES))
def test_phi_of_every_feature_through_ls_spa(engine, p):
    sep = phi_case(p)
    res = public(ls_spa, *sep.data(), method="subsets", _engine=engine)
    held("ls_spa(method='subsets')", f"p={p}", res.attribution, sep.phi())
    assert abs(res.attribution.sum() - sep.total()) <= 1e-11 and abs(res.attribution.sum() - res.r_squared) <= 1e-12


# ---- interactions ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", sorted(SR.INTER_FIXED))
def test_interactions_of_every_pair(engine, p):
    """Every slot of the high-high pairs holds within-block pairs (the block's own index) and cross-block pairs (0)."""
    sep = inter_case(p)
    engine.load_data(*sep.data(), 0.0)
    phi, raw, info = engine.subsets_interactions()
    assert info == 0
    held("subsets_interactions", f"p={p} raw index", raw, sep.interactions())
    held("subsets_interactions", f"p={p} phi", phi, sep.phi())
    np.testing.assert_array_equal(raw, raw.T)
    np.testing.assert_array_equal(np.diag(raw), np.zeros(p))


@pytest.mark.parametrize("p", sorted(SR.INTER_FIXED))
def test_interactions_of_every_pair_through_ls_spa_interactions(engine, p):
    sep = inter_case(p)
    res = public(ls_spa_interactions, *sep.data(), _engine=engine)
    held("ls_spa_interactions", f"p={p} matrix", res.interactions, shap_matrix(sep.interactions(), sep.phi()))
    held("ls_spa_interactions", f"p={p} phi", res.attribution, sep.phi())


# ---- many responses ----------------------------------------------------------------------------------------------------
@pytest.mark.slow                          # m + 1 enumerations: 9.7 s at p = 30, 14.9 s at p = 32 on the MI355X
@pytest.mark.parametrize("p", sorted(SR.MULTI_RESPONSES))
def test_multi_every_row_and_bitwise_alone(engine, p):
    """p = 30, m = 9: two chunks, the second holding one response; p = 32, m = 3.  Every row against its own response's
    truth, and bit-equal to the same response enumerated alone: a response's bits depend neither on its slot in a chunk
    of eight nor on the responses beside it, also where a unit accumulates thousands of subsets in registers."""
    m = SR.MULTI_RESPONSES[p]
    sep = phi_case(p, m)
    engine.multi_load(*sep.multi_data(), 0.0)
    try:
        phi, info = engine.multi_shapley()
        assert info == 0 and phi.shape == (m, p)
        held("multi_shapley", f"p={p} m={m}", phi, np.array([sep.phi(r) for r in range(m)]))
        for r in range(m):
            alone, info_r = engine.multi_shapley(first=r, count=1)
            assert info_r == 0
            np.testing.assert_array_equal(alone[0], phi[r])
    finally:
        engine.multi_free()
    assert np.abs(sep.phi(0) - sep.phi(m - 1)).max() > 1e-3


@pytest.mark.parametrize("p", sorted(SR.MULTI_RESPONSES))
def test_multi_through_ls_spa_multi(engine, p):
    m = SR.MULTI_RESPONSES[p]
    sep = phi_case(p, m)
    res = public(ls_spa_multi, *sep.multi_data(), _engine=engine)
    held("ls_spa_multi", f"p={p} m={m}", res.attribution, np.array([sep.phi(r) for r in range(m)]))


# ---- groups ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["g24_p64", "g28_p56"])
def test_phi_of_every_group(engine, name):
    sep, labels = group_case(name)
    engine.load_data(*sep.data(), 0.0)
    _, r2, _ = engine.full_fit()
    phi, info = engine.groups_shapley(labels)
    assert info == 0 and engine.groups_timing()[2] > 1
    held("groups_shapley", name, phi, sep.group_phi(labels))
    base = engine.debug_group_values(labels, np.zeros(1, dtype=np.uint64))[0]          # R^2 of the baseline alone
    assert ((labels == -1).sum() == 0) == (base == 0.0)
    assert abs(phi.sum() - (r2 - base)) <= 1e-12 and abs(phi.sum() - sep.group_gain(labels)) <= 1e-11
    assert np.abs(sep.group_phi(labels)).max() > 1e-3


@pytest.mark.parametrize("name", ["g24_p64", "g28_p56"])
def test_phi_of_every_group_through_ls_spa(engine, name):
    sep, labels = group_case(name)
    res = public(ls_spa, *sep.data(), method="subsets", groups=labels, _engine=engine)
    held("ls_spa(groups=)", name, res.attribution, sep.group_phi(labels))


def test_multi_groups_every_row_and_bitwise_alone(engine):
    """g = 24, p = 48, m = 9 (256 high subsets a unit): every row against its own response's truth, and bit-equal to the
    same response enumerated alone, whichever slot of its wave it stands in."""
    name, m = "g24_p48", SR.MULTI_GROUP_RESPONSES
    sep, labels = group_case(name, m)
    engine.multi_load(*sep.multi_data(), 0.0)
    try:
        phi, info = engine.multi_groups_shapley(labels)
        assert info == 0 and phi.shape == (m, 24)
        held("multi_groups_shapley", f"{name} m={m}", phi, np.array([sep.group_phi(labels, r) for r in range(m)]))
        for r in range(m):
            alone, info_r = engine.multi_groups_shapley(labels, first=r, count=1)
            assert info_r == 0
            np.testing.assert_array_equal(alone[0], phi[r])
    finally:
        engine.multi_free()


# ---- Owen --------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def owen_case():
    return SR.owen_case(BIG_CASE, 14)


def test_owen_values_of_the_22_player_game(engine):
    """The layout of tests/test_gpu_owen.py's p = 64 case: the group of 8 and two groups of 4 are one block (a refined game
    of 10 players in long double); one group of 4 of another block the same way."""
    sep, parts = owen_case()
    other = parts[1][0]
    engine.load_data(*sep.data(), 0.0)
    owen, phi, info = engine.groups_owen(BIG_CASE)
    assert info == 0
    for k in (14, other):
        held("groups_owen", f"group {k}", owen[BIG_CASE == k], sep.owen(BIG_CASE, k))
    held("groups_owen", "group phi", phi, sep.group_phi(BIG_CASE))
    assert np.abs(sep.owen(BIG_CASE, 14)).max() > 1e-3


def test_owen_values_through_ls_spa_owen(engine):
    sep, parts = owen_case()
    res = public(ls_spa_owen, *sep.data(), BIG_CASE, _engine=engine)
    for k in (14, parts[1][0]):
        held("ls_spa_owen", f"group {k}", res.attribution[BIG_CASE == k], sep.owen(BIG_CASE, k))


# ---- subset values at the top: correlated data, the rule of tests/test_gpu_accuracy.py --------------------------------------
KAPPA = 10.0


def timed(fn):
    """fn with its host seconds added to the report's."""
    def run(*a):
        t0 = time.perf_counter()
        try:
            return fn(*a)
        finally:
            SR.HOST_SECONDS["truth"] += time.perf_counter() - t0
    return run


def ld_values(ref, masks):
    return np.array([float(ref.mask_value(m)) for m in masks])


def test_subset_values_p32():
    """The sweep matrix of every size up to 33 rows (entry slot 17), bit 31, all 26 high pivots."""
    masks = SR.top_masks(32, 256, seed=32)
    values_case("subset_values", 32, KAPPA, lambda eng: (eng.debug_subset_values(masks), 0),
                timed(lambda ref: ld_values(ref, masks)), lambda prob: subset_values(*prob, masks))


def test_group_values_g32_p64():
    """Masks with the groups 28 .. 31 and the 65-row matrix of all 64 columns."""
    labels, masks = SR.G32_LABELS, SR.g32_masks(128, seed=32)
    values_case("group_values", 64, KAPPA, lambda eng: (eng.debug_group_values(labels, masks), 0),
                timed(lambda ref: np.array([float(ref.group_value(m, labels)) for m in masks])),
                lambda prob: group_values(*prob, labels, masks))


def multi_values_case(name, p, m, call, want_of, plain_of):
    """values_case for m responses: response 0 is hp_ref.gen's, the others further seeded linear models on the same X."""
    Xa, Xe, ya, ye = hp_ref.gen(p, *shape(p), KAPPA, 7100 + p)
    rng = np.random.default_rng(p + m)
    W = rng.standard_normal((p, m - 1))
    Ya = np.column_stack([ya, Xa @ W + rng.standard_normal((len(ya), m - 1))])
    Ye = np.column_stack([ye, Xe @ W + rng.standard_normal((len(ye), m - 1))])
    t0 = time.perf_counter()
    refs = [hp_ref.Problem(Xa, Xe, Ya[:, r], Ye[:, r]) for r in range(m)]
    want = np.column_stack([want_of(ref) for ref in refs])
    SR.HOST_SECONDS["truth"] += time.perf_counter() - t0
    e_plain = float(np.abs(plain_of(multi_gram_problem(Xa, Xe, Ya, Ye)) - want).max())
    from ls_spa._engine import HipEngine
    eng = HipEngine(0)
    try:
        eng.multi_load(Xa, Xe, Ya, Ye, 0.0)
        got = call(eng)
        eng.multi_free()
    finally:
        eng.close()
    assert got.shape == want.shape
    judge(f"{name} p={p} m={m} kappa={KAPPA:g}", got, want, e_plain, 0, min(r.min_pivot for r in refs) / threshold(p))


def test_multi_values_p32_m9():
    masks = SR.top_masks(32, 16, seed=33)
    multi_values_case("multi_values", 32, 9, lambda eng: eng.multi_values(masks), lambda ref: ld_values(ref, masks),
                      lambda prob: multi_subset_values(*prob, masks))


def test_multi_group_values_g32_p64_m9():
    labels, masks = SR.G32_LABELS, SR.g32_masks(16, seed=33, singles=range(3, 32, 4))
    assert (1 << 32) - 1 in masks and any(int(m) >> 28 == 15 for m in masks)
    multi_values_case("multi_group_values", 64, 9, lambda eng: eng.multi_group_values(labels, masks),
                      lambda ref: np.array([float(ref.group_value(m, labels)) for m in masks]),
                      lambda prob: multi_group_values(*prob, labels, masks))


def test_report():
    """Not a check: the worst error per entry point and the host time of the long-double truths, for DESIGN.md."""
    for entry in sorted(WORST):
        print(f"SEPTOP worst {entry}: {WORST[entry]:.3e}")
    print(f"SEPTOP host seconds of the long-double truths: {SR.HOST_SECONDS['truth']:.1f}")
