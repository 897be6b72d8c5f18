"""ls_spa_multi_sampled(groups=) on the MI355X (the GROUPED instantiation of csrc/k_small_multi.hip,
lsspa_multi_lift_set_players of include/lsspa.h).

The contract is bitwise: a group lift has exactly the bits of the fold -- sequential fp64 adds over the group's columns in
ascending column order from 0.0, then 0.5 (a + b) for an antithetical pair -- of the column lifts that the call WITHOUT a
map returns, antithetical = 0, for the same expanded rows.  Beside it: the long-double truth of tests/hp_ref.py under the
rule of tests/test_gpu_multi_sampled.py (tol = max(1e-10, 8 e_plain), NOT_PD excused only near the threshold), all group
orderings against the exact ls_spa_multi(groups=), independence of the other responses and of the cut, the running
statistics, the state, and the public call against ls_spa_groups per response."""
import functools
import warnings

import numpy as np
import pytest

import hp_ref
from ls_spa import (SampledMultiGroupResults, SampledMultiResults, ls_spa_groups, ls_spa_multi, ls_spa_multi_sampled)
from ls_spa import _native as N
from ls_spa._native import LSSPANativeError
from test_gpu_multi_sampled import MG, T0, case, first, judge
from test_multi_host import with_responses

pytestmark = pytest.mark.gpu

EPS = 2.220446049250313e-16


# ---- label layouts ---------------------------------------------------------------------------------------------------
def layout(name, p):
    if name == "A":                      # g = p, no baseline: a fixed non-identity relabelling
        lab = (np.arange(p) + 3) % p
        lab[[0, 1]] = lab[[1, 0]]
    elif name == "B":                    # one group, no baseline
        lab = np.zeros(p)
    elif name == "C":                    # g = 4: baseline = first and last column, group 0 one column, 1 .. 3 interleaved
        lab = 1 + np.arange(p) % 3
        lab[[0, p - 1]] = -1
        lab[1] = 0
    elif name == "D":                    # one group of one column, everything else baseline
        lab = np.full(p, -1)
        lab[p // 2] = 0
    lab = np.ascontiguousarray(lab, dtype=np.int32)
    lab.setflags(write=False)
    return lab, int(lab.max()) + 1


def expand_group_row(labels, gperm, reverse):
    """host_perms.cpp's: the baseline's columns ascending, then each group's ascending, the groups in the order of gperm
    -- reversed for the second row of a pair."""
    order = list(gperm)[::-1] if reverse else list(gperm)
    return np.concatenate([np.nonzero(labels == -1)[0]] + [np.nonzero(labels == k)[0] for k in order]).astype(np.int32)


def expanded(labels, gorders, anti):
    """[B (x 2)][p]: rows 2 s and 2 s + 1 are sample s's with anti."""
    return np.array([expand_group_row(labels, gp, rev) for gp in gorders for rev in ((0, 1) if anti else (0,))],
                    dtype=np.int32)


def group_orderings(g, seed, count=1):
    rng = np.random.default_rng(seed)
    return np.array([np.arange(g), np.arange(g)[::-1]] + [rng.permutation(g) for _ in range(count)], dtype=np.int32)


def fold(col, labels, g, anti, dtype=np.float64):
    """[rows][..][p] column lifts -> [samples][..][g]: per group sequential adds in ascending column order from 0.0, then
    0.5 (a + b) over a pair's two rows."""
    col = np.asarray(col, dtype=dtype)
    out = np.zeros(col.shape[:-1] + (g,), dtype=dtype)
    for k in range(g):
        acc = np.zeros(col.shape[:-1], dtype=dtype)
        for c in np.nonzero(labels == k)[0]:
            acc = acc + col[..., c]
        out[..., k] = acc
    return dtype(0.5) * (out[0::2] + out[1::2]) if anti else out


def grouped_lifts(engine, labels, gorders, anti):
    engine.multi_lift_set_players(labels)
    return engine.multi_lift_batch(gorders, anti, want_lifts=True, accumulate=False)


def column_fold(engine, labels, g, gorders, anti):
    """The fold of what the engine WITHOUT a map gives for the expanded rows (and those column lifts)."""
    engine.multi_lift_clear_players()
    col = engine.multi_lift_batch(expanded(labels, gorders, anti), False, want_lifts=True, accumulate=False)
    return fold(col, labels, g, anti), col


# ---- 1. bitwise against the fold of the column lifts ------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "C", "D"])
@pytest.mark.parametrize("m", [1, 9, 11])
@pytest.mark.parametrize("p", [9, 24, 104])
def test_group_lifts_are_the_fold_of_the_column_lifts_bitwise(engine, p, m, name):
    d, _, _ = case(p, 1e1)
    labels, g = layout(name, p)
    gorders = group_orderings(g, 100 + p)
    try:
        engine.multi_lift_load(*first(d, m), 0.0)
        for anti in (False, True):
            want, col = column_fold(engine, labels, g, gorders, anti)
            got = grouped_lifts(engine, labels, gorders, anti)
            assert got.shape == (len(gorders), m, g)
            assert np.all(np.isfinite(got))
            np.testing.assert_array_equal(got, want)
            if name == "A" and not anti:          # every group one column: the column lifts, relabelled
                np.testing.assert_array_equal(got[:, :, labels], col)
        assert engine.multi_lift_info() == 0
    finally:
        engine.multi_lift_free()


# ---- 2. against the long-double truth ---------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def group_truth(p, kappa, r, anti):
    """(long-double group lifts [3][g] of layout C, e_plain, true smallest pivot / threshold) of response r."""
    d, _, refs = case(p, kappa)
    labels, g = layout("C", p)
    rows = expanded(labels, group_orderings(g, 100 + p), anti)
    want = fold(refs[r].lifts(rows, False, raw=True), labels, g, anti, dtype=np.longdouble)
    plain = fold(hp_ref.plain_lifts(d[0], d[1], d[2][:, r], d[3][:, r], 0.0, rows, False), labels, g, anti,
                 dtype=np.longdouble)
    e_plain = float(np.nanmax(np.abs(plain - want)))
    want = want.astype(np.float64)
    want.setflags(write=False)
    return (want, (e_plain if np.isfinite(e_plain) else 0.0),
            min(refs[r].min_pivot, refs[r].min_pivot_test) / (16 * p * EPS))


@pytest.mark.parametrize("kappa", [1e1, 1e4])
@pytest.mark.parametrize("p", [9, 24, 100])
def test_group_lifts_against_the_long_double_truth(engine, p, kappa):
    m = 9
    d, _, _ = case(p, kappa)
    labels, g = layout("C", p)
    gorders = group_orderings(g, 100 + p)
    try:
        engine.multi_lift_load(*first(d, m), 0.0)
        for anti in (False, True):
            engine.multi_lift_reset()
            got = grouped_lifts(engine, labels, gorders, anti)
            info = engine.multi_lift_info()
            for r in range(m):
                want, e_plain, ratio = group_truth(p, kappa, r, anti)
                judge(f"groups p={p} kappa={kappa:g} anti={int(anti)} r={r}", got[:, r], want, e_plain, info & 1, ratio)
            assert info & ~1 == 0
    finally:
        engine.multi_lift_free()


# ---- 3. all orderings give the exact value ----------------------------------------------------------------------------
def test_all_group_orderings_give_the_exact_attribution():
    from itertools import permutations
    p, m, kappa = 24, 9, 1e1
    d, _, refs = case(p, kappa)
    labels, g = layout("C", p)
    data = first(d, m)
    res = ls_spa_multi_sampled(*data, groups=labels, method="exact", antithetical=False)
    exact = ls_spa_multi(*data, groups=labels)
    assert isinstance(res, SampledMultiGroupResults) and res.n_samples == 24 and res.attribution.shape == (m, g)
    rows = expanded(labels, np.array(list(permutations(range(g)))), False)
    for r in range(m):
        want = fold(refs[r].lifts(rows, False, raw=True), labels, g, False, dtype=np.longdouble)
        plain = fold(hp_ref.plain_lifts(d[0], d[1], d[2][:, r], d[3][:, r], 0.0, rows, False), labels, g, False,
                     dtype=np.longdouble)
        e_plain = float(np.nanmax(np.abs(plain - want)))
        ratio = min(refs[r].min_pivot, refs[r].min_pivot_test) / (16 * p * EPS)
        judge(f"groups exact r={r}", res.attribution[r], exact.attribution[r], e_plain, 0, ratio)
        judge(f"groups exact r={r} (truth)", res.attribution[r], want.mean(axis=0).astype(np.float64), e_plain, 0, ratio)
    np.testing.assert_allclose(res.baseline_r_squared, exact.baseline_r_squared, rtol=0, atol=1e-11)
    np.testing.assert_allclose(res.r_squared, exact.r_squared, rtol=0, atol=1e-11)


# ---- 4. independence and cutting, bitwise -----------------------------------------------------------------------------
P_BIT, KAPPA_BIT = 9, 1e1


@pytest.fixture(scope="module")
def bits(engine):
    d, _, _ = case(P_BIT, KAPPA_BIT)
    labels, g = layout("C", P_BIT)
    rng = np.random.default_rng(99)
    gorders = np.array([rng.permutation(g) for _ in range(6)], dtype=np.int32)
    out = {}
    engine.multi_lift_load(*d, 0.0)
    for anti in (False, True):
        out[anti] = grouped_lifts(engine, labels, gorders, anti)
    engine.multi_lift_free()
    return d, labels, g, gorders, out


@pytest.mark.parametrize("anti", [False, True])
def test_two_calls_agree(engine, bits, anti):
    d, labels, g, gorders, out = bits
    engine.multi_lift_load(*d, 0.0)
    got = grouped_lifts(engine, labels, gorders, anti)
    engine.multi_lift_free()
    np.testing.assert_array_equal(got, out[anti])


@pytest.mark.parametrize("anti", [False, True])
def test_a_response_alone_has_the_bits_it_has_among_eleven(engine, bits, anti):
    d, labels, g, gorders, out = bits
    r = 2
    cols = [0, 1, r]                                             # the same slot, other (fewer) neighbours
    engine.multi_lift_load(d[0], d[1], d[2][:, cols], d[3][:, cols], 0.0)
    got = grouped_lifts(engine, labels, gorders, anti)
    rng = np.random.default_rng(5)
    Ya, Ye = rng.standard_normal(d[2].shape) * 3.0, rng.standard_normal(d[3].shape) * 3.0
    Ya[:, r], Ye[:, r] = d[2][:, r], d[3][:, r]
    engine.multi_lift_load(d[0], d[1], Ya, Ye, 0.0)
    other = grouped_lifts(engine, labels, gorders, anti)
    engine.multi_lift_free()
    np.testing.assert_array_equal(got[:, 2], out[anti][:, r])
    np.testing.assert_array_equal(other[:, r], out[anti][:, r])
    assert np.abs(other[:, r + 1] - out[anti][:, r + 1]).max() > 1e-6


@pytest.mark.parametrize("anti", [False, True])
def test_a_batch_cut_in_two_and_a_sample_inside_another_batch(engine, bits, anti):
    d, labels, g, gorders, out = bits
    engine.multi_lift_load(*d, 0.0)
    engine.multi_lift_set_players(labels)
    head = engine.multi_lift_batch(gorders[:2], anti, want_lifts=True, accumulate=False)
    tail = engine.multi_lift_batch(gorders[2:], anti, want_lifts=True, accumulate=False)
    rng = np.random.default_rng(17)
    other = np.array([rng.permutation(g) for _ in range(5)], dtype=np.int32)
    other[2] = gorders[4]
    mid = engine.multi_lift_batch(other, anti, want_lifts=True, accumulate=False)
    engine.multi_lift_free()
    np.testing.assert_array_equal(np.concatenate([head, tail]), out[anti])
    np.testing.assert_array_equal(mid[2], out[anti][4])


# ---- 5. running statistics --------------------------------------------------------------------------------------------
def test_running_statistics_against_numpy(engine):
    p, m = 24, 11
    d, _, _ = case(p, 1e1)
    labels, g = layout("C", p)
    rng = np.random.default_rng(24)
    batches = [np.array([rng.permutation(g) for _ in range(b)], dtype=np.int32) for b in (5, 7)]
    try:
        engine.multi_lift_load(*first(d, m), 0.0)
        engine.multi_lift_set_players(labels)
        n0, mean0, m20 = engine.multi_lift_get()
        assert n0 == 0 and mean0.shape == (m, g) and not mean0.any() and not m20.any()
        x = np.concatenate([engine.multi_lift_batch(b, True, want_lifts=True, accumulate=True) for b in batches])
        n, mean, m2 = engine.multi_lift_get()
        assert n == 12 and mean.shape == (m, g) and m2.shape == (m, g)
        want_mean = x.mean(axis=0)
        want_m2 = ((x - want_mean) ** 2).sum(axis=0)
        print(f"MLIFT group stats: mean {np.abs(mean - want_mean).max():.3e}, M2 rel {np.abs(m2 / want_m2 - 1).max():.3e}")
        np.testing.assert_allclose(mean, want_mean, rtol=0, atol=1e-14)
        np.testing.assert_allclose(m2, want_m2, rtol=1e-12, atol=0)
    finally:
        engine.multi_lift_free()


# ---- 6. state -----------------------------------------------------------------------------------------------------------
def test_the_map_and_the_statistics(engine):
    p, m = 9, 3
    d, orders, _ = case(p, 1e1)
    labels, g = layout("C", p)
    gorders = group_orderings(g, 1)
    try:
        engine.multi_lift_load(*first(d, m), 0.0)
        never = engine.multi_lift_batch(orders, True, want_lifts=True, accumulate=True)    # a context without a map
        assert engine.multi_lift_get()[0] == len(orders)
        engine.multi_lift_set_players(labels)
        assert engine.multi_lift_get()[0] == 0                                             # set_players resets n
        got = engine.multi_lift_batch(gorders, True, want_lifts=True, accumulate=True)
        assert got.shape == (len(gorders), m, g) and engine.multi_lift_get()[0] == len(gorders)
        bad = gorders.copy()
        bad[1, 0] = bad[1, 1]
        with pytest.raises(ValueError, match="not a permutation of 0 .. g-1"):
            engine.multi_lift_batch(bad, True)
        with pytest.raises(ValueError, match="not a permutation of 0 .. g-1"):            # column orderings, read as [.][g]
            engine._check(engine._lib.lsspa_multi_lift_batch(engine._h, N.iptr(np.ascontiguousarray(orders)), 2, 0,
                                                             None, 0))
        assert engine.multi_lift_get()[0] == len(gorders)                                  # neither ran
        engine.multi_lift_clear_players()
        assert engine.multi_lift_get()[0] == 0                                             # clearing resets as well
        np.testing.assert_array_equal(engine.multi_lift_batch(orders, True, want_lifts=True, accumulate=False), never)
        # a new load drops the map: the next batch wants [B][p] rows, and [B][g] rows are refused
        engine.multi_lift_set_players(labels)
        engine.multi_lift_load(*first(d, m), 0.0)
        np.testing.assert_array_equal(engine.multi_lift_batch(orders, True, want_lifts=True, accumulate=False), never)
        pad = np.zeros((len(gorders), p), dtype=np.int32)                                  # [B][g] rows in a big enough array
        pad.ravel()[:gorders.size] = gorders.ravel()
        with pytest.raises(ValueError, match="not a permutation of 0 .. p-1"):
            engine._check(engine._lib.lsspa_multi_lift_batch(engine._h, N.iptr(pad), len(gorders), 0, None, 0))
        # so does the Gram form
        engine.multi_lift_set_players(labels)
        engine.multi_lift_load_reduced(*engine.multi_lift_gram())
        assert engine.multi_lift_get()[1].shape == (m, p)
        np.testing.assert_array_equal(engine.multi_lift_batch(orders, True, want_lifts=True, accumulate=False), never)
    finally:
        engine.multi_lift_free()


@pytest.mark.parametrize("change, g, text", [
    (lambda lab: lab.__setitem__(3, 4), None, "every label must be -1 \\(baseline\\) or a group number"),     # a label >= g
    (lambda lab: lab.__setitem__(3, -2), None, "every label must be -1 \\(baseline\\) or a group number"),    # a label < -1
    (lambda lab: lab.__setitem__(1, 1), None, "a group has no column"),                                       # group 0 unused
    (lambda lab: None, 10, "the number of groups g must be between 1 and p"),                                 # g > p
])
def test_label_errors_of_the_library(engine, change, g, text):
    p = 9
    d, _, _ = case(p, 1e1)
    labels, g0 = layout("C", p)
    labels = labels.copy()
    change(labels)
    try:
        engine.multi_lift_load(*first(d, 2), 0.0)
        with pytest.raises(ValueError, match=text):
            engine.multi_lift_set_players(labels, g=g0 if g is None else g)
        assert engine.multi_lift_get()[1].shape == (2, p)             # no map was set
    finally:
        engine.multi_lift_free()


def test_set_players_before_a_load_is_a_state_error(engine):
    engine.multi_lift_free()
    with pytest.raises(LSSPANativeError, match="comes first"):
        engine.multi_lift_set_players(layout("C", 9)[0])
    with pytest.raises(LSSPANativeError, match="comes first"):
        engine.multi_lift_clear_players()


def test_the_loaded_problem_its_players_and_the_exact_state_are_left_alone(engine):
    p = 12
    d, _, _ = case(16, 1e1)
    one = hp_ref.gen(p, 60, 40, 1e1, 12)
    own, g_own = layout("C", p)
    o1 = group_orderings(g_own, 12)
    engine.load_data(*one, 0.0)
    engine.full_fit()
    engine.set_players(own)
    try:
        before = engine.run_batch(o1, True, want_lifts=True, accumulate=True)
        stats_before, info_before, gram_before = engine.stats(), engine.info(), engine.gram()
        small = with_responses(*hp_ref.gen(6, 40, 20, 1e1, 6), 3, 6)
        engine.multi_load(*small, 0.0)
        phi_before, _ = engine.multi_shapley()
        labels, g = layout("C", 16)
        try:
            engine.multi_lift_load(*first(d, 9), 0.0)
            got = grouped_lifts(engine, labels, group_orderings(g, 3), True)
            engine.multi_lift_batch(group_orderings(g, 3), True, accumulate=True)
            assert engine.multi_lift_info() == 0 and got.shape == (3, 9, g)
        finally:
            engine.multi_lift_free()
        assert engine.players == g_own and engine.info() == info_before
        for a, b in zip(engine.stats(), stats_before):
            np.testing.assert_array_equal(a, b)
        for a, b in zip(engine.gram(), gram_before):
            np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(engine.run_batch(o1, True, want_lifts=True, accumulate=False), before)
        phi_after, _ = engine.multi_shapley()
        engine.multi_free()
        np.testing.assert_array_equal(phi_after, phi_before)
    finally:
        engine.clear_players()


# ---- 7. the public call -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("anti", [False, True])
def test_public_call_against_ls_spa_groups_per_response(anti):
    p, m, kappa, g = 40, 9, 1e1, 10
    d, _, refs = case(p, kappa)
    labels = np.concatenate([[-1, -1, -1], np.arange(p - 3) % g]).astype(np.int32)      # a 3-column baseline
    rng = np.random.default_rng(40)
    gorders = np.array([rng.permutation(g) for _ in range(32)], dtype=np.int32)
    data = first(d, m)
    res = ls_spa_multi_sampled(*data, groups=labels, perms=gorders, antithetical=anti)
    assert isinstance(res, SampledMultiGroupResults)
    assert res.n_samples == 32 and res.attribution.shape == (m, g) and res.attribution_errors.shape == (m, g)
    np.testing.assert_allclose(res.attribution.sum(axis=1), res.r_squared - res.baseline_r_squared, rtol=0, atol=1e-9)
    rows = expanded(labels, gorders, anti)
    for r in range(m):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            one = ls_spa_groups(d[0], d[1], d[2][:, r], d[3][:, r], labels, perms=gorders, antithetical=anti,
                                tolerance=0.0)
        want = fold(refs[r].lifts(rows, False, raw=True), labels, g, anti, dtype=np.longdouble)
        plain = fold(hp_ref.plain_lifts(d[0], d[1], d[2][:, r], d[3][:, r], 0.0, rows, False), labels, g, anti,
                     dtype=np.longdouble)
        tol = max(T0, MG * float(np.nanmax(np.abs(plain - want))))
        print(f"MLIFT groups public anti={int(anti)} r={r}: |multi - ls_spa_groups| "
              f"{np.abs(res.attribution[r] - one.attribution).max():.3e} tol {tol:.3e}")
        assert np.abs(res.attribution[r] - one.attribution).max() <= tol
        assert np.abs(res.attribution[r] - want.mean(axis=0).astype(np.float64)).max() <= tol
        assert abs(res.r_squared[r] - one.r_squared) <= 1e-10
        np.testing.assert_allclose(res.theta[r], one.theta, rtol=1e-9, atol=1e-12)


def test_groups_none_is_the_column_call_bit_for_bit():
    p, m = 24, 9
    d, orders, _ = case(p, 1e1)
    a = ls_spa_multi_sampled(*first(d, m), perms=orders)
    b = ls_spa_multi_sampled(*first(d, m), perms=orders, groups=None)
    assert isinstance(b, SampledMultiResults) and b.attribution.shape == (m, p)
    for name in ("attribution", "attribution_errors", "theta", "r_squared"):
        np.testing.assert_array_equal(getattr(a, name), getattr(b, name))


def test_one_group_gets_the_whole_r_squared():
    p, m = 24, 9
    d, _, _ = case(p, 1e1)
    labels, g = layout("B", p)
    res = ls_spa_multi_sampled(*first(d, m), groups=labels, max_samples=4, batch_size=4)
    assert g == 1 and res.attribution.shape == (m, 1) and not res.baseline_r_squared.any()
    np.testing.assert_allclose(res.attribution[:, 0], res.r_squared, rtol=0, atol=1e-9)
