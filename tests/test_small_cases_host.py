"""tests/small_cases.py has to reach what it was written for, and every truth case has to lie where the engine may not call
it non-positive-definite, before tests/test_gpu_small_edges.py leans on it -- checked on the CPU.

COVERAGE CONDITION: every nb = 1 .. 8 with each residue of p + 1 mod 16 in {15, 0, 1} that exists for it, under both forms
(register: nb <= 7 only); both parities of p under the register form; p = 1, 2, 3; both kappas everywhere; the ridge once
per form under flags = 0.  Dropping the last case of a class fails a test of this file.

SAFE RANGE: the smallest relative pivot of any G_pi or H_pi over a case's orderings and their reverses, computed in long
double, divided by the engine's threshold 16 p eps, is at least 100 for every truth case (the project's rule for "may not
be flagged", tests/test_gpu_accuracy.py).  Measured: the smallest ratio is 1.4e12 at kappa = 1 (p = 127) and 1.3e6 at
kappa = 1e4 (p = 46); no seed had to be changed.  The near copy of test d (x_dup = x_src + 4.5e-5 noise, both sets) has
its smallest pivot 3623 x the threshold at p = 111 and 3561 x at p = 127 (required: between 1e3 and 1e4); the exact copy
has a pivot of 0 (training Gram) / -1.9e-7 x the threshold (test Gram: round-off of the long-double sums) in every set
it is made in, and 1.7e12 x the threshold in the set it is not."""
import functools

import numpy as np
import pytest

import hp_ref
import small_cases as SC

EPS = 2.220446049250313e-16


@functools.lru_cache(maxsize=None)
def ratio_of(p, kappa, reg):
    ref = hp_ref.Problem(*SC.data_of(p, kappa), reg)
    return SC.pivot_ratio(ref, SC.with_reverses(SC.orderings_of(p, kappa)))


def test_names_shapes_and_forms():
    names = [c.name for c in SC.CASES]
    assert len(names) == len(set(names)) and len(names) <= 130
    for c in SC.CASES:
        assert 1 <= c.p <= SC.SMALL_P_MAX and (c.n, c.m) == (4 * c.p + 50, 3 * c.p + 40) and c.m >= c.p, c.name
        assert c.nb == (c.p + 1 + 15) // 16 and 1 <= c.nb <= 8, c.name
        assert c.flags in (0, SC.FLAG_LDS) and c.kappa in SC.KAPPAS and c.reg in (0.0, SC.RIDGE), c.name
        # the form is the library's rule: the register kernel exists for nb <= 7 and flag 16384 switches it off
        assert c.form == (SC.REG if c.flags == 0 and c.nb <= 7 else SC.LDS), c.name
    assert max(c.n for c in SC.CASES) <= 560            # p = 127: 558 rows


def test_shape_and_threshold_are_those_of_the_accuracy_tests():
    import test_gpu_accuracy as acc          # importable without a GPU; nothing of it runs here
    for p in SC.P_EDGES:
        assert SC.shape(p) == acc.shape(p)
        assert acc.threshold(p) == 16 * p * EPS


def test_every_block_count_and_residue_under_both_forms():
    for form in (SC.REG, SC.LDS):
        for kappa in SC.KAPPAS:
            seen = {(c.nb, (c.p + 1) % 16) for c in SC.CASES if c.form == form and c.kappa == kappa and c.reg == 0.0}
            for nb in range(1, 9 if form == SC.LDS else 8):
                # p + 1 = 16 nb (last row of the last block), 16 nb - 1, and 16 (nb - 1) + 1 (the row opens the block)
                assert (nb, 0) in seen and (nb, 15) in seen, (form, kappa, nb)
                assert (nb, 1) in seen or nb == 1, (form, kappa, nb)        # p = 0 does not exist
            if form == SC.REG:
                assert all(nb <= 7 for nb, _ in seen)
            else:
                # nb = 8 under flags = 0 and under flag 16384; nb < 8 only under the flag
                assert {c.flags for c in SC.CASES if c.form == form and c.nb == 8} == {0, SC.FLAG_LDS}
                assert {c.flags for c in SC.CASES if c.form == form and c.nb < 8} == {SC.FLAG_LDS}
    # p = 127: p + 1 = 128, the largest problem; p = 112: the first that leaves the registers
    assert {c.p for c in SC.CASES if c.flags == 0 and c.form == SC.LDS} == {112, 126, 127}


def test_parities_and_the_tiny_shapes():
    for nb in range(1, 8):
        par = {c.p % 2 for c in SC.CASES if c.form == SC.REG and c.nb == nb}
        assert par == {0, 1}, nb
    for p in (1, 2, 3):
        assert {(c.form, c.kappa) for c in SC.CASES if c.p == p} == {(f, k) for f in (SC.REG, SC.LDS) for k in SC.KAPPAS}
    # the clamp min(2 lane, (p - 1) & ~1): p = 1 (one column, the pair reads the padding column), 2 (one pair), 3 (the
    # last pair starts at column 2 and ends in the padding)
    assert [(p - 1) & ~1 for p in (1, 2, 3)] == [0, 0, 2]


def test_the_ridge_once_per_form():
    ridge = [c for c in SC.CASES if c.reg]
    assert {c.form for c in ridge if c.flags == 0} == {SC.REG, SC.LDS}
    assert {(c.p, c.form) for c in ridge if c.flags == 0} == {(47, SC.REG), (127, SC.LDS)}
    assert all(c.reg == 0.25 for c in ridge)


def test_orderings_and_data_depend_on_p_and_kappa_alone():
    for p in (1, 47):
        o = SC.orderings_of(p, 1.0)
        assert o.dtype == np.int32 and o.shape == (5, p)
        np.testing.assert_array_equal(o[0], np.arange(p))
        np.testing.assert_array_equal(o[1], np.arange(p)[::-1])
        assert all(sorted(r) == list(range(p)) for r in o)
    a, b = SC.data_of(47, 1e4), SC.data_of(47, 1e4)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert SC.seed_of(47, 1.0) != SC.seed_of(47, 1e4) != SC.seed_of(48, 1.0)
    full = SC.bit_orderings(63, SC.N_BIT_ORDERS)
    np.testing.assert_array_equal(SC.bit_orderings(63, 24), full[:24])
    np.testing.assert_array_equal(SC.bit_orderings(63, 24, 5), full[5:29])
    assert len({r.tobytes() for r in full}) == SC.N_BIT_ORDERS


@pytest.mark.parametrize("kappa", SC.KAPPAS)
def test_every_truth_case_is_in_the_safe_range(kappa):
    worst = (float("inf"), None)
    for c in SC.CASES:
        if c.kappa != kappa:
            continue
        r = ratio_of(c.p, c.kappa, c.reg)
        worst = min(worst, (r, c.name))
        assert r >= 100, f"{c.name}: smallest true pivot {r:.3g} x the threshold: change its seed (SC.SEED_OVERRIDE)"
    print(f"SMALL smallest pivot / threshold at kappa = {kappa:g}: {worst[0]:.3g} ({worst[1]})")
    assert SC.SEED_OVERRIDE == {} or all(k in {(c.p, c.kappa) for c in SC.CASES} for k in SC.SEED_OVERRIDE)


# ---- the duplicated and the nearly duplicated column of test d ----------------------------------------------------------
def test_dup_positions_and_orderings():
    assert SC.dup_positions(111) == [1, 15, 16, 17, 31, 32, 47, 48, 63, 64, 79, 80, 95, 96, 110]
    assert SC.dup_positions(127) == [1, 15, 16, 17, 31, 32, 47, 48, 63, 64, 79, 80, 95, 96, 111, 112, 126]
    for p, _ in SC.NOT_PD_RUNS:
        pos, orders = SC.dup_positions(p), SC.dup_orderings(p)
        assert orders.shape == (len(pos), p) and orders.dtype == np.int32
        for b, o in zip(pos, orders):
            assert sorted(o) == list(range(p)) and o[0] == SC.DUP_SRC and o[b] == SC.dup_col(p)
        # every block row of the matrix holds a failing pivot once, and so does the last position
        assert {b // 16 for b in pos} == set(range((p - 1) // 16 + 1)) and pos[-1] == p - 1
    assert {(p, SC.form_of(p, f)) for p, f in SC.NOT_PD_RUNS} == {(111, SC.REG), (127, SC.LDS), (111, SC.LDS)}


@pytest.mark.parametrize("where", SC.DUP_WHERE)
def test_the_truth_sees_the_exact_copy_far_under_the_threshold(where):
    p = 111
    ref = hp_ref.Problem(*SC.dup_data(p, where))
    with np.errstate(all="ignore"):
        ref.ordering_lift(SC.dup_orderings(p)[3])
    piv, piv_t = ref.min_pivot, ref.min_pivot_test
    thr = 16 * p * EPS
    print(f"SMALL exact copy, {where}: pivot / threshold {piv / thr:.3g} (training) {piv_t / thr:.3g} (test)")
    assert (abs(piv) < 1e-3 * thr) == (where != "test_set_only")
    assert (abs(piv_t) < 1e-3 * thr) == (where != "training_set_only")
    # ... and the set without the copy stays in the safe range
    assert where == "both_sets" or max(piv, piv_t) >= 100 * thr


@pytest.mark.parametrize("p", sorted({p for p, _ in SC.NOT_PD_RUNS}))
def test_the_near_copy_is_three_to_four_decades_above_the_threshold(p):
    ref = hp_ref.Problem(*SC.near_data(p))
    r = SC.pivot_ratio(ref, SC.with_reverses(SC.dup_orderings(p)))
    print(f"SMALL near copy p = {p}, t = {SC.NEAR_T[p]:g}: smallest pivot / threshold {r:.4g}")
    assert 1e3 <= r <= 1e4
