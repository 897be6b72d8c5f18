"""tests/pairs_truth.py vetted without a GPU: the exact (count, mean, M2) truth of the pair tables against the fp64
restatement tests/pair_ref.py on the cases tests/test_gpu_pairs.py runs, its int64 sums against overflow at the shapes of
tests/test_gpu_sampled_edges.py, its mean against the definition of the interaction index in rationals -- and the teeth
of the offset case: the one-pass formula M2 = sum x^2 - n mean^2 in fp64 misses the tolerance the kernel is held to."""
import itertools
from fractions import Fraction
from math import factorial

import numpy as np
import pytest

import pair_ref
import pairs_truth as PT

EPS = 2.0 ** -52
MG = 8              # tests/test_gpu_accuracy.py: the margin between two correct implementations


def existing_batches(d, B):
    """The data of test_pair_kernels_against_the_restatement (tests/test_gpu_pairs.py), stream for stream."""
    rng = np.random.default_rng(1000 * d + B)
    out = []
    for _ in range(2):
        perms = np.array([rng.permutation(d) for _ in range(B)], dtype=np.int32)
        out.append((rng.integers(-1024, 1025, size=(3 * B, d)).astype(np.float64), perms))
    return out


def both(d, batches, shift=0):
    ref, truth = pair_ref.PairTables(d), PT.PairTruth(d, shift=shift)
    for lifts, perms in batches:
        ref.add_batch(lifts, perms)
        truth.add_batch(lifts, perms)
    return ref, truth


# ---- 1. against the restatement on the existing cases ------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 5, 257])
@pytest.mark.parametrize("d", [2, 3, 63, 64, 65, 129])
def test_truth_equals_the_restatement_on_the_existing_cases(d, B):
    """Counts equal.  pair_ref rounds: a Welford step makes three roundings of numbers no larger than 2 max|Delta| for
    the mean and four of numbers no larger than 4 max|Delta|^2 for M2, the Chan merge a handful more; n steps a pair.
    Counted generously that is 8 n eps max|Delta| and 8 n eps max|Delta|^2 -- the bounds test_gpu_pairs.py holds the
    kernel to against pair_ref, here held by pair_ref against the exact tables."""
    ref, truth = both(d, existing_batches(d, B))
    count, mean, m2, max_delta = truth.tables()
    np.testing.assert_array_equal(count, ref.count)
    np.testing.assert_array_equal(max_delta, ref.max_abs)
    assert np.all(np.diag(count) == 0) and np.all(np.diag(mean) == 0) and np.all(np.diag(m2) == 0)
    mean_err, m2_err = np.abs(ref.mean - mean), np.abs(ref.m2 - m2)
    print(f"d = {d}, B = {B}: pair_ref against the exact truth: mean {float(mean_err.max()):.2e}, "
          f"M2 {float(m2_err.max()):.2e}")
    assert np.all(mean_err <= 8 * count * EPS * max_delta)
    assert np.all(m2_err <= 8 * count * EPS * max_delta ** 2)
    assert np.all(m2 >= 0)
    np.testing.assert_allclose(ref.phi, truth.phi.astype(np.float64), rtol=0, atol=8 * 6 * B * EPS * 1024)


def test_truth_does_not_depend_on_the_batching_or_the_shift():
    """One batch of 2 B samples, two of B, and any integer shift: the same integers, so the same bits."""
    (l0, p0), (l1, p1) = PT.integer_batches(65, 40, seed=1)
    want = PT.PairTruth(65).add_batch(l0, p0).add_batch(l1, p1).tables()
    one = PT.PairTruth(65).add_batch(np.concatenate([l0, l1]), np.concatenate([p0, p1])).tables()
    shifted = PT.PairTruth(65, shift=-777).add_batch(l1, p1).add_batch(l0, p0).tables()
    for a, b, c in zip(want, one, shifted):
        np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(a, c)
    # ... and the long-double flavour (whole path: lifts that are no integers) agrees on integers to its rounding
    ld = PT.PairTruth(65, dtype=PT.LD).add_batch(l0, p0).add_batch(l1, p1).tables()
    np.testing.assert_array_equal(ld[0], want[0])
    assert np.abs(ld[1] - want[1]).max() <= 2.0 ** -63 * 2048 * 4
    upper = PT.PairTruth(65).add_batch(l0, p0).add_batch(l1, p1).tables(symmetric=False)
    for a, b in zip(want, upper):
        np.testing.assert_array_equal(np.triu(a), b)


# ---- 2. the int64 sums at the shapes of the GPU tests ------------------------------------------------------------------
def test_int64_sums_cannot_overflow_at_the_shapes_of_the_gpu_tests():
    """N <= 2 batches * B <= 1026 hits a pair (every sample holds a pair at most once), |u| <= 2048 (lifts in
    [-1024, 1024], shift 0) or <= 8 (offset class, shift 2^30).  The largest intermediates are n S2 <= N^2 U^2 and
    |c n + S1| <= N (|c| + U)."""
    N = 2 * 513
    for U, c in ((2048, 0), (8, PT.OFFSET)):
        assert N * N * U * U < 2 ** 62 and N * (c + U) < 2 ** 62
    assert N * N * 2048 * 2048 <= 2 ** 44
    # without the shift the offset class would not fit: that is what the shift is for
    assert N * N * (PT.OFFSET + 8) ** 2 > 2 ** 63
    # the guard itself: tables() refuses data that would overflow
    t = PT.PairTruth(2)
    t.add_batch(np.array([[0.0, 2.0 ** 31], [0.0, 0.0], [0.0, 0.0]] * 3), np.array([[0, 1]] * 3, dtype=np.int32))
    t.n[1] = 2 ** 20          # as if the pair had been hit a million times
    with pytest.raises(AssertionError, match="overflow"):
        t.tables()
    # d = 2, the densest table: every sample hits the one pair
    lifts, perms = PT.integer_batches(2, 513, seed=2, n_batches=1)[0]
    count = PT.PairTruth(2).add_batch(lifts, perms).tables()[0]
    assert count[0, 1] == 513


# ---- 3. against the definition, in rationals ---------------------------------------------------------------------------
def rational_index(v, d):
    """pair_ref.interaction_index with Fraction weights on an integer game: the definition, exactly."""
    out = {}
    for a in range(d):
        for b in range(a + 1, d):
            acc = Fraction(0)
            for S in range(1 << d):
                if S & ((1 << a) | (1 << b)):
                    continue
                s = bin(S).count("1")
                dd = int(v[S | (1 << a) | (1 << b)]) - int(v[S | (1 << a)]) - int(v[S | (1 << b)]) + int(v[S])
                acc += Fraction(factorial(s) * factorial(d - 2 - s), factorial(d - 1)) * dd
            out[a, b] = acc
    return out


@pytest.mark.parametrize("d", [5, 6])
def test_mean_over_all_orderings_is_the_index_in_rationals(d):
    rng = np.random.default_rng(50 + d)
    v = rng.integers(-1000, 1001, size=1 << d).astype(np.float64)
    v[0] = 0.0
    perms = np.array(list(itertools.permutations(range(d))), dtype=np.int32)
    lifts = pair_ref.game_lifts(v, pair_ref.expand(perms))
    half = len(perms) // 3
    truth = PT.PairTruth(d, shift=17).add_batch(lifts[:3 * half], perms[:half]).add_batch(lifts[3 * half:], perms[half:])
    count, mean, _, _ = truth.tables()
    off = ~np.eye(d, dtype=bool)
    assert np.all(count[off] == 2 * factorial(d - 1))
    want = rational_index(v, d)
    floats = pair_ref.interaction_index(v, d)
    for (a, b), w in want.items():
        assert truth.mean_fraction(a, b) == w                 # exactly
        assert truth.mean_fraction(b, a) == w
        assert abs(float(mean[a, b]) - float(w)) <= EPS * abs(float(w))          # the table is that rational, rounded
        assert abs(floats[a, b] - float(w)) <= 16 * EPS * 4000           # pair_ref's floats say the same
    np.testing.assert_allclose(truth.phi.astype(np.float64).sum(), v[-1], rtol=0, atol=1e-9)


# ---- 4. the offset class has teeth -------------------------------------------------------------------------------------
def offset_tolerances(ref, truth_tables):
    """The tolerances tests/test_gpu_sampled_edges.py holds the kernel to on the offset data: max(floor, MG e_plain),
    e_plain the error of pair_ref (fp64 NumPy, the kernel's order) against the exact truth; floors 8 n eps max|Delta|
    for the mean and 8 n eps max|u|^2 for M2."""
    count, mean, m2, max_delta = truth_tables
    e_mean = float(np.abs(ref.mean - mean).max())
    e_m2 = float(np.abs(ref.m2 - m2).max())
    n = int(count.max())
    return (e_mean, max(8 * n * EPS * float(max_delta.max()), MG * e_mean)), (e_m2, max(8 * n * EPS * 8.0 ** 2, MG * e_m2))


def test_offset_class_fails_the_one_pass_formula():
    batches = PT.offset_batches()
    ref, truth = both(PT.OFFSET_D, batches, shift=PT.OFFSET)
    tables = truth.tables()
    count, mean, m2, max_delta = tables
    # the data are what the case says: every Delta = 2^30 + u, |u| <= 8, and the variance is there
    assert truth.max_u <= 8 and np.all(max_delta[count > 0] >= PT.OFFSET - 8) and max_delta.max() <= PT.OFFSET + 8
    assert np.all(m2 >= 0) and float(m2.max()) > 100
    (e_mean, tol_mean), (e_m2, tol_m2) = offset_tolerances(ref, tables)
    naive = PT.naive_m2(batches, PT.OFFSET_D)
    naive_err = float(np.abs(naive - m2).max())
    print(f"offset class: e_plain mean {e_mean:.2e} (tol {tol_mean:.2e}), e_plain M2 {e_m2:.2e} (tol {tol_m2:.2e}), "
          f"sum x^2 - n mean^2 in fp64 misses M2 by {naive_err:.2e}")
    assert e_m2 <= tol_m2 and e_mean <= tol_mean
    assert naive_err > 100 * tol_m2           # not a near miss: the case tells the two formulas apart
    # without the common offset the same formula is inside the ordinary bound: it is the offset that bites
    plain = PT.integer_batches(PT.OFFSET_D, PT.OFFSET_B, seed=30, lo=-4, hi=4)
    t0 = PT.PairTruth(PT.OFFSET_D).add_batch(*plain[0]).add_batch(*plain[1]).tables()
    assert float(np.abs(PT.naive_m2(plain, PT.OFFSET_D) - t0[2]).max()) <= 8 * int(t0[0].max()) * EPS * 8.0 ** 2
