"""An exact truth for the per-pair (count, mean, M2) tables of the sampled pairwise interaction index (include/lsspa.h,
lsspa_pairs_*; csrc/k_pairs.hip).  TESTS ONLY -- the product never imports this.

tests/pair_ref.py restates the kernel's own algorithm (Welford over a batch, one Chan merge a batch) in fp64; whatever
that algorithm loses, pair_ref loses too.  This file computes the same tables with no running mean at all:

    integer-valued lift vectors  ->  every Delta = lift[b] - lift'[b] is an integer
    per unordered pair, over ALL batches at once:   n,  S1 = sum u,  S2 = sum u^2,   u = Delta - c   (int64, exact)
    mean = (c n + S1) / n                           one long-double division of an exact integer
    M2   = (n S2 - S1^2) / n                        one long-double division of an exact integer

c ("shift") is an integer common to all Delta of the table; M2 does not depend on it, the sums stay small with it.  The
sums are formed with np.add.at over all (sample, position) cells of a batch -- no loop over samples, no order, nothing
that knows how the samples were cut into batches or chunks.

No overflow: with N the largest count of a pair and U the largest |u|, the largest intermediate is n S2 <= N^2 U^2 (and
|c n + S1| <= N (|c| + U)).  `tables()` checks N^2 U^2 < 2^62 and N (|c| + U) < 2^62 on the data it was given; at the
shapes of tests/test_gpu_sampled_edges.py N <= 2 * 2 * 513 = 2052 (d = 2: every sample hits the one pair; two batches),
U <= 2048 (lifts in [-1024, 1024]) or 8 (the offset class, c = 2^30), so N^2 U^2 <= 2^22 * 2^22 = 2^44 and
N (|c| + U) < 2^42 (tests/test_pairs_truth_host.py asserts both).

With dtype=np.longdouble the same machinery takes lift vectors that are not integers (the long-double lifts of real
orderings): the sums are then long-double sums (64-bit mantissa), not exact -- good for a mean that is compared at 1e-10,
and nothing else is taken from it."""
from fractions import Fraction

import numpy as np

LD = np.longdouble


def batch_deltas(lifts, perms):
    """(3 B, d) lift vectors and (B, d) orderings -> Delta (B, d - 1) and the pairs (lo, hi) they belong to, all cells at
    once: Delta[s, k] = lifts[3 s][b] - lifts[3 s + 1 + (k & 1)][b], b = perms[s, k + 1], pair {perms[s, k], b}."""
    perms = np.asarray(perms)
    B, d = perms.shape
    assert lifts.shape == (3 * B, d)
    s = np.arange(B)[:, None]
    b = perms[:, 1:]
    odd = (np.arange(d - 1) & 1).astype(bool)[None, :]
    x = lifts[0::3][s, b] - np.where(odd, lifts[2::3][s, b], lifts[1::3][s, b])
    return x, np.minimum(perms[:, :-1], b), np.maximum(perms[:, :-1], b)


class PairTruth:
    """Feed batches with add_batch, read tables().  dtype np.int64: integer-valued lifts, exact.  dtype np.longdouble:
    any lifts, long-double sums."""

    def __init__(self, d, shift=0, dtype=np.int64):
        assert dtype in (np.int64, LD) and int(shift) == shift
        self.d, self.dtype, self.shift, self.n_samples = d, dtype, int(shift), 0
        self.n = np.zeros(d * d, dtype=np.int64)           # kept at [lo][hi]
        self.s1 = np.zeros(d * d, dtype=dtype)
        self.s2 = np.zeros(d * d, dtype=dtype)
        self.col = np.zeros(d, dtype=dtype)                # sum of all lift vectors
        self.max_u = 0
        self.max_delta = np.zeros(d * d)                   # largest |Delta| of a pair (the tests' rounding bounds)

    def add_batch(self, lifts, perms):
        lifts = np.asarray(lifts)
        if self.dtype is np.int64:
            as_int = np.rint(lifts).astype(np.int64)
            assert np.array_equal(as_int, lifts), "integer-valued lifts wanted"
            lifts = as_int
        else:
            lifts = np.asarray(lifts, dtype=LD)
        x, lo, hi = batch_deltas(lifts, perms)
        at = (lo.astype(np.int64) * self.d + hi).ravel()
        u = (x - self.dtype(self.shift)).ravel()
        np.add.at(self.n, at, 1)
        np.add.at(self.s1, at, u)
        np.add.at(self.s2, at, u * u)
        np.maximum.at(self.max_delta, at, np.abs(x).ravel().astype(np.float64))
        self.max_u = max(self.max_u, float(np.abs(u).max()))
        self.col += lifts.sum(axis=0)
        self.n_samples += len(perms)
        return self

    def tables(self, symmetric=True):
        """count (int64), mean, M2 (long double), max |Delta| (fp64) as (d, d) tables; symmetric, or (symmetric=False)
        the upper triangle [lo][hi] alone with zeros below, as the device keeps them."""
        d, n = self.d, self.n
        hit = n > 0
        nn = np.where(hit, n, 1)
        if self.dtype is np.int64:
            N, U = int(n.max()), int(self.max_u)
            assert N * N * U * U < 2 ** 62 and N * (abs(self.shift) + U) < 2 ** 62, "int64 would overflow"
            mean = (self.shift * n + self.s1).astype(LD) / nn.astype(LD)
            m2 = (n * self.s2 - self.s1 * self.s1).astype(LD) / nn.astype(LD)
        else:
            nl = nn.astype(LD)
            mean = np.where(hit, LD(self.shift) + self.s1 / nl, LD(0))
            m2 = np.where(hit, (nl * self.s2 - self.s1 * self.s1) / nl, LD(0))
        out = [a.reshape(d, d) for a in (n, mean, m2, self.max_delta)]
        return [a + a.T for a in out] if symmetric else out

    def mean_fraction(self, a, b):
        """The mean of pair {a, b} as a rational (integer lifts only)."""
        assert self.dtype is np.int64
        at = min(a, b) * self.d + max(a, b)
        return Fraction(self.shift * int(self.n[at]) + int(self.s1[at]), int(self.n[at]))

    @property
    def phi(self):
        """The mean of all 3 n lift vectors (long double)."""
        return self.col.astype(LD) / LD(3 * self.n_samples)


def naive_m2(lifts_and_perms, d):
    """What the exact truth is there to catch: M2 = sum x^2 - n mean^2 in fp64, mean = sum x / n, over all batches.
    Returns the symmetric (d, d) table."""
    n, s1, s2 = np.zeros(d * d), np.zeros(d * d), np.zeros(d * d)
    for lifts, perms in lifts_and_perms:
        x, lo, hi = batch_deltas(np.asarray(lifts, dtype=np.float64), perms)
        at = (lo.astype(np.int64) * d + hi).ravel()
        np.add.at(n, at, 1.0)
        np.add.at(s1, at, x.ravel())
        np.add.at(s2, at, (x * x).ravel())
    mean = s1 / np.where(n > 0, n, 1.0)
    out = (s2 - n * mean * mean).reshape(d, d)
    return out + out.T


# ---- the cases of tests/test_gpu_sampled_edges.py (shared with the host test, which vets them without a GPU) -----------
def integer_batches(d, B, seed, n_batches=2, lo=-1024, hi=1024):
    """n_batches of (lifts (3 B, d) integer-valued fp64 in [lo, hi], perms (B, d) int32); the orderings of a batch come
    from one rng.permuted call."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_batches):
        perms = rng.permuted(np.tile(np.arange(d, dtype=np.int32), (B, 1)), axis=1)
        out.append((rng.integers(lo, hi + 1, size=(3 * B, d)).astype(np.float64), perms))
    return out


OFFSET = 2 ** 30
OFFSET_D, OFFSET_B = 65, 257


def offset_batches(d=OFFSET_D, B=OFFSET_B, seed=30):
    """Every Delta = 2^30 + u with integer |u| <= 8: a sample's first row is 2^30 + [-4, 4], its two swapped rows
    [-4, 4].  mean^2 ~ 2^60 against a variance of some 10: the cancellation case."""
    out = integer_batches(d, B, seed, lo=-4, hi=4)
    for lifts, _ in out:
        lifts[0::3] += OFFSET
    return out
