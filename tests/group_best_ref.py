"""Brute-force truth of ls_spa_best_subsets(groups=)  --  TEST INFRASTRUCTURE, NOT PRODUCT CODE.

u(S) of every one of the 2^g group masks (bit k = group k) from the grouped oracle of tests/test_groups_host.py (one fp64
solve per mask, error ~1e-14), then tests/best_ref.py's best_truth over the g players: per size (the number of groups)
the arg-max under the library's tie rule and the runner-up's value.  The cases the GPU tests run are named here, so that
the host tests can vet every one of them -- the gap between best and runner-up, and what the layout of their labels
reaches (lsspa_debug_groups_best_plan) -- without a GPU."""
import functools

import numpy as np

import best_ref as B
from test_groups_host import group_values, labels_of
from test_subsets_host import data, gram_problem

MIN_GAP = B.MIN_GAP
REGS = (0.0, 0.1)

# name -> (group sizes, baseline columns, seed of the label shuffle, (n, m, seed) of data(p, ...)); m < p: rect mode.
# Seeds picked on the CPU so that best and runner-up of every size are more than MIN_GAP apart
# (tests/test_group_best_host.py asserts it).
CASES = {
    "gl0": ([7, 7, 7], 0, 1, (80, 60, 601)),                     # no low group: only lane 0 holds a value
    "gl6": ([1] * 6 + [3, 4], 2, 2, (80, 60, 602)),              # six low singletons: every lane of 64
    "mixed": ([2, 2, 1, 2, 3], 1, 3, (80, 60, 603)),             # low 1, 2, 2; the next group of 2 no longer fits
    "alllow": ([1, 2, 3], 2, 4, (60, 40, 604)),                  # gh = 0: one unit, one step
    "nine": ([2, 5, 1, 4, 3, 6, 1, 2, 7], 3, 5, (120, 90, 605)),
    "g12p64": ([5] * 12, 4, 6, (256, 192, 606)),
    "rect": ([3, 1, 4, 2, 2, 5, 1], 2, 7, (90, 9, 607)),         # p = 20 columns, M = 9 test rows
}
RECT = ("rect",)
# what lsspa_debug_groups_best_plan must report for them
PLAN = {
    "gl0": dict(gl=0, gh=3, ql=0, nb=0, units=8, per=1, launches=1, classes=1),
    "gl6": dict(gl=6, gh=2, ql=6, nb=2, units=4, per=1, launches=1, classes=1),
    "mixed": dict(gl=3, gh=2, ql=5, nb=1, units=4, per=1, launches=1, classes=1),
    "alllow": dict(gl=3, gh=0, ql=6, nb=2, units=1, per=1, launches=1, classes=1),
    "nine": dict(gl=4, gh=5, ql=6, nb=3, units=32, per=1, launches=1, classes=1),
    "g12p64": dict(gl=1, gh=11, ql=5, nb=4, units=2048, per=1, launches=1, classes=1),
    "rect": dict(gl=4, gh=3, ql=6, nb=2, units=8, per=1, launches=1, classes=1),
}
# the planted problems of tests/test_gpu_group_best.py, where brute force cannot go: labels -> plan
PLANTED = {
    "g20x3": (np.repeat(np.arange(20), 3), dict(gl=2, gh=18, ql=6, nb=0, units=8192, per=32, launches=5, classes=6)),
    "g28": (np.arange(28), dict(gl=6, gh=22, ql=6, nb=0, units=8192, per=512, launches=21, classes=10)),
}


def case_labels(name):
    sizes, nb, shuffle, _ = CASES[name]
    return labels_of(sizes, nb, seed=shuffle)


def case_data(name):
    sizes, nb, _, (n, m, seed) = CASES[name]
    return data(sum(sizes) + nb, n=n, m=m, seed=seed)


def all_group_values(d, labels, reg=0.0):
    """u of every group mask 0 .. 2^g - 1, as fp64."""
    g = int(np.max(labels)) + 1
    return group_values(*gram_problem(*d, reg=reg), labels, np.arange(1 << g))


@functools.lru_cache(maxsize=None)
def brute_case(name, reg):
    """(data, labels, u of all group masks): computed once, shared by the tests, never written."""
    d, labels = case_data(name), case_labels(name)
    u = all_group_values(d, labels, reg)
    u.setflags(write=False)
    labels.setflags(write=False)
    return d, labels, u


def columns_of(labels, mask):
    """[p] bool: the baseline's columns and those of the groups in mask."""
    labels = np.asarray(labels)
    return (labels < 0) | (((int(mask) >> np.maximum(labels, 0)) & 1) == 1)


# ---- the exact-tie problem ----------------------------------------------------------------------------------------------
# Rounding never gives ties, so they are built: groups a (one column), b and c (seven columns each) are nonzero only on
# training rows whose y is 0, so g = X^T y / N is exactly 0 on their columns and u(S) = 0.0 exactly for every S within
# {a, b, c} (theta = 0), in any arithmetic.  Groups d (one column) and e (two) carry the signal on the other rows, with
# its sign flipped on the test side: every subset that contains one of them is worse than 0.  The layout makes a, d, e
# low and b, c high.
TIE_SIZES = dict(a=1, b=7, c=7, d=1, e=2)
# run -> caller's label of every group.  "agree": a < b < c in both numberings.  "disagree": a has the largest label but,
# being low, the smallest layout number.
TIE_RUNS = {"agree": dict(a=0, b=1, c=2, d=3, e=4), "disagree": dict(b=0, d=1, c=2, e=3, a=4)}


@functools.lru_cache(maxsize=None)
def tie_case(run):
    """(data, labels, u of all 32 masks) of the exact-tie problem under the run's numbering."""
    rng = np.random.default_rng(77)
    n0, n1, m = 40, 40, 50
    order = "abcde"
    width = [TIE_SIZES[k] for k in order]
    start = np.concatenate([[0], np.cumsum(width)])
    p = int(start[-1])
    Xa, Xe = np.zeros((n0 + n1, p)), np.zeros((m, p))
    abc = slice(0, int(start[3]))
    Xa[:n0, abc] = rng.integers(-3, 4, size=(n0, int(start[3]))).astype(float)
    Xe[:, abc] = rng.integers(-3, 4, size=(m, int(start[3]))).astype(float)
    sig = slice(int(start[3]), p)
    Xa[n0:, sig] = rng.standard_normal((n1, 3))
    w = np.array([1.0, 0.8, -0.7])
    ya = np.concatenate([np.zeros(n0), Xa[n0:, sig] @ w + 0.1 * rng.standard_normal(n1)])
    Xe[:, sig] = rng.standard_normal((m, 3))
    ye = -(Xe[:, sig] @ w) + 0.1 * rng.standard_normal(m)
    labels = np.concatenate([np.full(TIE_SIZES[k], TIE_RUNS[run][k]) for k in order]).astype(np.int64)
    perm = rng.permutation(p)                    # the columns in no particular order
    d = (Xa[:, perm], Xe[:, perm], ya, ye)
    labels = labels[perm]
    u = all_group_values(d, labels)
    u.setflags(write=False)
    labels.setflags(write=False)
    return d, labels, u


def tie_winners(run):
    """masks[1], masks[2], masks[3] the library must return: the smallest caller masks among the subsets of {a, b, c}."""
    lab = TIE_RUNS[run]
    abc = sorted(1 << lab[k] for k in "abc")
    return [abc[0], abc[0] | abc[1], abc[0] | abc[1] | abc[2]]
