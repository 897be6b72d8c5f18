"""Brute-force truth of ls_spa_best_subsets  --  TEST INFRASTRUCTURE, NOT PRODUCT CODE.

v(K) of every one of the 2^p masks (bit j = feature j) from the oracle of tests/test_subsets_host.py -- in long double
through tests/hp_ref.py where that is cheap (p <= 9), in fp64 (one batched LAPACK solve per size, error ~1e-14) above --
then, per size, the arg-max under the library's tie rule (larger value, then smaller mask) and the runner-up's value.
The cases the GPU tests run are named here, so that the host tests can vet every one of them (the gap between best and
runner-up) without a GPU."""
import functools
import os

import numpy as np

from hp_ref import Problem
from test_subsets_host import data, gram_problem, subset_values

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
LD_MAX_P = 9
MIN_GAP = 1e-9

# (p, reg) -> seed of data(p, ...): picked on the CPU so that best and runner-up of every size are more than MIN_GAP
# apart (tests/test_best_subsets_host.py asserts it), with and without the include sets below
BRUTE_P = (1, 2, 5, 6, 7, 9, 12)
BRUTE_REG = (0.0, 0.1)
BRUTE_SEED = {p: 500 + p for p in BRUTE_P}
INCLUDE_P = (9, 12)


def include_sets(p):
    return [(0,), (3, 8), tuple(range(p))]


def case_data(p):
    return data(p, n=max(60, 3 * p), m=max(40, 2 * p), seed=BRUTE_SEED[p])


def edge_data():
    g = np.load(os.path.join(GOLDEN, "edge.npz"), allow_pickle=False)       # p = 12, M = 8: rect mode
    return [g[k] for k in ("X_train", "X_test", "y_train", "y_test")]


def all_values(d, reg=0.0):
    """v of every mask 0 .. 2^p - 1, as fp64."""
    p = d[0].shape[1]
    if p <= LD_MAX_P:
        prob = Problem(*d, reg=reg)
        return np.array([float(prob.mask_value(m)) for m in range(1 << p)])
    return subset_values(*gram_problem(*d, reg=reg), np.arange(1 << p, dtype=np.uint64))


def popcounts(p):
    m = np.arange(1 << p, dtype=np.uint64)
    return ((m[:, None] >> np.arange(p, dtype=np.uint64)) & np.uint64(1)).sum(axis=1).astype(int)


def mask_of(cols):
    return sum(1 << int(j) for j in cols)


def best_truth(v, p, include=0):
    """(best [p + 1], masks [p + 1], found [p + 1], runner_up [p + 1]) over the masks that contain `include`: per size
    the largest value (NaN where the size has no candidate), the smallest mask that attains it, and the largest value
    of another mask of that size (-inf where there is none)."""
    size = popcounts(p)
    masks = np.arange(1 << p, dtype=np.int64)
    ok = (masks & include) == include
    best, arg, found = np.full(p + 1, np.nan), np.zeros(p + 1, dtype=np.uint32), np.zeros(p + 1, dtype=bool)
    runner = np.full(p + 1, -np.inf)
    for k in range(p + 1):
        sel = masks[ok & (size == k)]                 # ascending masks: argmax takes the smallest of equal maxima
        if len(sel) == 0:
            continue
        i = int(np.argmax(v[sel]))
        best[k], arg[k], found[k] = v[sel[i]], sel[i], True
        rest = np.delete(v[sel], i)
        if len(rest):
            runner[k] = rest.max()
    return best, arg, found, runner


@functools.lru_cache(maxsize=None)
def brute_case(p, reg):
    """(data, v of all masks): computed once, shared by the tests, never written."""
    d = edge_data() if p == "edge" else case_data(p)
    v = all_values(d, reg)
    v.setflags(write=False)
    return d, v
