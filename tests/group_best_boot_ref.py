"""Truth of a replicate of ls_spa_best_group_subsets_bootstrap  --  TEST INFRASTRUCTURE, NOT PRODUCT CODE.

A replicate with integer weights is the grouped best-subset selection on the rows repeated as often as their weight
says: its truth is tests/group_best_ref.py's all_group_values on the np.repeat-ed rows, then tests/best_ref.py's
best_truth over the g groups.  The cases the GPU tests compare with that truth are named here, so that the host tests
vet every (replicate, size) of them -- the gap between best and runner-up -- without a GPU."""
import functools

import numpy as np

import best_ref as B
import group_best_ref as GR
from best_boot_ref import repeated

R = 3
NAMES = ("gl0", "gl6", "mixed", "alllow", "nine", "rect")
# case -> seed of the integer weights 0 .. 3: picked on the CPU so that best and runner-up of every replicate and size
# are more than group_best_ref.MIN_GAP apart at both values of reg, and so that every replicate of "rect" (M = 9 test
# rows) keeps a positive sum of test weights (tests/test_group_best_bootstrap_host.py asserts both)
WEIGHT_SEED = {name: 1300 + i for i, name in enumerate(NAMES)}
CASES = [(name, reg) for name in NAMES for reg in GR.REGS]


def weights(name):
    """(w_train [R][n], w_test [R][m]) int64, 0 .. 3, for group_best_ref.case_data(name)."""
    _, _, _, (n, m, _) = GR.CASES[name]
    rng = np.random.default_rng(WEIGHT_SEED[name])
    return rng.integers(0, 4, size=(R, n)), rng.integers(0, 4, size=(R, m))


def replicate_values(d, labels, wa, we, reg=0.0):
    """u of every group mask of one replicate: the one-problem truth on the repeated rows."""
    return GR.all_group_values(repeated(d, wa, we), labels, reg)


@functools.lru_cache(maxsize=None)
def boot_case(name, reg):
    """(data, labels, w_train, w_test, u of all group masks per replicate [R][2^g]): computed once, shared by the tests,
    never written."""
    d, labels = GR.case_data(name), GR.case_labels(name)
    wa, we = weights(name)
    u = np.stack([replicate_values(d, labels, wa[r], we[r], reg) for r in range(R)])
    for a in (labels, wa, we, u):
        a.setflags(write=False)
    return d, labels, wa, we, u


def truth(u_all, g):
    """best_ref.best_truth over the g groups: (best [g + 1], masks, found, runner_up)."""
    return B.best_truth(u_all, g)
