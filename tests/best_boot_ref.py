"""Truth of a replicate of ls_spa_best_subsets_bootstrap  --  TEST INFRASTRUCTURE, NOT PRODUCT CODE.

A replicate with integer weights is the best-subset selection on the rows repeated as often as their weight says: its
truth is tests/best_ref.py's (all_values, best_truth) on the np.repeat-ed rows.  The cases the GPU tests compare with
that truth are named here, so that the host tests vet every (replicate, size) of them -- the gap between best and
runner-up -- without a GPU."""
import functools

import numpy as np

import best_ref as B

R = 3
# p -> seed of the integer weights 0 .. 3: picked on the CPU so that best and runner-up of every replicate and size are
# more than best_ref.MIN_GAP apart at both values of reg, with and without the include sets
# (tests/test_best_subsets_bootstrap_host.py asserts it)
WEIGHT_SEED = {p: 900 + p for p in B.BRUTE_P}


def weights(p):
    """(w_train [R][n], w_test [R][m]) int64, 0 .. 3, for best_ref.case_data(p)."""
    d = B.case_data(p)
    rng = np.random.default_rng(WEIGHT_SEED[p])
    return rng.integers(0, 4, size=(R, d[0].shape[0])), rng.integers(0, 4, size=(R, d[1].shape[0]))


def repeated(d, wa, we):
    """The rows of d, row i of a side as often as its weight says."""
    return (np.repeat(d[0], wa, axis=0), np.repeat(d[1], we, axis=0), np.repeat(d[2], wa), np.repeat(d[3], we))


@functools.lru_cache(maxsize=None)
def boot_case(p, reg):
    """(data, w_train, w_test, v of all masks per replicate [R][2^p]): computed once, shared by the tests, never written."""
    d = B.case_data(p)
    wa, we = weights(p)
    v = np.stack([B.all_values(repeated(d, wa[r], we[r]), reg) for r in range(R)])
    for a in (wa, we, v):
        a.setflags(write=False)
    return d, wa, we, v


def includes(p, reg):
    """The include masks the GPU tests run at (p, reg): none, and at p = 9, 12 the sets of best_ref.include_sets."""
    out = [0]
    if p in B.INCLUDE_P and reg == 0.0:
        out += [B.mask_of(s) for s in B.include_sets(p)]
    return out


CASES = [(p, reg) for p in B.BRUTE_P for reg in B.BRUTE_REG]
