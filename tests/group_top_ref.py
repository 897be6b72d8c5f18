"""Truth of ls_spa_top_group_subsets  --  TEST INFRASTRUCTURE, NOT PRODUCT CODE.

The T best group subsets of every size are tests/top_ref.py's top_truth over the g groups as players, from u of all 2^g
group masks (tests/group_best_ref.py).  Where brute force cannot go, the planted additive design over groups: column
worths drawn at random per group (top_ref.generic_worths -- the grid of tests/test_gpu_group_best.py's planted is no use
here: equal spacing makes different subsets' sums coincide), the group's worth their sum, and top_ref.additive_top's
search for the T best of every size."""
import functools

import numpy as np

import group_best_ref as R
import top_ref as T_

# (case of group_best_ref.PLANTED, seed, T) the GPU tests run; tests/test_top_group_subsets_host.py asserts their gaps
PLANTED_RUNS = (("g20x3", 6102, 4), ("g20x3", 6102, 16), ("g28", 2811, 4))


def planted_groups(labels, seed):
    """(data, dj [p], dk [g]): top_ref.planted on t = generic_worths(g, seed)[labels] -- every column of group k has the
    worth t_k --, the columns' d and their sums over each group's columns: u(S) = sum_{k in S} dk_k up to a few p eps."""
    labels = np.asarray(labels)
    g = int(labels.max()) + 1
    t = T_.generic_worths(g, seed)[labels]
    data, dj = T_.planted(t, seed)
    dk = np.array([dj[labels == k].sum() for k in range(g)])
    return data, dj, dk


@functools.lru_cache(maxsize=None)
def planted_case(name, seed, T):
    """(data, labels, dk, values [g + 1][T], masks [g + 1][T], gap) of the planted design on group_best_ref.PLANTED[name]:
    the search's T best of every size and the smallest difference between neighbours among the T + 1 best of any size.
    Computed once, shared, never written."""
    labels = R.PLANTED[name][0]
    g = int(labels.max()) + 1
    data, _, dk = planted_groups(labels, seed)
    vals, masks, gap = np.full((g + 1, T), np.nan), np.zeros((g + 1, T), dtype=np.uint32), np.inf
    for k in range(g + 1):
        v, m = T_.additive_top(dk, k, T + 1)
        if len(v) > 1:
            gap = min(gap, float(-np.diff(v).max()))
        n = min(T, len(v))
        vals[k, :n], masks[k, :n] = v[:n], m[:n]
    for a in (dk, vals, masks):
        a.setflags(write=False)
    return data, labels, dk, vals, masks, gap


def neighbour_gap(u_all, g, T):
    """The smallest difference between neighbours among the T best of every size."""
    v, _, count = T_.top_truth(u_all, g, T)
    return min(float(-np.diff(v[k, :count[k]]).max()) for k in range(g + 1) if count[k] > 1)
