"""Truth of ls_spa_top_subsets  --  TEST INFRASTRUCTURE, NOT PRODUCT CODE.

The T best subsets of every size under the library's total order (larger value, then smaller mask; bit j = feature j)
from an array of all 2^p values (top_truth, on best_ref.popcounts); an integer design whose values are exact integers
times one constant, so that ties are exact and the tie rule is what decides (integer_design, integer_values); planted
additive designs where brute force cannot go (planted) and a best-first search for the T best size-k subsets of an
additive game (additive_top)."""
import functools
import heapq

import numpy as np

import best_ref as B

T_MAX = 16


@functools.lru_cache(maxsize=None)
def _popcounts(p):
    size = B.popcounts(p)           # (2^p x p words on the way: once per p)
    size.setflags(write=False)
    return size


def top_truth(v_all, p, T, include=0, valid=None):
    """(v [p + 1][T], masks [p + 1][T] uint32, count [p + 1]): per size the T first masks in the order "larger value,
    then smaller mask" among those that contain `include` (and, with valid [2^p] bool, are valid and not NaN), NaN / 0
    past count."""
    v_all = np.asarray(v_all, dtype=np.float64)
    size = _popcounts(p)
    masks = np.arange(1 << p, dtype=np.int64)
    ok = ((masks & include) == include) & ~np.isnan(v_all)
    if valid is not None:
        ok &= np.asarray(valid, dtype=bool)
    v = np.full((p + 1, T), np.nan)
    arg = np.zeros((p + 1, T), dtype=np.uint32)
    count = np.zeros(p + 1, dtype=np.int32)
    for k in range(p + 1):
        sel = masks[ok & (size == k)]
        order = sel[np.lexsort((sel, -v_all[sel]))][:T]
        count[k] = len(order)
        v[k, :len(order)], arg[k, :len(order)] = v_all[order], order
    return v, arg, count


# ---- exact ties: the integer design -----------------------------------------------------------------------------------
# worth of feature j in units of 1 / ||y_test||^2, all odd; equal worths among the low features (0 .. 5), between a low
# and a high one and among the high ones (the kernel's lanes enumerate the low features, its steps the high ones)
INT_WORTH = {9: (3, 3, 1, 5, -3, 1, 5, 7, 7), 12: (3, 3, 1, 5, -3, 1, 5, 7, 7, 3, -3, 9)}


def integer_design(p):
    """(X_train, X_test, y_train, y_test) with N = M = 64 rows: X_train = 2 [I_p; 0], X_test = [I_p; 0], y_train = 2 on
    the first p rows, y_test_j = (w_j + 1) / 2.  Then G = X^T X / N = I / 16, g = 1 / 16, theta = 1, H = I, h = y_test and
    v(K) = sum_{j in K} (2 h_j - 1) / ||y_test||^2 = sum_{j in K} w_j / ||y_test||^2: every intermediate is a small
    integer times a power of two, so subsets of equal integer worth have equal values to the bit."""
    w = np.array(INT_WORTH[p], dtype=np.float64)
    n = 64
    Xa, Xe = np.zeros((n, p)), np.zeros((n, p))
    Xa[np.arange(p), np.arange(p)] = 2.0
    Xe[np.arange(p), np.arange(p)] = 1.0
    ya, ye = np.zeros(n), np.zeros(n)
    ya[:p] = 2.0
    ye[:p] = (w + 1.0) / 2.0
    return Xa, Xe, ya, ye


def integer_values(p):
    """The integer worth of every mask 0 .. 2^p - 1 (as exact fp64)."""
    m = np.arange(1 << p, dtype=np.uint64)
    bits = ((m[:, None] >> np.arange(p, dtype=np.uint64)) & np.uint64(1)).astype(np.float64)
    return bits @ np.array(INT_WORTH[p], dtype=np.float64)


def ties_straddling_rank(values, p, T):
    """Sizes at which the T-th and the (T + 1)-th best value are equal: the tie rule decides who is listed."""
    v, _, count = top_truth(values, p, T + 1)
    return [k for k in range(p + 1) if count[k] == T + 1 and v[k, T - 1] == v[k, T]]


# ---- planted additive designs -----------------------------------------------------------------------------------------
def planted(t, seed):
    """Orthonormal columns on both sides (tests/test_gpu_best_subsets.py, planted): G = I / N and H = I to rounding, so
    v(K) = sum_{j in K} d_j with d_j = t_j / ||y_test||^2 up to a few p eps.  Returns (data, d)."""
    t = np.asarray(t, dtype=np.float64)
    p = len(t)
    rng = np.random.default_rng(seed)
    n = 2 * p + 8
    Qa = np.linalg.qr(rng.standard_normal((n, p)))[0]
    Qe = np.linalg.qr(rng.standard_normal((n, p)))[0]
    noise = rng.standard_normal(n)
    noise -= Qe @ (Qe.T @ noise)
    ya, ye = Qa @ np.ones(p), Qe @ ((1.0 + t) / 2.0) + noise
    a, b, yy = Qa.T @ ya, Qe.T @ ye, float(ye @ ye)
    return (Qa, Qe, ya, ye), (2.0 * a * b - a * a) / yy


def generic_worths(p, seed):
    """p worths of both signs in a shuffled order, no two sums of few of them close: drawn at random, not a grid."""
    rng = np.random.default_rng(seed)
    return rng.uniform(-1.0, 1.5, p)


def additive_top(d, k, T):
    """(values [n], masks [n]), n = min(T, C(p, k)): the T best size-k subsets of the additive game v(K) = sum_{j in K}
    d_j, best first, by a best-first search over the positions in the descending order of d: from the k largest, every
    move of one chosen position to the next free one lowers the sum, and every subset is reached by such moves.  The sums
    it returns must be distinct (asserted): among equal sums it would not know the library's order."""
    d = np.asarray(d, dtype=np.float64)
    p = len(d)
    order = np.argsort(-d, kind="stable")
    ds = d[order]

    def entry(pos):
        return (-float(ds[list(pos)].sum()), pos)

    start = tuple(range(k))
    heap, seen, out_v, out_m = [entry(start)], {start}, [], []
    while heap and len(out_v) < T:
        neg, pos = heapq.heappop(heap)
        out_v.append(-neg)
        out_m.append(sum(1 << int(order[i]) for i in pos))
        for i in range(k):
            nxt = pos[i] + 1
            if nxt < p and (i + 1 == k or nxt < pos[i + 1]):
                child = pos[:i] + (nxt,) + pos[i + 1:]
                if child not in seen:
                    seen.add(child)
                    heapq.heappush(heap, entry(child))
    assert len(set(out_v)) == len(out_v), "equal sums: the search does not know the tie rule"
    return np.array(out_v), np.array(out_m, dtype=np.uint32)


@functools.lru_cache(maxsize=None)
def planted_case(p, T, seed):
    """(data, d, values [p + 1][T], masks [p + 1][T], gap): the planted design of generic_worths(p, seed) and the search's
    T best of every size; gap: the smallest difference between neighbours among the T + 1 best of any size -- what the
    GPU test needs to be far above the rounding of the device's values.  Computed once, shared, never written."""
    data, d = planted(generic_worths(p, seed), seed)
    vals, masks, gap = np.full((p + 1, T), np.nan), np.zeros((p + 1, T), dtype=np.uint32), np.inf
    for k in range(p + 1):
        v, m = additive_top(d, k, T + 1)
        if len(v) > 1:
            gap = min(gap, float(-np.diff(v).max()))
        n = min(T, len(v))
        vals[k, :n], masks[k, :n] = v[:n], m[:n]
    for a in (d, vals, masks):
        a.setflags(write=False)
    return data, d, vals, masks, gap
