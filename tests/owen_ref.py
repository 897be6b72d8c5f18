"""The truth for the Owen value (ls_spa_owen, lsspa_groups_owen), NumPy fp64.  TESTS ONLY.

owen_values: the two-level formula over group_values() of tests/test_groups_host.py -- one numpy.linalg.solve per subset
of every group's refined game (the other groups whole, its own columns as singletons).
owen_by_orderings: the definition for tiny cases -- the mean of a column's lift over all orderings in which the baseline
comes first and every group's columns are contiguous, over value().
owen_values_fast: the same numbers as owen_values where 2^(g - 1 + b) solves of up to 64 columns per group take minutes
(12 groups of 5): per subset R of the other groups one block elimination of B + cols(R), then the 2^b subsets of the
group's columns on the b x b Schur complement, batched over R.  tests/test_owen_host.py pins it to owen_values."""
from itertools import permutations, product
from math import comb

import numpy as np

from test_groups_host import group_values, value


def refined_labels(labels, k):
    """(labels of target k's refined game, b): the other groups keep their order as players 0 .. g-2, the target's
    columns are players g-1 .. g-2+b in column order; the baseline stays -1."""
    labels = np.asarray(labels)
    ng = int(labels.max()) + 1
    ref = np.full(len(labels), -1, dtype=np.int64)
    for idx, l in enumerate([l for l in range(ng) if l != k]):
        ref[labels == l] = idx
    inner = np.nonzero(labels == k)[0]
    ref[inner] = ng - 1 + np.arange(len(inner))
    return ref, len(inner)


def owen_weights(ng, b):
    """wo[r] = r! (g - 1 - r)! / g!, wi[t] = t! (b - 1 - t)! / b!."""
    return (np.array([1.0 / (ng * comb(ng - 1, r)) for r in range(ng)]),
            np.array([1.0 / (b * comb(b - 1, t)) for t in range(b)]))


def popcount(x):
    x = np.asarray(x, dtype=np.int64)
    return ((x[:, None] >> np.arange(40)) & 1).sum(axis=1)


def owen_of_table(u, ng, b):
    """Ow of the b inner players from the table u[mask] of a refined game (outer players in bits 0 .. g-2)."""
    n = ng - 1 + b
    masks = np.arange(1 << n, dtype=np.int64)
    r = popcount(masks & ((1 << (ng - 1)) - 1))
    t = popcount(masks >> (ng - 1))
    wo, wi = owen_weights(ng, b)
    out = np.zeros(b)
    for i in range(b):
        bit = 1 << (ng - 1 + i)
        S_ = masks[(masks & bit) == 0]
        out[i] = np.sum(wo[r[S_]] * wi[t[S_]] * (u[S_ | bit] - u[S_]))
    return out


def owen_values(G, g, H, h, yy, labels):
    """Ow [p] by the two-level formula; 0.0 on baseline columns."""
    labels = np.asarray(labels)
    ng = int(labels.max()) + 1
    out = np.zeros(len(labels))
    for k in range(ng):
        ref, b = refined_labels(labels, k)
        u = group_values(G, g, H, h, yy, ref, np.arange(1 << (ng - 1 + b)))
        out[labels == k] = owen_of_table(u, ng, b)
    return out


def owen_by_orderings(G, g, H, h, yy, labels):
    """Ow [p] as the mean lift over all g! prod_k b_k! group-contiguous orderings (tiny cases only)."""
    labels = np.asarray(labels)
    ng = int(labels.max()) + 1
    base = list(np.nonzero(labels == -1)[0])
    member = [list(np.nonzero(labels == k)[0]) for k in range(ng)]
    cache = {}

    def v(cols):
        key = tuple(sorted(cols))
        if key not in cache:
            cache[key] = value(G, g, H, h, yy, np.array(key, dtype=np.int64))
        return cache[key]

    total, count = np.zeros(len(labels)), 0
    for order in permutations(range(ng)):
        for inner in product(*[list(permutations(member[k])) for k in order]):
            have = list(base)
            before = v(have)
            for blk in inner:
                for c in blk:
                    have.append(c)
                    after = v(have)
                    total[c] += after - before
                    before = after
            count += 1
    return total / count


def owen_values_fast(G, g, H, h, yy, labels):
    """owen_values by block elimination (the module's docstring)."""
    labels = np.asarray(labels)
    ng = int(labels.max()) + 1
    base = np.nonzero(labels == -1)[0]
    out = np.zeros(len(labels))
    for k in range(ng):
        inner = np.nonzero(labels == k)[0]
        b = len(inner)
        others = [np.nonzero(labels == l)[0] for l in range(ng) if l != k]
        nR = 1 << (ng - 1)
        S = np.empty((nR, b, b))
        gt, z = np.empty((nR, b)), np.empty((nR, b))
        Z, c0 = np.empty((nR, b, b)), np.empty(nR)
        for R in range(nR):
            A = np.sort(np.concatenate([base] + [others[j] for j in range(ng - 1) if (R >> j) & 1])).astype(np.int64)
            cols = np.concatenate([A, inner])
            E = np.zeros((len(cols), b))
            E[len(A):] = np.eye(b)
            e0 = np.zeros(len(cols))
            S[R], gt[R] = G[np.ix_(inner, inner)], g[inner]
            if len(A):
                W = np.linalg.solve(G[np.ix_(A, A)], np.column_stack([G[np.ix_(A, inner)], g[A]]))
                S[R] -= G[np.ix_(inner, A)] @ W[:, :b]
                gt[R] -= G[np.ix_(inner, A)] @ W[:, b]
                E[:len(A)] = -W[:, :b]
                e0[:len(A)] = W[:, b]
            Hc, hc = H[np.ix_(cols, cols)], h[cols]
            Z[R] = E.T @ Hc @ E
            z[R] = E.T @ (hc - Hc @ e0)
            c0[R] = 2.0 * e0 @ hc - e0 @ Hc @ e0
        u = np.empty(nR << b)                        # mask = R | T << (g - 1)
        for T in range(1 << b):
            sel = np.array([i for i in range(b) if (T >> i) & 1], dtype=np.int64)
            val = c0.copy()
            if len(sel):
                th = np.linalg.solve(S[:, sel][:, :, sel], gt[:, sel][:, :, None])[:, :, 0]
                val += 2.0 * np.einsum("ri,ri->r", th, z[:, sel]) - np.einsum("ri,rij,rj->r", th, Z[:, sel][:, :, sel], th)
            u[np.arange(nR) | (T << (ng - 1))] = val / yy
        out[inner] = owen_of_table(u, ng, b)
    return out


# ---- the shapes of tests/test_gpu_owen.py, and the reach tests/test_owen_host.py proves for them ------------------------
def _labels(sizes, baseline=0):
    """Group k has sizes[k] columns; the columns shuffled (which players are low depends on sizes and numbering only)."""
    lab = np.concatenate([np.full(baseline, -1)] + [np.full(s, k) for k, s in enumerate(sizes)]).astype(np.int64)
    np.random.default_rng(len(lab)).shuffle(lab)
    return lab


# name -> (labels, {target: what lsspa_debug_owen_plan must report for it})
GPU_CASES = {
    # p - nb = 6: every player of every refined game is low, no high subset but the empty one
    "sizes_2_1_3": (_labels([2, 1, 3]), {k: dict(gh=0, inner_high=0) for k in range(3)}),
    # nine columns: one outer group is high for every target, every inner player low
    "sizes_3_2_4": (_labels([3, 2, 4]), {0: dict(gh=1, inner_low=3, inner_high=0),
                                         1: dict(gh=1, inner_low=2, inner_high=0),
                                         2: dict(gh=1, inner_low=4, inner_high=0)}),
    "sizes_8_3_3_3": (_labels([8, 3, 3, 3]), {0: dict(players=11, inner_low=6, inner_high=2, gh=5)}),
    # the outer singletons take every low slot: all inner players high
    "singletons_before_the_target": (_labels([1] * 6 + [4, 5]), {6: dict(gl=6, inner_low=0, inner_high=4),
                                                                 0: dict(launches=0)}),
    # the target numbered first: its columns low, four of the outer singletons high
    "target_before_the_singletons": (_labels([4] + [1] * 6 + [5]), {0: dict(inner_low=4, inner_high=0, gh=5)}),
    "12_groups_of_5_and_4_baseline": (_labels([5] * 12, 4), {k: dict(players=16, inner_low=5, gh=11)
                                                             for k in range(12)}),
    "one_group_of_12": (_labels([12]), {0: dict(players=12, inner_low=6, inner_high=6)}),
    "singletons_p12": (_labels([1] * 12), {k: dict(players=12, launches=0) for k in range(12)}),
}
# too slow for the CPU truth: 14 outer groups of 4 and a target of 8, p = 64, 22 players
BIG_CASE = _labels([4] * 14 + [8])
BIG_PLAN = {14: dict(players=22, gh=16, inner_low=6, inner_high=2), 0: dict(players=18, gh=14, inner_low=4)}
