"""Separable games: an exact per-player truth at any p  --  TEST INFRASTRUCTURE, NOT PRODUCT CODE.

Every block of columns gets rows of its own, in X_train and in X_test, so the cross products between blocks are sums of
exact zeros: G and H are block diagonal in every precision, and with any y the game is a sum of per-block games,
v(K) = sum_b v_b(K n B_b).  By additivity and the null-player property the Shapley value of a column is its value in its
own block's game, the interaction index is the block's own inside a block and exactly 0 between blocks, and the same holds
over groups of columns that lie inside one block (baseline columns counted in their own block) and for Owen values
(unions of null players drop out of the quotient game).  The games are not additive inside a block.

hp_ref.Problem(X_train[:, B], X_test[:, B], y_train, y_test) is exactly block B's game (the same row count, the same
||y_test||^2), so a block of at most 10 players is a table of at most 1024 long-double subset values; phi, the raw
interaction index and the Owen value are folded from that table in long double by their definitions.
tests/test_separable_host.py pins all of it to the fp64 host oracles of the whole problem at small p."""
import time
from math import comb

import numpy as np

import hp_ref

LD = np.longdouble
HOST_SECONDS = {"truth": 0.0}          # spent in the long-double tables, for the report of the GPU tests
MAX_PLAYERS = 10                       # of one block's game: 2^10 long-double solves


def place(p, sizes, fixed, seed):
    """The layout helper: the columns of every block, with the positions of `fixed` ({block: positions}) in the blocks
    named there and the remaining positions dealt by a seeded permutation, so that a case hits a chosen slot."""
    taken = sorted(c for cols in fixed.values() for c in cols)
    assert len(set(taken)) == len(taken) and sum(sizes) == p
    free = [int(c) for c in np.random.default_rng(seed).permutation([c for c in range(p) if c not in set(taken)])]
    out = []
    for b, s in enumerate(sizes):
        cols = list(fixed.get(b, ()))
        assert len(cols) <= s
        cols += [free.pop() for _ in range(s - len(cols))]
        out.append(np.sort(np.asarray(cols, dtype=np.int64)))
    assert not free
    return out


def _popcount(x, bits):
    return ((np.asarray(x, dtype=np.int64)[:, None] >> np.arange(bits)) & 1).sum(axis=1)


def shapley_of_table(u, n):
    """phi [n] in long double from the table u[mask] of an n-player game."""
    masks = np.arange(1 << n, dtype=np.int64)
    size = _popcount(masks, n)
    w = np.array([LD(1) / LD(n * comb(n - 1, k)) for k in range(n)], dtype=LD)
    phi = np.zeros(n, dtype=LD)
    for k in range(n):
        S_ = masks[(masks >> k) & 1 == 0]
        phi[k] = np.sum(w[size[S_]] * (u[S_ | (1 << k)] - u[S_]))
    return phi


def interactions_of_table(u, n):
    """The raw interaction index [n][n] in long double: tests/test_interactions_host.exact_interactions restated."""
    out = np.zeros((n, n), dtype=LD)
    if n < 2:
        return out
    masks = np.arange(1 << n, dtype=np.int64)
    size = _popcount(masks, n)
    w2 = np.array([LD(1) / LD((n - 1) * comb(n - 2, s)) for s in range(n - 1)], dtype=LD)
    for i in range(n):
        for j in range(i + 1, n):
            bi, bj = 1 << i, 1 << j
            S_ = masks[(masks & (bi | bj)) == 0]
            out[i, j] = out[j, i] = np.sum(w2[size[S_]] * (u[S_ | bi | bj] - u[S_ | bi] - u[S_ | bj] + u[S_]))
    return out


def owen_of_table(u, n_outer, b):
    """Ow [b] in long double of the inner players (bits n_outer ..) of a refined game with n_outer other groups
    (tests/owen_ref.owen_of_table restated; the quotient game has n_outer + 1 players)."""
    ng = n_outer + 1
    masks = np.arange(1 << (n_outer + b), dtype=np.int64)
    r = _popcount(masks & ((1 << n_outer) - 1), n_outer + 1)
    t = _popcount(masks >> n_outer, b + 1)
    wo = np.array([LD(1) / LD(ng * comb(ng - 1, k)) for k in range(ng)], dtype=LD)
    wi = np.array([LD(1) / LD(b * comb(b - 1, k)) for k in range(b)], dtype=LD)
    out = np.zeros(b, dtype=LD)
    for i in range(b):
        bit = 1 << (n_outer + i)
        S_ = masks[(masks & bit) == 0]
        out[i] = np.sum(wo[r[S_]] * wi[t[S_]] * (u[S_ | bit] - u[S_]))
    return out


class Separable:
    """The data (Y with one column per response) and the blockwise long-double truths.  blocks[b]: the sorted columns of
    block b.  Every truth is computed once and handed out read-only."""

    def __init__(self, X_train, X_test, Y_train, Y_test, blocks):
        self.X_train, self.X_test, self.Y_train, self.Y_test = X_train, X_test, Y_train, Y_test
        self.blocks = blocks
        self.p, self.responses = X_train.shape[1], Y_train.shape[1]
        self.block_of = np.empty(self.p, dtype=np.int64)
        for b, cols in enumerate(blocks):
            self.block_of[cols] = b
        self._problems, self._tables, self._cache = {}, {}, {}
        for a in (X_train, X_test, Y_train, Y_test):
            a.setflags(write=False)

    def data(self, r=0):
        return self.X_train, self.X_test, self.Y_train[:, r], self.Y_test[:, r]

    def multi_data(self):
        return self.X_train, self.X_test, self.Y_train, self.Y_test

    def problem(self, b, r=0):
        if (b, r) not in self._problems:
            cols = self.blocks[b]
            self._problems[b, r] = hp_ref.Problem(self.X_train[:, cols], self.X_test[:, cols], self.Y_train[:, r],
                                                  self.Y_test[:, r])
        return self._problems[b, r]

    def worst_condition(self):
        """The largest 2-norm condition number of a block's G or H (fp64: a description of the data, not a truth)."""
        out = 0.0
        for cols in self.blocks:
            for X in (self.X_train[:, cols], self.X_test[:, cols]):
                out = max(out, float(np.linalg.cond(X.T @ X)))
        return out

    def min_pivot(self):
        """The true smallest relative pivot met by the long-double factorisations of every block so far."""
        return min(prob.min_pivot for prob in self._problems.values())

    def _table(self, b, r, base, players):
        """u[mask] = v_b(base + the columns of the players in mask), block-local columns, long double."""
        key = (b, r, tuple(base), tuple(tuple(c) for c in players))
        if key not in self._tables:
            assert len(players) <= MAX_PLAYERS
            t0 = time.perf_counter()
            prob = self.problem(b, r)
            u = np.zeros(1 << len(players), dtype=LD)
            for mask in range(1 << len(players)):
                cols = list(base) + [c for k, cs in enumerate(players) if (mask >> k) & 1 for c in cs]
                u[mask] = prob.subset_value(sorted(cols))
            self._tables[key] = u
            HOST_SECONDS["truth"] += time.perf_counter() - t0
        return self._tables[key]

    def _kept(self, key, make):
        if key not in self._cache:
            out = np.asarray(make(), dtype=np.float64)
            out.setflags(write=False)
            self._cache[key] = out
        return self._cache[key]

    # ---- the games over columns ------------------------------------------------------------------------------------
    def phi(self, r=0):
        def make():
            out = np.zeros(self.p, dtype=LD)
            for b, cols in enumerate(self.blocks):
                s = len(cols)
                out[cols] = shapley_of_table(self._table(b, r, (), [(c,) for c in range(s)]), s)
            return out
        return self._kept(("phi", r), make)

    def interactions(self, r=0):
        """The raw index [p][p]: the block's own inside a block, exactly 0 between blocks."""
        def make():
            out = np.zeros((self.p, self.p), dtype=LD)
            for b, cols in enumerate(self.blocks):
                s = len(cols)
                out[np.ix_(cols, cols)] = interactions_of_table(self._table(b, r, (), [(c,) for c in range(s)]), s)
            return out
        return self._kept(("inter", r), make)

    def total(self, r=0):
        """v of all columns: the sum of the blocks' full values (what sum phi is in long double)."""
        return float(sum(self._table(b, r, (), [(c,) for c in range(len(cols))])[-1]
                         for b, cols in enumerate(self.blocks)))

    # ---- the games over groups of columns --------------------------------------------------------------------------
    def _block_groups(self, labels, b):
        """(block-local baseline columns, the labels of the block's groups ascending, their block-local columns)."""
        labels = np.asarray(labels)
        cols = self.blocks[b]
        lab = labels[cols]
        ids = sorted(set(int(k) for k in lab if k >= 0))
        for k in ids:
            assert (self.block_of[labels == k] == b).all(), f"group {k} does not lie inside block {b}"
        return tuple(np.nonzero(lab == -1)[0]), ids, [tuple(np.nonzero(lab == k)[0]) for k in ids]

    def group_phi(self, labels, r=0):
        def make():
            out = np.zeros(int(np.max(labels)) + 1, dtype=LD)
            for b in range(len(self.blocks)):
                base, ids, players = self._block_groups(labels, b)
                if ids:
                    out[ids] = shapley_of_table(self._table(b, r, base, players), len(ids))
            return out
        return self._kept(("gphi", r, tuple(labels)), make)

    def group_interactions(self, labels, r=0):
        def make():
            g = int(np.max(labels)) + 1
            out = np.zeros((g, g), dtype=LD)
            for b in range(len(self.blocks)):
                base, ids, players = self._block_groups(labels, b)
                if ids:
                    out[np.ix_(ids, ids)] = interactions_of_table(self._table(b, r, base, players), len(ids))
            return out
        return self._kept(("ginter", r, tuple(labels)), make)

    def group_gain(self, labels, r=0):
        """u(all groups) - u(no group) = R^2 - R^2(B)."""
        tot = LD(0)
        for b in range(len(self.blocks)):
            base, ids, players = self._block_groups(labels, b)
            u = self._table(b, r, base, players)
            tot += u[-1] - u[0]
        return float(tot)

    def owen(self, labels, k, r=0):
        """The Owen values of the columns of group k, in column order (tests/owen_ref.py has the rule): the other groups
        of k's block are the outer players, k's columns the inner ones."""
        def make():
            b = int(self.block_of[np.nonzero(np.asarray(labels) == k)[0][0]])
            base, ids, players = self._block_groups(labels, b)
            at = ids.index(k)
            outer = [c for i, c in enumerate(players) if i != at]
            inner = [(c,) for c in players[at]]
            u = self._table(b, r, base, outer + inner)
            return owen_of_table(u, len(outer), len(inner))
        return self._kept(("owen", r, k, tuple(labels)), make)

    # ---- labels whose groups lie inside the blocks ---------------------------------------------------------------------
    def labels(self, groups, seed):
        """groups[b]: the sizes of block b's groups; the block's remaining columns are baseline (label -1).  Inside a
        block the columns are dealt to its groups by a seeded shuffle; the groups are numbered in block order and then
        renumbered by a seeded permutation, so which groups the layout makes low is the sizes' and the seed's doing."""
        rng = np.random.default_rng(seed)
        lab = np.full(self.p, -1, dtype=np.int64)
        g = 0
        for b, sizes in enumerate(groups):
            cols = rng.permutation(self.blocks[b])
            assert sum(sizes) <= len(cols)
            at = 0
            for s in sizes:
                lab[cols[at:at + s]] = g
                g, at = g + 1, at + s
        renum = rng.permutation(g)
        return np.where(lab < 0, -1, renum[np.maximum(lab, 0)])


MIX_COND = 20.0                        # of a block's mixing matrix at most


def mild_mix(rng, s):
    """I + 0.5 N(0, 1) at s <= 4 columns, the Gaussian part scaled by 2 / sqrt(s) above (the same spectral radius, about
    1, at every size), drawn again while its condition number exceeds MIX_COND.  Unscaled and unchecked, a block of 8
    columns came out with kappa(G) = 1.8e8, where NumPy's fp64 on the block alone misses the long-double phi by 9e-13:
    "mild" has to be made, not hoped for, if 1e-11 is to speak of the kernels and not of the data."""
    while True:
        mix = np.eye(s) + 0.5 * min(1.0, 2.0 / np.sqrt(s)) * rng.standard_normal((s, s))
        if np.linalg.cond(mix) <= MIX_COND:
            return mix


def make(sizes, n, m, seed, responses=1, columns=None):
    """Blocks of the given sizes on n training and m test rows.  Columns are dealt to the blocks by a seeded permutation
    (or taken from `columns`, see place()), rows disjointly (row i belongs to block i mod #blocks).  Inside a block the
    columns are a Gaussian matrix times a mild mixing matrix (mild_mix), y = X w + N(0, 1) per response."""
    rng = np.random.default_rng(seed)
    p, nb = sum(sizes), len(sizes)
    if columns is None:
        perm = rng.permutation(p)
        ends = np.cumsum(sizes)
        columns = [np.sort(perm[e - s:e]) for s, e in zip(sizes, ends)]
    assert sorted(int(c) for cols in columns for c in cols) == list(range(p))
    Xa, Xe = np.zeros((n, p)), np.zeros((m, p))
    for b, (s, cols) in enumerate(zip(sizes, columns)):
        assert len(cols) == s
        ra, re = np.arange(b, n, nb), np.arange(b, m, nb)
        mix = mild_mix(rng, s)
        Xa[np.ix_(ra, cols)] = rng.standard_normal((len(ra), s)) @ mix
        Xe[np.ix_(re, cols)] = rng.standard_normal((len(re), s)) @ mix
    W = rng.standard_normal((p, responses))
    Ya = Xa @ W + rng.standard_normal((n, responses))
    Ye = Xe @ W + rng.standard_normal((m, responses))
    return Separable(Xa, Xe, Ya, Ye, [np.asarray(c, dtype=np.int64) for c in columns])


# ---- the kernels' maps, restated (csrc/k_subsets.hip, csrc/k_groups.hip) -----------------------------------------------
SQ = 6                                  # low features of the ungrouped enumeration
LOW_COLS = 6                            # low columns of the grouped one at most


def high_pairs(p):
    """The pairs (j1, j2) of high features in the interactions kernel's order (j1-major), as FEATURE numbers; pair
    number e sits in slot e >> 6 of lane e & 63."""
    return [(SQ + j1, SQ + j2) for j1 in range(p - SQ) for j2 in range(j1 + 1, p - SQ)]


def sweep_slot(mask, p):
    """The last entry slot a lane owns in the sweep matrix of the subset `mask`: n = |high part| + q + 1 rows, n^2
    entries dealt as entry e to slot e >> 6."""
    n = bin(int(mask) >> SQ).count("1") + min(p, SQ) + 1
    return n, (n * n - 1) >> 6


def group_layout(labels):
    """(gl, gh, ql, nb) by the layout rule: the smallest groups, ties by number, are low while their columns total
    <= 6 (tests/test_gpu_group_interactions.layout_of restated with the baseline count)."""
    labels = np.asarray(labels)
    size = np.bincount(labels[labels >= 0])
    gl = ql = 0
    for s in sorted(size):
        if ql + s > LOW_COLS:
            break
        gl, ql = gl + 1, ql + int(s)
    return gl, len(size) - gl, ql, int((labels == -1).sum())


def low_groups(labels):
    """The labels of the low groups (stable by number among equal sizes)."""
    labels = np.asarray(labels)
    size = np.bincount(labels[labels >= 0])
    order = sorted(range(len(size)), key=lambda k: (size[k], k))
    return order[:group_layout(labels)[0]]


# ---- the cases of tests/test_gpu_enum_top.py, whose reach tests/test_separable_host.py proves ---------------------------
# The smallest shapes that reach the named edge.  Each is built once (functools.lru_cache in the tests).
# phi, one response, and -- with more responses -- ls_spa_multi: blocks of 7 - 9 columns dealt by the seed; p = 32 is
# 8192 units x 8192 high subsets a unit in 64 launches.
PHI_SIZES = {29: (8, 7, 7, 7), 30: (9, 7, 7, 7), 31: (9, 8, 7, 7), 32: (9, 8, 8, 7)}
# interactions: the high-high pairs of slot 4 (p = 30) and slot 5 (p = 32) lie among the last features, so two blocks
# get two of them each (one within-block pair each, cross-block pairs between them) beside two low features
INTER_FIXED = {30: {0: [0, 1, 26, 28], 1: [2, 3, 27, 29]}, 32: {0: [0, 1, 28, 30], 1: [2, 3, 29, 31]}}
MULTI_RESPONSES = {30: 9, 32: 3}         # p = 30: two chunks of responses, the second holding one


def rows_for(sizes):
    """(n, m): every block gets 5 training and 4 test rows for each column of the widest block, and m >= p (the test
    Gram is factored)."""
    widest, blocks = max(sizes), len(sizes)
    return 5 * widest * blocks, max(4 * widest * blocks, sum(sizes))


def phi_case(p, responses=1):
    sizes = PHI_SIZES[p]
    return make(sizes, *rows_for(sizes), seed=1000 + p, responses=responses)


def inter_case(p):
    sizes = PHI_SIZES[p]
    return make(sizes, *rows_for(sizes), seed=2000 + p, columns=place(p, sizes, INTER_FIXED[p], seed=p))


# grouped: name -> (block sizes in columns, the group sizes of every block, (gl, gh, ql, nb) the layout must show)
GROUP_CASES = {
    # g = 24 over p = 64: three blocks of eight groups (four of 3 columns, four of 2) and 1 + 1 + 2 baseline columns
    # from inside the blocks; the three low groups are pairs, each beside high groups of its block
    "g24_p64": ((21, 21, 22), [[3, 3, 3, 3, 2, 2, 2, 2]] * 3, (3, 21, 6, 4)),
    # g = 28 over p = 56: four blocks of seven pairs, no baseline
    "g28_p56": ((14, 14, 14, 14), [[2] * 7] * 4, (3, 25, 6, 0)),
    # many responses: g = 24 over p = 48, three blocks of eight pairs
    "g24_p48": ((16, 16, 16), [[2] * 8] * 3, (3, 21, 6, 0)),
}
MULTI_GROUP_RESPONSES = 9


def group_case(name, responses=1):
    sizes, groups, _ = GROUP_CASES[name]
    p = sum(sizes)
    sep = make(sizes, *rows_for(sizes), seed=3000 + p, responses=responses)
    return sep, sep.labels(groups, seed=p)


def owen_case(labels, target, beside=2, per_block=3):
    """The labels of tests/owen_ref.BIG_CASE made separable: the target group and `beside` other groups are one block,
    the remaining groups blocks of `per_block` groups, in label order."""
    labels = np.asarray(labels)
    g = int(labels.max()) + 1
    others = [k for k in range(g) if k != target]
    parts = [[target] + others[:beside]] + [others[i:i + per_block] for i in range(beside, len(others), per_block)]
    columns = [np.nonzero(np.isin(labels, part))[0] for part in parts]
    sizes = tuple(len(c) for c in columns)
    p = len(labels)
    return make(sizes, *rows_for(sizes), seed=4000 + p, columns=columns), parts


# ---- subset values at the top (correlated data, not separable: tests/test_gpu_accuracy.values_case) ---------------------
def top_masks(p, n_random, seed):
    """Every size 0 .. p - 6 of the high part with the low subsets of sizes 0 and 6 (the second of the largest is the
    full mask: the sweep matrix of 33 rows at p = 32), the full mask, the single features, the last bit alone, and
    seeded random masks."""
    rng = np.random.default_rng(seed)
    nh, low_all = p - SQ, (1 << SQ) - 1
    out = []
    for k in range(nh + 1):
        hi = sum(1 << int(j) for j in rng.choice(nh, k, replace=False))
        out += [hi << SQ, (hi << SQ) | low_all]
    out += [(1 << p) - 1] + [1 << j for j in range(p)] + [1 << (p - 1)]
    out += [int(x) for x in rng.integers(0, 1 << p, n_random)]
    return np.array(out, dtype=np.uint64)


def _g32_labels():
    lab = np.repeat(np.arange(32), 2)
    np.random.default_rng(32).shuffle(lab)
    return lab


G32_LABELS = _g32_labels()              # g = 32 over p = 64: three low pairs, 29 high ones, 65 rows with all groups


def g32_masks(n_random, seed, singles=range(32)):
    """No group, the single groups, the full mask (all 64 columns), the full mask less one group, the groups 28 .. 31
    together and seeded random masks over all 32 bits."""
    full = (1 << 32) - 1
    single = [1 << k for k in singles]
    rnd = [int(x) for x in np.random.default_rng(seed).integers(0, 1 << 32, n_random)]
    return np.array([0] + single + [full] + [full ^ s for s in single] + [15 << 28, (15 << 28) | 7] + rnd, dtype=np.uint64)
