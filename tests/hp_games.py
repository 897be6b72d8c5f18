"""Long-double truths for the games built on the one-response enumeration  --  TEST INFRASTRUCTURE, NOT PRODUCT CODE.

tests/hp_ref.py knows one response on one pair of row sets.  This module adds, in the same arithmetic (long double from
the fp64 inputs on) and with the same bookkeeping of the smallest relative pivot d_j / G_jj:

    MultiProblem    Y with m columns on one design: values(masks) [n][m], shapley() [m][p] or, with labels, [m][g].
    owen            the Owen value of every column of an hp_ref.Problem for a labelling (include/lsspa.h,
                    lsspa_groups_owen; tests/owen_ref.py restates the same definition in fp64).
    RowsProblem     one response, the Gram quantities formed in long double from rows and non-negative weights per side
                    (a bootstrap replicate, lsspa_boot_run) or from fold labels (a fold problem of lsspa_cv_load, through
                    tests/cv_ref.py:problems): mask_value, group_value, shapley(labels), and the smallest relative pivot
                    of that replicate or fold alone.

All of them evaluate subsets through `table`: the subsets are the leading axis of ONE column Cholesky whose rows and
columns outside a subset are masked to the identity (the device of tests/cv_ref.py:all_values), with the m responses
carried as m right-hand sides -- one factorisation per subset serves every response.  The pivots of a subset come in
ascending column order, as in hp_ref.Problem.subset_value, so the two agree to the rounding of a long double.

plain_rows_problem / plain_fold_problems form the same reduced problems in fp64 NumPy: with the fp64 host oracles
(subset_values, exact_shapley, group_shapley, multi_subset_values, multi_group_values, owen_values) they are the
same-precision routes whose error against the truth is the e_plain of tests/test_gpu_accuracy.py's rule."""
from math import comb

import numpy as np

import cv_ref
import hp_ref

LD = np.longdouble


class _Float64:
    """A third arithmetic for `table`: the same masked column Cholesky in fp64 NumPy -- the Cholesky form of the route,
    a second same-precision reference beside the LU solves of the host oracles (Numerics)."""
    name = "float64"
    dtype = np.float64

    def conv(self, a):
        return np.asarray(a, dtype=np.float64)

    def zeros(self, shape):
        return np.zeros(shape)

    def sqrt(self, x):
        with np.errstate(invalid="ignore"):
            return np.sqrt(x)

    def to_float(self, a):
        return np.asarray(a, dtype=np.float64)


FP64 = _Float64()
CHUNK = 512          # subsets factored together: CHUNK * p * p long doubles


def bits_of(masks, n):
    """[len(masks)][n] bool: bit j of every mask."""
    masks = np.asarray(masks, dtype=np.uint64)
    return ((masks[:, None] >> np.arange(n, dtype=np.uint64)) & np.uint64(1)).astype(bool)


def group_members(masks, labels):
    """[len(masks)][p] bool: the baseline columns (label -1) and the columns of the groups in each mask (bit k)."""
    labels = np.asarray(labels)
    ng = int(labels.max()) + 1
    b = bits_of(masks, ng)
    return np.where(labels[None, :] < 0, True, b[:, np.maximum(labels, 0)])


def _num(ar, x):
    """The fp64 number x as a scalar of the arithmetic."""
    return ar.conv(np.float64(x))[()]


def _sqrt(ar, d):
    return ar.sqrt(d) if ar.dtype is not object else np.array([ar.sqrt(x) for x in d], dtype=object)


def _table(G, g, H, h, yy, member, ar):
    n, p = member.shape
    both = member[:, :, None] & member[:, None, :]
    A = np.where(both, G[None], ar.conv(np.eye(p))[None])
    B = np.where(member[:, None, :], g[None], _num(ar, 0.0))                   # [n][m][p]
    L = ar.zeros(A.shape)
    piv = np.full(n, np.inf)
    with np.errstate(invalid="ignore", divide="ignore"):
        for j in range(p):
            d = A[:, j, j] - (L[:, j, :j] ** 2).sum(axis=1)
            piv = np.minimum(piv, np.where(member[:, j], (d / A[:, j, j]).astype(np.float64), np.inf))
            L[:, j, j] = _sqrt(ar, d)
            if j + 1 < p:
                L[:, j + 1:, j] = (A[:, j + 1:, j] - (L[:, j + 1:, :j] * L[:, j, None, :j]).sum(axis=2)) / L[:, j, j, None]
        T = ar.zeros(B.shape)
        for i in range(p):                                                     # L t = g_S
            T[:, :, i] = (B[:, :, i] - (L[:, i, None, :i] * T[:, :, :i]).sum(axis=2)) / L[:, i, i, None]
        TH = ar.zeros(B.shape)
        for i in range(p - 1, -1, -1):                                         # L^T theta = t
            TH[:, :, i] = (T[:, :, i] - (L[:, i + 1:, i, None].transpose(0, 2, 1) * TH[:, :, i + 1:]).sum(axis=2)) \
                / L[:, i, i, None]
        lin = (TH * h[None]).sum(axis=2)
        quad = ((TH @ H) * TH).sum(axis=2)
        return (2 * lin - quad) / yy[None, :], piv


def table(G, g, H, h, yy, member, ar=hp_ref.LD):
    """(v [n][m] in the arithmetic `ar`, piv [n] float64): v_r(S) = (2 th.h_S - th.H_SS th) / yy_r, th = G_SS^-1 g_S, for the
    column sets member [n][p] (bool) and the responses g, h [m][p], yy [m]; piv the smallest relative pivot d_j / G_jj
    of each set's factorisation (inf for the empty set, whose value is 0)."""
    member = np.asarray(member, dtype=bool)
    g, h, yy = np.atleast_2d(g), np.atleast_2d(h), np.atleast_1d(yy)
    parts = [_table(G, g, H, h, yy, member[i:i + CHUNK], ar) for i in range(0, len(member), CHUNK)]
    if not parts:
        return ar.zeros((0, len(yy))), np.zeros(0)
    return np.concatenate([v for v, _ in parts]), np.concatenate([q for _, q in parts])


def shapley_of_table(u, n, ar=hp_ref.LD):
    """phi [m][n] (in the arithmetic `ar`) of the tables u [2^n][m] of m games of n players."""
    masks = np.arange(1 << n, dtype=np.int64)
    size = bits_of(masks, n).sum(axis=1)
    w = np.array([_num(ar, 1.0) / _num(ar, n * comb(n - 1, k)) for k in range(n)], dtype=ar.dtype)
    phi = ar.zeros((u.shape[1], n))
    for k in range(n):
        S_ = masks[(masks >> k) & 1 == 0]
        phi[:, k] = (w[size[S_]][:, None] * (u[S_ | (1 << k)] - u[S_])).sum(axis=0)
    return phi


class _Tables:
    """The batched evaluation, for a problem that has G, H [p][p], gm, hm [m][p] and yym [m] in its arithmetic `ar`."""

    def _note(self, piv):
        if len(piv):
            self.min_pivot = min(self.min_pivot, float(np.min(piv)))

    def values(self, masks, with_pivots=False):
        """v [len(masks)][m] (long double) of the column subsets `masks` (bit j = column j)."""
        v, piv = table(self.G, self.gm, self.H, self.hm, self.yym, bits_of(masks, self.p), self.ar)
        self._note(piv)
        return (v, piv) if with_pivots else v

    def group_values(self, masks, labels, with_pivots=False):
        """u [len(masks)][m]: the baseline and the columns of the groups in each mask (bit k = group k)."""
        v, piv = table(self.G, self.gm, self.H, self.hm, self.yym, group_members(masks, labels), self.ar)
        self._note(piv)
        return (v, piv) if with_pivots else v

    def all_values(self, labels=None, with_pivots=False):
        """The table of all 2^p subsets, or of all 2^g sets of groups."""
        if labels is None:
            return self.values(np.arange(1 << self.p, dtype=np.uint64), with_pivots)
        return self.group_values(np.arange(1 << (int(np.max(labels)) + 1), dtype=np.uint64), labels, with_pivots)

    def _shapley(self, labels):
        n = self.p if labels is None else int(np.max(labels)) + 1
        assert n <= 16
        return shapley_of_table(self.all_values(labels), n, self.ar)

    def _set(self, ar, G, g, H, h, yy):
        """G, g, H, h, yy already in the arithmetic `ar`."""
        self.ar, self.G, self.H = ar, G, H
        self.gm, self.hm, self.yym = np.atleast_2d(g), np.atleast_2d(h), np.atleast_1d(yy)
        self.g, self.h, self.yy = self.gm[0], self.hm[0], self.yym[0]      # response 0, for hp_ref.Problem's methods
        self.p, self.n_responses = self.G.shape[0], len(self.yym)
        self.m, self.tri = self.p, True
        self.min_pivot = self.min_pivot_test = float("inf")
        self._lift_cache = {}


class MultiProblem(_Tables, hp_ref.Problem):
    """hp_ref.Problem for Y_train [N][m], Y_test [M][m] on one design (include/lsspa.h, lsspa_multi_load)."""

    def __init__(self, X_train, X_test, Y_train, Y_test, reg=0.0, ar=hp_ref.LD):
        Xa, Xe, Ya, Ye = (ar.conv(np.asarray(a, dtype=np.float64)) for a in (X_train, X_test, Y_train, Y_test))
        if Ya.ndim == 1:
            Ya, Ye = Ya[:, None], Ye[:, None]
        n, p = Xa.shape
        nn = _num(ar, n)
        self._set(ar, (Xa.T @ Xa) / nn + _num(ar, reg) * ar.conv(np.eye(p)), ((Xa.T @ Ya) / nn).T, Xe.T @ Xe,
                  (Xe.T @ Ye).T, (Ye * Ye).sum(axis=0))
        self.m = Xe.shape[0]

    def shapley(self, labels=None, raw=False):
        """phi [m][p], or [m][g] over the groups of `labels`."""
        phi = self._shapley(labels)
        return phi if raw else self.ar.to_float(phi)

    def total(self, labels=None):
        """[m] float64: what a row of shapley() sums to -- R^2 of all columns, less that of the baseline alone."""
        if labels is None:
            u = self.values(np.array([0, (1 << self.p) - 1], dtype=np.uint64))
        else:
            u = self.group_values(np.array([0, (1 << (int(np.max(labels)) + 1)) - 1], dtype=np.uint64), labels)
        return self.ar.to_float(u[1] - u[0])


class RowsProblem(_Tables, hp_ref.Problem):
    """One response, the reduced problem formed in long double from the rows Z = [X | y] of each side and non-negative
    weights (include/lsspa.h, lsspa_boot_run): S = sum_i w_i z_i z_i^T per side, W = sum_i w_i of the training side,
    G = S_tr[:p,:p] / W + reg I, g = S_tr[:p,p] / W, H = S_te[:p,:p], h = S_te[:p,p], ||y||^2 = S_te[p][p]."""

    def __init__(self, Z_train, w_train, Z_test, w_test, reg=0.0, ar=hp_ref.LD):
        w64 = [np.asarray(a, dtype=np.float64) for a in (w_train, w_test)]
        assert all((w >= 0).all() and w.sum() > 0 for w in w64)
        Za, Ze = (ar.conv(np.asarray(a, dtype=np.float64)) for a in (Z_train, Z_test))
        wa, we = (ar.conv(w) for w in w64)
        p = Za.shape[1] - 1
        Sa, Se, W = (Za * wa[:, None]).T @ Za, (Ze * we[:, None]).T @ Ze, wa.sum()
        self._set(ar, Sa[:p, :p] / W + _num(ar, reg) * ar.conv(np.eye(p)), Sa[:p, p] / W, Se[:p, :p], Se[:p, p],
                  Se[p, p])

    @classmethod
    def of_gram(cls, G, g, H, h, yy):
        """From long-double Gram quantities that a caller formed from the rows (the fold problems below)."""
        self = cls.__new__(cls)
        self._set(hp_ref.LD, *(np.asarray(a, dtype=LD) for a in (G, g, H, h, yy)))
        return self

    @classmethod
    def of_folds(cls, X, y, ids, K, reg=0.0):
        """The K fold problems of lsspa_cv_load as tests/cv_ref.py:problems forms them; each has the pooled ||y||^2."""
        probs, yy = cv_ref.problems(X, y, np.asarray(ids), K, reg)
        return [cls.of_gram(*pr, yy) for pr in probs]

    def shapley(self, labels=None, raw=False):
        """phi [p], or [g] over the groups of `labels`: hp_ref.Problem.shapley from the batched table."""
        phi = self._shapley(labels)[0]
        return phi if raw else self.ar.to_float(phi)


# ---- Owen values -------------------------------------------------------------------------------------------------------
def refined_labels(labels, k):
    """(labels of target k's refined game, b): the other groups whole as players 0 .. g-2, the target's b columns as
    players g-1 .. g-2+b in column order, the baseline -1 (the numbering of tests/owen_ref.py)."""
    labels = np.asarray(labels)
    ng = int(labels.max()) + 1
    ref = np.full(len(labels), -1, dtype=np.int64)
    for idx, l in enumerate([l for l in range(ng) if l != k]):
        ref[labels == l] = idx
    inner = np.nonzero(labels == k)[0]
    ref[inner] = ng - 1 + np.arange(len(inner))
    return ref, len(inner)


def owen(ref, labels, raw=False):
    """Ow [p] of response 0 of the hp_ref.Problem `ref` (0 on baseline columns): for column i of group k
    sum over R within groups \\ {k}, T within B_k \\ {i} of |R|! (g-1-|R|)! / g! |T|! (b-1-|T|)! / b!
    (v(B + cols(R) + T + i) - v(B + cols(R) + T)), from the long-double table of k's refined game.  ref.min_pivot takes
    in every factorisation made."""
    labels, ar = np.asarray(labels), ref.ar
    ng = int(labels.max()) + 1
    out = ar.zeros(len(labels))
    for k in range(ng):
        rl, b = refined_labels(labels, k)
        n = ng - 1 + b
        masks = np.arange(1 << n, dtype=np.int64)
        u, piv = table(ref.G, ref.g, ref.H, ref.h, ref.yy, group_members(masks, rl), ar)
        ref.min_pivot = min(ref.min_pivot, float(piv.min()))
        u = u[:, 0]
        r = bits_of(masks & ((1 << (ng - 1)) - 1), ng - 1).sum(axis=1) if ng > 1 else np.zeros(len(masks), dtype=int)
        t = bits_of(masks >> (ng - 1), b).sum(axis=1)
        wo = np.array([_num(ar, 1.0) / _num(ar, ng * comb(ng - 1, i)) for i in range(ng)], dtype=ar.dtype)
        wi = np.array([_num(ar, 1.0) / _num(ar, b * comb(b - 1, i)) for i in range(b)], dtype=ar.dtype)
        cols = np.nonzero(labels == k)[0]
        for i in range(b):
            bit = 1 << (ng - 1 + i)
            S_ = masks[(masks & bit) == 0]
            out[cols[i]] = (wo[r[S_]] * wi[t[S_]] * (u[S_ | bit] - u[S_])).sum()
    return out if raw else ar.to_float(out)


# ---- the same reduced problems at fp64 ---------------------------------------------------------------------------------
def plain_rows_problem(Z_train, w_train, Z_test, w_test, reg=0.0):
    """(G, g, H, h, yy) of RowsProblem in fp64 NumPy."""
    Za, Ze, wa, we = (np.asarray(a, dtype=np.float64) for a in (Z_train, Z_test, w_train, w_test))
    p = Za.shape[1] - 1
    Sa, Se, W = (Za * wa[:, None]).T @ Za, (Ze * we[:, None]).T @ Ze, wa.sum()
    return Sa[:p, :p] / W + reg * np.eye(p), Sa[:p, p] / W, Se[:p, :p], Se[:p, p], float(Se[p, p])


def plain_fold_problems(X, y, ids, K, reg=0.0):
    """[(G, g, H, h, yy)] of RowsProblem.of_folds in fp64 NumPy: per-fold Grams, the others summed, divided by N - n_f."""
    Z = np.concatenate([np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64)[:, None]], axis=1)
    ids = np.asarray(ids)
    n, p = Z.shape[0], Z.shape[1] - 1
    S = [Z[ids == f].T @ Z[ids == f] for f in range(K)]
    yy = float(sum(S[f][p, p] for f in range(K)))
    out = []
    for f in range(K):
        A = sum(S[j] for j in range(K) if j != f)
        W = float(n - int((ids == f).sum()))
        out.append((A[:p, :p] / W + reg * np.eye(p), A[:p, p] / W, S[f][:p, :p], S[f][:p, p], yy))
    return out
