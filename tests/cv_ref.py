"""NumPy restatement of the K-fold cross-validation calls (include/lsspa.h, lsspa_cv_*), in long double.

TESTS ONLY.  Rows z_i = [x_i, y_i]; fold f holds the rows with fold_ids[i] == f, S_f = sum_{i in f} z_i z_i^T.  Fold
problem f, with W_f = N - n_f:
    G_f = (sum_{j != f} S_j)[:p,:p] / W_f + reg I,  g_f likewise,  H_f = S_f[:p,:p],  h_f = S_f[:p,p],
every fold over the pooled ||y||^2 = sum_j S_j[p][p].  v_f(K) = (2 th.h_K - th.H_KK th) / ||y||^2 with th = G_KK^-1 g_K,
v_cv = sum_f v_f, phi_cv = the Shapley value of v_cv.  Everything over all 2^p subsets at once (p <= 12): the subsets are
the leading axis of one batched Cholesky whose rows and columns outside a subset are masked to the identity.
"""
from math import comb

import numpy as np

import perm_ref

LD = np.longdouble


def fold_ids(n, K, seed=42, shuffle=True):
    """[n] int32: row pi[i] goes to fold i mod K, pi the host permutation of (seed, replicate 0, side 0, n); without
    shuffle row i goes to fold i mod K."""
    ids = np.empty(n, dtype=np.int32)
    order = perm_ref.indices(seed, 0, 0, n).astype(np.int64) if shuffle else np.arange(n)
    ids[order] = np.arange(n) % K
    return ids


def problems(X, y, ids, K, reg=0.0):
    """([(G_f, g_f, H_f, h_f)] for f < K, yy): the fold problems and the pooled ||y||^2, long double."""
    Z = np.concatenate([np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64)[:, None]], axis=1).astype(LD)
    n, c = Z.shape
    p = c - 1
    S = [Z[ids == f].T @ Z[ids == f] for f in range(K)]
    yy = sum(S[f][p, p] for f in range(K))
    out = []
    for f in range(K):
        A = sum(S[j] for j in range(K) if j != f)
        W = LD(n - int((ids == f).sum()))
        G = A[:p, :p] / W + LD(reg) * np.eye(p, dtype=LD)
        out.append((G, A[:p, p] / W, S[f][:p, :p], S[f][:p, p]))
    return out, yy


def all_values(G, g, H, h, yy):
    """v [2^p] (long double): the value of every subset of one problem, mask m = bit j for column j."""
    p = len(g)
    m = np.arange(1 << p)
    inn = ((m[:, None] >> np.arange(p)) & 1).astype(bool)                      # [M][p]
    both = inn[:, :, None] & inn[:, None, :]
    A = np.where(both, G[None], np.eye(p, dtype=LD)[None])
    b = np.where(inn, g[None], LD(0))
    L = np.zeros_like(A)
    for j in range(p):
        d = A[:, j, j] - (L[:, j, :j] ** 2).sum(axis=1)
        L[:, j, j] = np.sqrt(d)
        if j + 1 < p:
            L[:, j + 1:, j] = (A[:, j + 1:, j] - np.einsum("mik,mk->mi", L[:, j + 1:, :j], L[:, j, :j])) / L[:, j, j, None]
    t = np.zeros_like(b)
    for i in range(p):
        t[:, i] = (b[:, i] - (L[:, i, :i] * t[:, :i]).sum(axis=1)) / L[:, i, i]
    th = np.zeros_like(b)
    for i in range(p - 1, -1, -1):
        th[:, i] = (t[:, i] - (L[:, i + 1:, i] * th[:, i + 1:]).sum(axis=1)) / L[:, i, i]
    lin = th @ h
    quad = np.einsum("mi,ij,mj->m", th, H, th)
    return (2 * lin - quad) / yy


def cv_values(X, y, ids, K, reg=0.0):
    """(v_cv [2^p], v_fold [2^p][K]), long double."""
    probs, yy = problems(X, y, ids, K, reg)
    vf = np.stack([all_values(*pr, yy) for pr in probs], axis=1)
    v = vf[:, 0].copy()
    for f in range(1, K):
        v = v + vf[:, f]
    return v, vf


def shapley(v, p):
    """phi [p] (long double) of the table v [2^p] of a game."""
    m = np.arange(1 << p)
    size = np.array([bin(int(x)).count("1") for x in m])
    phi = np.zeros(p, dtype=LD)
    for j in range(p):
        without = m[(m >> j) & 1 == 0]
        w = np.array([LD(1) / LD(p * comb(p - 1, int(s))) for s in size[without]], dtype=LD)
        phi[j] = (w * (v[without | (1 << j)] - v[without])).sum()
    return phi


def best(v, p, include=0, ok=None):
    """(best [p + 1], masks [p + 1], found [p + 1], runner [p + 1]) of the table v: per size the largest value among the
    subsets that contain `include` (and, with ok [2^p] bool, are candidates), on equal values the smaller mask; NaN / 0 /
    False where a size has none; runner: the second largest value (-inf: none)."""
    m = np.arange(1 << p)
    size = np.array([bin(int(x)).count("1") for x in m])
    cand = (m & include) == include
    if ok is not None:
        cand &= ok
    bestv, masks = np.full(p + 1, np.nan, dtype=v.dtype), np.zeros(p + 1, dtype=np.uint32)
    found, runner = np.zeros(p + 1, dtype=bool), np.full(p + 1, -np.inf)
    for k in range(p + 1):
        sel = m[cand & (size == k) & ~np.isnan(v)]
        if len(sel) == 0:
            continue
        vals = v[sel]
        top = vals.max()
        bestv[k], masks[k], found[k] = top, sel[vals == top].min(), True
        rest = vals[sel != masks[k]]
        if len(rest):
            runner[k] = float(rest.max())
    return bestv, masks, found, runner


def split_value(X_train, X_test, y_train, y_test, cols, yy, reg=0.0):
    """The split formula on explicit rows, for vetting: 1-fold value of the columns `cols` over the denominator yy --
    (||y_te||^2 - ||y_te - X_te th||^2) / yy with th the ridge fit on the training rows."""
    Xa, Xe = np.asarray(X_train, dtype=LD)[:, cols], np.asarray(X_test, dtype=LD)[:, cols]
    ya, ye = np.asarray(y_train, dtype=LD), np.asarray(y_test, dtype=LD)
    n = LD(Xa.shape[0])
    G = (Xa.T @ Xa / n + LD(reg) * np.eye(len(cols), dtype=LD)).astype(np.float64)
    th = np.linalg.solve(G, (Xa.T @ ya / n).astype(np.float64)).astype(LD)
    r = ye - Xe @ th
    return (ye @ ye - r @ r) / yy


def data(p, n, seed, noise=0.5):
    """A regression problem with a clear signal on every third column: (X [n][p], y [n]) float64."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, p)) + 0.3 * rng.standard_normal((n, 1))
    beta = np.where(np.arange(p) % 3 == 0, 1.0 + 0.37 * np.arange(p), 0.05 * (1 + np.arange(p) % 5))
    y = X @ beta + noise * rng.standard_normal(n)
    return X, y
