"""A reference more accurate than the code under test  --  TEST INFRASTRUCTURE, NOT PRODUCT CODE.

The Gram-form algorithm of DESIGN.md section 3 ("Numerics"), every step in extended precision from the fp64 inputs on:

    G = X^T X / N + reg I,  g = X^T y / N,  H = X_te^T X_te,  h = X_te^T y_te,  yy = ||y_te||^2
    per ordering pi:  G_pi = L L^T (hand-written column Cholesky),  z = L^-1 g_pi,  H_pi = L_t L_t^T,  yt = L_t^-1 h_pi,
                      V = L^-1 L_t,  N_j = sum_{k <= j} z_k V[k,:],  lift_j = z_j V[j,:].(2 yt - N_j - N_{j-1}) / yy
    M < p ("rect"):   V = L^-1 F^T[pi,:] with F = X_te, yt = y_te

One body of code runs in two arithmetics: ``LD`` (numpy.longdouble: 64-bit mantissa on x86, eps 1.1e-19) is the truth the
GPU tests compare with, ``MP`` (mpmath at 50 digits, p <= 24) exists to validate LD (tests/test_hp_ref_host.py).  The
algorithm itself is validated there against the fixtures made from the real reference and against the QR oracle.

``plain_lifts`` is the same route in ordinary NumPy / LAPACK fp64 or fp32: the same-precision baseline that sets the scale
of the tolerances.  ``gen`` makes data of a chosen condition number.
"""
from math import comb

import numpy as np
import scipy.linalg as sla


class _LongDouble:
    name = "longdouble"
    dtype = np.longdouble

    def conv(self, a):
        return np.asarray(a, dtype=np.longdouble)

    def zeros(self, shape):
        return np.zeros(shape, dtype=np.longdouble)

    def sqrt(self, x):
        with np.errstate(invalid="ignore"):
            return np.sqrt(x)

    def to_float(self, a):
        return np.asarray(a, dtype=np.float64)


class _MpMath:
    """numpy object arrays of mpmath.mpf: +, *, @, cumsum all go through the elements' own operators."""
    name = "mpmath"
    dtype = object

    def __init__(self, dps=50):
        import mpmath
        self.mp = mpmath.mp
        self.mp.dps = dps

    def conv(self, a):
        a = np.asarray(a)
        out = np.empty(a.shape, dtype=object)
        flat = out.reshape(-1)
        for i, v in enumerate(a.reshape(-1)):
            flat[i] = self.exact(v)
        return out

    def exact(self, v):
        """An fp64 or long-double number as an mpf, exactly (a 64-bit mantissa is the sum of two doubles)."""
        hi = float(v)
        lo = float(v - type(v)(hi)) if isinstance(v, np.longdouble) else 0.0
        return self.mp.mpf(hi) + self.mp.mpf(lo)

    def zeros(self, shape):
        out = np.empty(shape, dtype=object)
        out.reshape(-1)[:] = self.mp.mpf(0)
        return out

    def sqrt(self, x):
        return self.mp.sqrt(x) if x > 0 else self.mp.nan

    def to_float(self, a):
        return np.array([float(v) for v in np.asarray(a, dtype=object).reshape(-1)]).reshape(np.shape(a))


LD = _LongDouble()


def MP(dps=50):
    return _MpMath(dps)


def _dot(a, b):
    return a @ b if len(a) else 0


class Problem:
    """The reduced problem of (X_train, X_test, y_train, y_test, reg) and everything the engine computes from it, in
    the arithmetic ``ar``.  ``min_pivot`` / ``min_pivot_test`` are the smallest relative pivots L_jj^2 / G_jj met by the
    train / test factorisations of all orderings evaluated so far (what the engine's NOT_PD test looks at)."""

    def __init__(self, X_train, X_test, y_train, y_test, reg=0.0, ar=LD):
        self.ar = ar
        Xa, Xe, ya, ye = (ar.conv(np.asarray(a, dtype=np.float64)) for a in (X_train, X_test, y_train, y_test))
        n, p = Xa.shape
        self.p, self.m = p, Xe.shape[0]
        self.tri = self.m >= p
        nn = ar.conv(np.float64(n))
        self.G = (Xa.T @ Xa) / nn
        r = ar.conv(np.float64(reg))
        for j in range(p):
            self.G[j, j] = self.G[j, j] + r
        self.g = (Xa.T @ ya) / nn
        self.H = Xe.T @ Xe
        self.h = Xe.T @ ye
        self.yy = ye @ ye
        self.Ft, self.yte = Xe.T, ye
        self.min_pivot = self.min_pivot_test = float("inf")
        self._lift_cache = {}

    # ---- factorisation ------------------------------------------------------------------------------------------
    def _chol_aug(self, S, s):
        """Column Cholesky of S with the row s carried along: (L, L^-1 s, relative pivots)."""
        ar, q = self.ar, len(s)
        A = ar.zeros((q + 1, q))
        A[:q] = S
        A[q] = s
        L = ar.zeros((q + 1, q))
        piv = []
        for j in range(q):
            d = A[j, j] - _dot(L[j, :j], L[j, :j])
            piv.append(float(d / A[j, j]))
            ljj = ar.sqrt(d)
            L[j, j] = ljj
            if j:
                L[j + 1:, j] = (A[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / ljj
            else:
                L[j + 1:, j] = A[j + 1:, j] / ljj
        return L[:q], L[q], piv

    def _forward(self, L, R):
        """L^-1 R by forward substitution, row by row."""
        V = self.ar.zeros(R.shape)
        for j in range(L.shape[0]):
            V[j] = ((R[j] - L[j, :j] @ V[:j]) if j else R[j]) / L[j, j]
        return V

    # ---- lifts --------------------------------------------------------------------------------------------------
    def ordering_lift(self, order):
        """The lift vector of one ordering, per feature, in the arithmetic of the problem."""
        o = np.asarray(order, dtype=np.intp)
        key = o.tobytes()
        if key not in self._lift_cache:          # (an antithetical sample's reverse is often another sample's ordering)
            self._lift_cache[key] = self._ordering_lift(o)
        return self._lift_cache[key]

    def _ordering_lift(self, o):
        ar, p = self.ar, self.p
        L, z, piv = self._chol_aug(self.G[np.ix_(o, o)], self.g[o])
        self.min_pivot = min(self.min_pivot, min(piv))
        if self.tri:
            R, yt, piv_t = self._chol_aug(self.H[np.ix_(o, o)], self.h[o])
            self.min_pivot_test = min(self.min_pivot_test, min(piv_t))
        else:
            R, yt = self.Ft[o, :], self.yte
        V = self._forward(L, R)
        ZV = z[:, None] * V
        N = np.cumsum(ZV, axis=0)
        lift = ar.zeros(p)
        lift[o] = z * np.sum(V * (2 * yt[None, :] - N - (N - ZV)), axis=1) / self.yy
        return lift

    def sample_lift(self, order, antithetical):
        lift = self.ordering_lift(order)
        if antithetical:
            lift = (lift + self.ordering_lift(np.asarray(order)[::-1])) / 2
        return lift

    def lifts(self, orders, antithetical, raw=False):
        out = [self.sample_lift(o, antithetical) for o in orders]
        return np.array(out, dtype=self.ar.dtype) if raw else np.array([self.ar.to_float(v) for v in out])

    # ---- values of column sets ------------------------------------------------------------------------------------
    def subset_value(self, cols):
        """R^2 of the model on the columns `cols`: (2 th.h_S - th.H_SS th) / yy with th = G_SS^-1 g_S; v({}) = 0."""
        ar = self.ar
        c = np.asarray(cols, dtype=np.intp)
        if len(c) == 0:
            return ar.zeros(1)[0]
        L, z, piv = self._chol_aug(self.G[np.ix_(c, c)], self.g[c])
        self.min_pivot = min(self.min_pivot, min(piv))
        th = ar.zeros(len(c))
        for j in range(len(c) - 1, -1, -1):           # L^T th = z
            th[j] = (z[j] - _dot(L[j + 1:, j], th[j + 1:])) / L[j, j]
        return (2 * (th @ self.h[c]) - th @ (self.H[np.ix_(c, c)] @ th)) / self.yy

    def mask_value(self, mask):
        return self.subset_value([j for j in range(self.p) if (int(mask) >> j) & 1])

    def group_value(self, mask, labels):
        """u(S): the baseline columns (label -1) and the columns of the groups in `mask` (bit k = group k)."""
        labels = np.asarray(labels)
        keep = (labels == -1) | ((labels >= 0) & (((int(mask) >> np.maximum(labels, 0)) & 1) == 1))
        return self.subset_value(np.nonzero(keep)[0])

    def shapley(self, labels=None, raw=False):
        """Brute-force Shapley values over the columns, or over the groups of `labels`, from the table of all subsets
        (p or g <= 12)."""
        ng = self.p if labels is None else int(np.max(labels)) + 1
        assert ng <= 12
        tab = [self.mask_value(m) if labels is None else self.group_value(m, labels) for m in range(1 << ng)]
        size = [bin(m).count("1") for m in range(1 << ng)]
        phi = self.ar.zeros(ng)
        for k in range(ng):
            for m in range(1 << ng):
                if not (m >> k) & 1:
                    phi[k] = phi[k] + (tab[m | 1 << k] - tab[m]) / self.ar.conv(np.float64(ng * comb(ng - 1, size[m])))
        return phi if raw else self.ar.to_float(phi)

    def to_float(self, a):
        return self.ar.to_float(a)


# ---- the same route at working precision -------------------------------------------------------------------------------
def plain_gram(X_train, X_test, y_train, y_test, reg=0.0):
    Xa, Xe, ya, ye = (np.asarray(a, dtype=np.float64) for a in (X_train, X_test, y_train, y_test))
    n, p = Xa.shape
    return Xa.T @ Xa / n + reg * np.eye(p), Xa.T @ ya / n, Xe.T @ Xe, Xe.T @ ye, float(ye @ ye)


def plain_lifts(X_train, X_test, y_train, y_test, reg, orders, antithetical, dtype=np.float64):
    """NumPy / LAPACK at `dtype`: np.linalg.cholesky, scipy.linalg.solve_triangular; for fp32 the Gram quantities are
    formed in fp64 and then rounded, and the lift scan stays fp64, as in the engine.  A factorisation LAPACK refuses
    gives a row of NaN."""
    G, g, H, h, yy = plain_gram(X_train, X_test, y_train, y_test, reg)
    Xe, ye = np.asarray(X_test, dtype=np.float64), np.asarray(y_test, dtype=np.float64)
    p, tri = len(g), Xe.shape[0] >= len(g)
    G, g, H, h, Ft = (a.astype(dtype) for a in (G, g, H, h, Xe.T))

    def one(o):
        try:
            L = np.linalg.cholesky(G[np.ix_(o, o)])
            z = sla.solve_triangular(L, g[o], lower=True)
            if tri:
                R = np.linalg.cholesky(H[np.ix_(o, o)])
                yt = sla.solve_triangular(R, h[o], lower=True).astype(np.float64)
            else:
                R, yt = Ft[o, :], ye
            V = sla.solve_triangular(L, R, lower=True).astype(np.float64)
        except (np.linalg.LinAlgError, ValueError):      # not positive definite / not finite at this precision
            return np.full(p, np.nan)
        z = z.astype(np.float64)
        ZV = z[:, None] * V
        N = np.cumsum(ZV, axis=0)
        lift = np.empty(p)
        lift[o] = z * np.sum(V * (2 * yt[None, :] - N - (N - ZV)), axis=1) / yy
        return lift

    out = []
    for o in orders:
        o = np.asarray(o, dtype=np.intp)
        out.append(0.5 * (one(o) + one(o[::-1])) if antithetical else one(o))
    return np.array(out)


# ---- data of a chosen condition number ---------------------------------------------------------------------------------
def gen(p, n, m, kappa, seed):
    """X = Z M^T with M = (Q1 diag(s)) Q2, Q1 / Q2 the Q of seeded Gaussian p x p matrices, s_k = kappa^(-k/(p-1)):
    kappa(X) ~ kappa, kappa(G) ~ 1.3 kappa^2.  y = X w + N(0, 1), w ~ N(0, I)."""
    rng = np.random.default_rng(seed)
    Q1 = np.linalg.qr(rng.standard_normal((p, p)))[0]
    Q2 = np.linalg.qr(rng.standard_normal((p, p)))[0]
    s = float(kappa) ** (-np.arange(p) / max(p - 1, 1))
    M = (Q1 * s) @ Q2
    X_tr = rng.standard_normal((n, p)) @ M.T
    X_te = rng.standard_normal((m, p)) @ M.T
    w = rng.standard_normal(p)
    return X_tr, X_te, X_tr @ w + rng.standard_normal(n), X_te @ w + rng.standard_normal(m)


def orderings(p, seed, count=3):
    """Identity, reversed and `count` seeded orderings."""
    rng = np.random.default_rng(seed)
    return np.array([np.arange(p), np.arange(p)[::-1]] + [rng.permutation(p) for _ in range(count)], dtype=np.int32)
