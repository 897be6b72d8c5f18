"""Truth of the bootstrap of the sampled attribution (ls_spa_bootstrap_sampled, lsspa_boot_lift_* of include/lsspa.h), by
tests/hp_ref.py and tests/boot_ref.py.

TESTS ONLY.  Replicate r of boot_seed is hp_ref.Problem(X_train[idx_tr], X_test[idx_te], y_train[idx_tr], y_test[idx_te],
reg) in long double with idx = boot_ref.indices(boot_seed, r, side, n): the rows drawn, in draw order (a Gram does not
depend on the order).  r < 0 is the point problem: the original rows.  plain_*: the same rows through hp_ref.plain_lifts
(NumPy / LAPACK in fp64), the yardstick of the tolerance rule."""
import numpy as np

import boot_ref
import hp_ref


def replicate_rows(data, boot_seed, r):
    """(X_train, X_test, y_train, y_test) of replicate r (r < 0: the original rows)"""
    Xa, Xe, ya, ye = (np.asarray(a, dtype=np.float64) for a in data)
    if r < 0:
        return Xa, Xe, ya, ye
    ia, ie = boot_ref.indices(boot_seed, r, 0, len(Xa)), boot_ref.indices(boot_seed, r, 1, len(Xe))
    return Xa[ia], Xe[ie], ya[ia], ye[ie]


def problem(data, boot_seed, r, reg=0.0):
    return hp_ref.Problem(*replicate_rows(data, boot_seed, r), reg)


def truth_lifts(prob, orders, antithetical):
    """[B][p]: fp64 roundings of the long-double lifts of the samples"""
    return np.asarray(prob.lifts(orders, antithetical), dtype=np.float64)


def plain_lifts(data, boot_seed, r, reg, orders, antithetical):
    return hp_ref.plain_lifts(*replicate_rows(data, boot_seed, r), reg, orders, antithetical)


def weighted_problem(data, w_train, w_test, reg=0.0):
    """(G, g, H, h, inv_yy) of the weighted problem in long double, rounded to fp64: G = sum w z z^T / sum w + reg I on
    the training side, H = sum w z z^T on the test side."""
    Xa, Xe, ya, ye = (np.asarray(a, dtype=np.longdouble) for a in data)
    wa, we = np.asarray(w_train, dtype=np.longdouble), np.asarray(w_test, dtype=np.longdouble)
    W = wa.sum()
    G = (Xa.T * wa) @ Xa / W + np.longdouble(reg) * np.eye(Xa.shape[1], dtype=np.longdouble)
    g = (Xa.T * wa) @ ya / W
    H = (Xe.T * we) @ Xe
    h = (Xe.T * we) @ ye
    yy = (we * ye) @ ye
    return tuple(np.asarray(a, dtype=np.float64) for a in (G, g, H, h)) + (float(1 / yy),)


def group_fold(lifts, labels):
    """[..., g] from column lifts [..., p]: group k's columns added in ascending column order from 0.0 (the device's)."""
    labels = np.asarray(labels)
    g = int(labels.max()) + 1
    out = np.zeros(lifts.shape[:-1] + (g,), dtype=lifts.dtype)
    for k in range(g):
        acc = np.zeros(lifts.shape[:-1], dtype=lifts.dtype)
        for c in np.nonzero(labels == k)[0]:
            acc = acc + lifts[..., c]
        out[..., k] = acc
    return out


def welford(samples, cut):
    """(mean, M2) of samples [n][d] by the device's rule: Welford in sample order inside each launch of `cut` samples,
    one Chan merge per launch into the running state."""
    n, d = samples.shape
    mean, m2, done = np.zeros(d), np.zeros(d), 0
    for s0 in range(0, n, cut):
        blk = samples[s0:s0 + cut]
        mb, qb = np.zeros(d), np.zeros(d)
        for s, x in enumerate(blk):
            dl = x - mb
            mb = mb + dl / float(s + 1)
            qb = qb + dl * (x - mb)
        if done == 0:
            mean, m2 = mb, qb
        else:
            nb, tot = float(len(blk)), float(done + len(blk))
            dl = mb - mean
            mean = mean + dl * (nb / tot)
            m2 = m2 + (qb + dl * dl * (done * nb / tot))
        done += len(blk)
    return mean, m2
