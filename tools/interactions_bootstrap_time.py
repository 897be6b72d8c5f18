"""ls_spa_interactions_bootstrap against the loop a user wrote before it existed, in one process on one MI355X:

    python tools/interactions_bootstrap_time.py [--loop-reps K]

Features, (N = M, p, R) = (1e4, 12, 1000), (1e5, 16, 1000), (1e5, 24, 100); groups, (N = M, p, g, R) = (1e4, 40, 8, 1000),
(1e5, 64, 12, 1000).  Per shape: the whole call, the kernel seconds of its three parts (counts, Gram, enumeration;
lsspa_boot_timing) and R calls of ls_spa_interactions on np.take-n host rows.  The loop is timed over its first K
replicates (default 20, at least 20) and SCALED to R: every call of it costs the same.  One JSON line per shape."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ls-spa_amd"))

from ls_spa import ls_spa_interactions, ls_spa_interactions_bootstrap          # noqa: E402
from ls_spa._engine import HipEngine                                            # noqa: E402

SHAPES = [(10 ** 4, 12, None, 1000), (10 ** 5, 16, None, 1000), (10 ** 5, 24, None, 100),
          (10 ** 4, 40, 8, 1000), (10 ** 5, 64, 12, 1000)]


def make(n, p, seed):
    rng = np.random.default_rng(seed)
    Xa, Xe = rng.standard_normal((n, p)), rng.standard_normal((n, p))
    w = rng.standard_normal(p)
    return Xa, Xe, Xa @ w + rng.standard_normal(n), Xe @ w + rng.standard_normal(n)


def labels_of(p, g):
    """g groups of p // g or p // g + 1 neighbouring columns, no baseline."""
    return np.repeat(np.arange(g), [p // g + (k < p % g) for k in range(g)]).astype(np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loop-reps", type=int, default=20)
    args = ap.parse_args()
    eng = HipEngine(0)
    for n, p, g, R in SHAPES:
        d = make(n, p, p + (g or 0))
        labels = None if g is None else labels_of(p, g)
        ls_spa_interactions_bootstrap(*d, n_boot=8, groups=labels, _engine=eng)     # warm-up: allocations, first launches
        t0 = time.perf_counter()
        res = ls_spa_interactions_bootstrap(*d, n_boot=R, seed=1, groups=labels, _engine=eng)
        whole = time.perf_counter() - t0
        parts = eng.boot_timing_last                 # left by boot_free at the end of the call: the run's kernel shares
        assert all(parts[k] > 0 for k in ("counts", "gram", "enumeration")), parts
        rng = np.random.default_rng(0)
        k = min(max(args.loop_reps, 20), R)
        ls_spa_interactions(*d, groups=labels, _engine=eng)
        t0 = time.perf_counter()
        for _ in range(k):
            ia, ie = rng.integers(0, n, n), rng.integers(0, n, n)
            ls_spa_interactions(np.take(d[0], ia, axis=0), np.take(d[1], ie, axis=0), d[2][ia], d[3][ie], groups=labels,
                                _engine=eng)
        loop = (time.perf_counter() - t0) / k * R
        off = ~np.eye(len(res.attribution), dtype=bool)
        print(json.dumps({"N": n, "p": p, "g": g, "R": R, "bootstrap_s": round(whole, 4), "kernel_s": parts,
                          "loop_s_scaled": round(loop, 3), "loop_reps_timed": k, "speedup": round(loop / whole, 2),
                          "n_failed": res.n_failed, "mean_std_error_off_diagonal": float(res.std_error[off].mean())}),
              flush=True)
    eng.close()


if __name__ == "__main__":
    main()
