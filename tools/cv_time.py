"""Timing of ls_spa_best_subsets_cv on the GPU: N = 10^4 rows, K = 5 folds, p = 16, 20, 24.

    python tools/cv_time.py [--p 16 20 24] [--json out.json]

Per p it prints
  * the whole ls_spa_best_subsets_cv call (host seconds, engine kept);
  * (i)  the device time of the CV enumeration (lsspa_cv_timing) against K x the device time of lsspa_subsets_best on
         one fold problem in the same process -- the cost of switching the test-side matrix K times a step;
  * (ii) the whole call against the only route there was before: lsspa_debug_subset_values over all 2^p masks, once per
         fold problem on a loaded engine, then the host's sum over the folds and arg-max per size.  Must be < 1.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ls-spa_amd"))

from ls_spa import cv_fold_ids, ls_spa_best_subsets_cv      # noqa: E402
from ls_spa._engine import HipEngine                        # noqa: E402


def data(p, n, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, p)) + 0.3 * rng.standard_normal((n, 1))
    beta = np.where(np.arange(p) % 3 == 0, 1.0 + 0.37 * np.arange(p), 0.05 * (1 + np.arange(p) % 5))
    return X, X @ beta + 0.5 * rng.standard_normal(n)


def load_fold(engine, prob):
    G, g, H, h, inv_yy = prob
    yy = 1.0 / inv_yy
    for _ in range(8):
        if 1.0 / yy == inv_yy:
            break
        yy = np.nextafter(yy, np.inf if 1.0 / yy > inv_yy else -np.inf)
    engine.load_reduced(G, g, float(g @ np.linalg.solve(G, g)) * (1 + 1e-9), yy, H=H, h=h)


def popcount(m):
    m = m.astype(np.uint64)
    c = np.zeros(len(m), dtype=np.int64)
    for s in range(0, 32, 8):
        c += np.unpackbits(((m >> np.uint64(s)) & np.uint64(255)).astype(np.uint8)[:, None], axis=1).sum(axis=1, dtype=np.int64)
    return c


def prior_route(engine, probs, p):
    """debug_subset_values over all masks per fold, the host's sum and arg-max per size (smaller mask on ties)"""
    masks = np.arange(1 << p, dtype=np.uint64)
    total = None
    for prob in probs:
        load_fold(engine, prob)
        v = engine.debug_subset_values(masks)
        total = v if total is None else total + v
    size = popcount(masks)
    best, win = np.full(p + 1, np.nan), np.zeros(p + 1, dtype=np.uint32)
    for k in range(p + 1):
        sel = np.nonzero(size == k)[0]
        i = sel[np.argmax(total[sel])]          # the first of equal maxima: the smaller mask
        best[k], win[k] = total[i], i
    return best, win


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--p", type=int, nargs="+", default=[16, 20, 24])
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--folds", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    engine = HipEngine(0)
    rows = []
    for p in a.p:
        X, y = data(p, a.n, seed=p)
        K = a.folds
        ids, _ = cv_fold_ids(a.n, K)
        ls_spa_best_subsets_cv(X, y, folds=K, _engine=engine)                  # warm
        t0 = time.perf_counter()
        res = ls_spa_best_subsets_cv(X, y, folds=K, _engine=engine)
        whole = time.perf_counter() - t0
        engine.cv_load(X, y, ids, K, 0.0)
        v, masks, found, _, _ = engine.cv_best()
        tm = engine.cv_timing()
        probs = [engine.cv_get_problem(f) for f in range(K)]
        engine.cv_free()
        load_fold(engine, probs[0])
        engine.subsets_best()
        engine.subsets_best()
        one = engine.subsets_timing()
        one_s = one["kernel"] if isinstance(one, dict) else one[0]
        t0 = time.perf_counter()
        best, win = prior_route(engine, probs, p)
        prior = time.perf_counter() - t0
        assert np.array_equal(win, masks) and np.array_equal(best, v), "the two routes disagree"
        row = dict(p=p, n=a.n, folds=K, whole_call_s=whole, gram_s=tm["gram"], cv_enum_s=tm["enumeration"],
                   launches=tm["launches"], one_problem_best_s=one_s, enum_ratio=tm["enumeration"] / (K * one_s),
                   prior_route_s=prior, whole_over_prior=whole / prior, best_size=res.best_size)
        rows.append(row)
        print(json.dumps(row), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
