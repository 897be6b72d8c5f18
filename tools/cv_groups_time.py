"""Timing of ls_spa_best_subsets_cv(groups=) on the GPU: N = 10^4 rows, K = 5 folds, (g, p) = (12, 64), (16, 48),
(20, 60).

    python tools/cv_groups_time.py [--cases 12x64 16x48 20x60] [--json out.json]

Per case it prints
  * the whole ls_spa_best_subsets_cv(groups=) call (host seconds, engine kept);
  * (i)  the device time of the grouped CV enumeration (lsspa_cv_timing) against K x the device time of
         lsspa_groups_best on one fold problem in the same process -- the cost of restaging h and diag G K times a step;
  * (ii) the whole call against the only route there was before: lsspa_debug_group_values over all 2^g masks, once per
         fold problem loaded with load_reduced, then the host's sum over the folds and arg-max per size.  Must be < 1
         at g = 16 and 20, both routes returning the same winners and bits.
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
from cv_time import data, load_fold, popcount               # noqa: E402


def labels_of(g, p):
    """g groups of p // g columns each; what is left over is the baseline"""
    size = p // g
    return np.concatenate([np.full(p - g * size, -1), np.repeat(np.arange(g), size)]).astype(np.int32)


def prior_route(engine, probs, labels, g):
    """debug_group_values over all masks per fold, the host's sum and arg-max per size (smaller mask on ties)"""
    masks = np.arange(1 << g, dtype=np.uint64)
    total = None
    for prob in probs:
        load_fold(engine, prob)
        u = engine.debug_group_values(labels, masks)
        total = u if total is None else total + u
    size = popcount(masks)
    best, win = np.full(g + 1, np.nan), np.zeros(g + 1, dtype=np.uint32)
    for k in range(g + 1):
        sel = np.nonzero(size == k)[0]
        i = sel[np.argmax(total[sel])]          # the first of equal maxima: the smaller mask
        best[k], win[k] = total[i], i
    return best, win


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["12x64", "16x48", "20x60"], help="g x p")
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--folds", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    engine = HipEngine(0)
    rows = []
    for case in a.cases:
        g, p = (int(t) for t in case.split("x"))
        labels = labels_of(g, p)
        X, y = data(p, a.n, seed=p + g)
        K = a.folds
        ids, _ = cv_fold_ids(a.n, K)
        ls_spa_best_subsets_cv(X, y, folds=K, groups=labels, _engine=engine)      # warm
        t0 = time.perf_counter()
        res = ls_spa_best_subsets_cv(X, y, folds=K, groups=labels, _engine=engine)
        whole = time.perf_counter() - t0
        engine.cv_groups_load(X, y, ids, K, 0.0)
        u, masks, found, _, _ = engine.cv_groups_best(labels)
        tm = engine.cv_timing()
        probs = [engine.cv_get_problem(f) for f in range(K)]
        engine.cv_free()
        load_fold(engine, probs[0])
        engine.groups_best(labels)
        engine.groups_best(labels)
        one = engine.groups_timing()
        one_s = one["kernel"] if isinstance(one, dict) else one[0]
        t0 = time.perf_counter()
        best, win = prior_route(engine, probs, labels, g)
        prior = time.perf_counter() - t0
        assert np.array_equal(win, masks) and np.array_equal(best, u), "the two routes disagree"
        row = dict(g=g, p=p, n=a.n, folds=K, whole_call_s=whole, gram_s=tm["gram"], cv_enum_s=tm["enumeration"],
                   launches=tm["launches"], one_problem_best_s=one_s, enum_ratio=tm["enumeration"] / (K * one_s),
                   prior_route_s=prior, whole_over_prior=whole / prior, best_size=res.best_size)
        rows.append(row)
        print(json.dumps(row), flush=True)
        if g >= 16:
            assert whole < prior, "the call must beat the route through debug values"
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
