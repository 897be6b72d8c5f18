"""ls_spa_best_group_subsets_bootstrap against the loop a user wrote before it existed, and its enumeration against the
one-problem kernel, in one process on one MI355X:

    python tools/group_best_bootstrap_time.py [--loop-reps K] [--repeats 5]

(a) (N = M, p, g, R) = (1e4, 40, 8, 1000), (1e5, 64, 12, 1000), (1e5, 60, 20, 200), the columns dealt evenly over the
    groups (p = 64, g = 12: four baseline columns).  Per shape, medians of `repeats` alternating repeats of the whole
    call and of the loop of ls_spa_best_subsets(groups=) on np.take-n host rows; the loop is timed over its first
    min(R, K) replicates (default 20) and SCALED to R: every call of it costs the same.  ratio = call / loop.
(b) (g, p) = (8, 40), (12, 64), (16, 48), (20, 60) (N = M = 2000): the enumeration share of a run (lsspa_boot_timing)
    divided by its replicates, against the kernel time of lsspa_groups_best on one replicate's reduced problem
    (lsspa_groups_timing), medians of `repeats` alternating repeats.  The gate is ratio <= 1.05 at g = 16 and 20.
One JSON line per shape."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ls-spa_amd"))

from ls_spa import ls_spa_best_group_subsets_bootstrap, ls_spa_best_subsets     # noqa: E402
from ls_spa._engine import HipEngine                                            # noqa: E402

SHAPES = [(10 ** 4, 40, 8, 1000), (10 ** 5, 64, 12, 1000), (10 ** 5, 60, 20, 200)]
ENUM_SHAPES = [(8, 40, 1000), (12, 64, 400), (16, 48, 60), (20, 60, 16)]


def labels_of(p, g):
    """p columns dealt evenly over g groups; what is left over is the baseline."""
    each = p // g
    return np.concatenate([np.full(p - each * g, -1), np.repeat(np.arange(g), each)]).astype(np.int64)


def make(n, p, seed):
    rng = np.random.default_rng(seed)
    Xa, Xe = rng.standard_normal((n, p)), rng.standard_normal((n, p))
    w = rng.standard_normal(p)
    return Xa, Xe, Xa @ w + rng.standard_normal(n), Xe @ w + rng.standard_normal(n)


def whole_call(eng, args):
    for n, p, g, R in SHAPES:
        d, labels = make(n, p, p), labels_of(p, g)
        ls_spa_best_group_subsets_bootstrap(*d, labels, n_boot=8, _engine=eng)     # warm-up: allocations, first launches
        ls_spa_best_subsets(*d, groups=labels, _engine=eng)
        k = min(max(args.loop_reps, 1), R, 20)
        call, loop, parts = [], [], None
        for rep in range(args.repeats):
            t0 = time.perf_counter()
            res = ls_spa_best_group_subsets_bootstrap(*d, labels, n_boot=R, seed=1, _engine=eng)
            call.append(time.perf_counter() - t0)
            parts = eng.boot_timing_last             # left by boot_free at the end of the call: the run's kernel shares
            rng = np.random.default_rng(rep)
            t0 = time.perf_counter()
            for _ in range(k):
                ia, ie = rng.integers(0, n, n), rng.integers(0, n, n)
                ls_spa_best_subsets(np.take(d[0], ia, axis=0), np.take(d[1], ie, axis=0), d[2][ia], d[3][ie],
                                    groups=labels, _engine=eng)
            loop.append((time.perf_counter() - t0) / k * R)
        c, l = float(np.median(call)), float(np.median(loop))
        print(json.dumps({"what": "whole call", "N": n, "p": p, "g": g, "R": R, "bootstrap_s": round(c, 4),
                          "kernel_s": parts, "loop_s_scaled": round(l, 3), "loop_reps_timed": k,
                          "ratio": round(c / l, 4), "n_failed": res.n_failed, "best_size": res.best_size,
                          "best_size_frequency": float(res.best_size_frequency.max())}), flush=True)


def enumeration(eng, args):
    other = HipEngine(0)
    for g, p, R in ENUM_SHAPES:
        n = 2000
        d, labels = make(n, p, 100 + p), labels_of(p, g)
        eng.boot_load(*d, 0.0, grouped=True)
        Sa, Se, W = eng.boot_debug_grams(1, np.ones((1, n)), np.ones((1, n)))
        G, gv = Sa[0, :p, :p] / W[0], Sa[0, :p, p] / W[0]
        other.load_reduced(G, gv, float(gv @ np.linalg.solve(G, gv)) * 1.01 + 1.0, Se[0, p, p], H=Se[0, :p, :p],
                           h=Se[0, :p, p])
        eng.boot_groups_best_run(labels, R, 1)
        other.groups_best(labels)
        boot, one = [], []
        for _ in range(args.repeats):
            eng.boot_groups_best_run(labels, R, 1)
            boot.append(eng.boot_timing()["enumeration"] / R)
            other.groups_best(labels)
            one.append(other.groups_timing()[0])
        b, o = float(np.median(boot)), float(np.median(one))
        print(json.dumps({"what": "enumeration per replicate", "g": g, "p": p, "R": R, "boot_ms": round(1e3 * b, 5),
                          "one_problem_ms": round(1e3 * o, 5), "ratio": round(b / o, 4)}), flush=True)
        eng.boot_free()
    other.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loop-reps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--only", choices=("enumeration", "whole"), default=None)
    args = ap.parse_args()
    eng = HipEngine(0)
    if args.only != "whole":
        enumeration(eng, args)
    if args.only != "enumeration":
        whole_call(eng, args)
    eng.close()


if __name__ == "__main__":
    main()
