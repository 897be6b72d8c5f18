"""Timing of ls_spa_multi(groups=) against a loop of ls_spa(method='subsets', groups=) calls, on one MI355X, alone in
the process:

    python tools/multi_groups_time.py [--json out.json]

Per (g, p, m): the whole call of ls_spa_multi(groups=) against the loop of m one-response calls on the same arrays (the
loop is timed over min(m, 20) calls and scaled), and the enumeration's device time per response (lsspa_multi_timing)
against the device time of the one-response grouped enumeration (lsspa_groups_timing) in the same process: `ratio` is
the former over the latter, below 1 where carrying eight responses through one elimination pays."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ls-spa_amd"))

from ls_spa import ls_spa, ls_spa_multi          # noqa: E402
from ls_spa._engine import HipEngine             # noqa: E402

MIXED20 = [1, 2, 3, 4, 4, 3, 2, 1, 4, 4, 3, 3, 2, 4, 4, 1, 4, 4, 3, 4]      # 20 groups, 60 columns
# (g, p) -> group sizes and baseline columns
LAYOUTS = {(12, 64): ([5] * 12, 4), (16, 48): ([3] * 16, 0), (20, 60): (MIXED20, 0)}
CASES = [(12, 64, 64), (16, 48, 64), (20, 60, 8), (20, 60, 64)]


def labels_of(g, p):
    sizes, nb = LAYOUTS[(g, p)]
    lab = np.concatenate([np.full(nb, -1)] + [np.full(s, k) for k, s in enumerate(sizes)]).astype(np.int64)
    assert len(lab) == p and len(sizes) == g
    np.random.default_rng(g).shuffle(lab)
    return lab


def problem(p, m, n=4000, rows=2000, seed=0):
    rng = np.random.default_rng(seed + p)
    Xa, Xe = rng.standard_normal((n, p)), rng.standard_normal((rows, p))
    W = rng.standard_normal((p, m))
    return Xa, Xe, Xa @ W + rng.standard_normal((n, m)), Xe @ W + rng.standard_normal((rows, m))


def best(fn, reps=3):
    out = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t)
    return min(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--cases", default=None, help="g:p:m,g:p:m,... instead of the default list")
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    cases = [tuple(int(v) for v in c.split(":")) for c in a.cases.split(",")] if a.cases else CASES
    eng = HipEngine(0)
    rows = []
    for g, p, m in cases:
        labels = labels_of(g, p)
        Xa, Xe, Ya, Ye = problem(p, m)
        one = lambda r: ls_spa(Xa, Xe, Ya[:, r], Ye[:, r], method="subsets", groups=labels, _engine=eng)   # noqa: E731
        ls_spa_multi(Xa, Xe, Ya[:, :1], Ye[:, :1], groups=labels, _engine=eng)          # warm-up of both paths
        one(0)
        call_multi = best(lambda: ls_spa_multi(Xa, Xe, Ya, Ye, groups=labels, _engine=eng), a.reps)
        eng.multi_load(Xa, Xe, Ya, Ye, 0.0)
        enum = []
        for _ in range(a.reps):
            eng.multi_groups_shapley(labels)
            enum.append(eng.multi_timing())
        tm = min(enum, key=lambda t: t["enumeration"])
        eng.multi_free()
        k = min(m, 20)
        kernel_one = []

        def loop():
            for r in range(k):
                one(r)
                kernel_one.append(eng.groups_timing()[0])
        call_loop = best(loop, a.reps) * m / k
        k1 = float(np.median(kernel_one))
        row = {"g": g, "p": p, "m": m, "call_multi_ms": 1e3 * call_multi, "call_loop_ms": 1e3 * call_loop,
               "call_ratio": call_loop / call_multi, "enum_multi_ms": 1e3 * tm["enumeration"],
               "enum_multi_per_response_ms": 1e3 * tm["enumeration"] / m, "kernel_one_ms": 1e3 * k1,
               "ratio": tm["enumeration"] / m / k1, "gram_ms": 1e3 * tm["gram"],
               "max_launch_ms": 1e3 * tm["max_launch"], "launches": tm["launches"]}
        rows.append(row)
        print(json.dumps(row), flush=True)
    eng.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
