"""Timing of ls_spa_multi against a loop of ls_spa(method='subsets') calls, on one MI355X, alone in the process:

    python tools/multi_time.py [--json out.json]

Per (p, m): the whole call of ls_spa_multi against the loop of m one-response calls on the same arrays (the loop is
timed over min(m, 20) calls and scaled), and the enumeration's device time (lsspa_multi_timing) against m times the
device time of the one-response enumeration (lsspa_subsets_timing) in the same process."""
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

RB = HipEngine.MULTI_RB
CASES = [(16, 64), (20, 64), (24, RB), (24, 64), (28, RB)]


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
    ap.add_argument("--cases", default=None, help="p:m,p:m,... instead of the default list")
    a = ap.parse_args()
    cases = [tuple(int(v) for v in c.split(":")) for c in a.cases.split(",")] if a.cases else CASES
    eng = HipEngine(0)
    rows = []
    for p, m in cases:
        Xa, Xe, Ya, Ye = problem(p, m)
        ls_spa_multi(Xa, Xe, Ya[:, :1], Ye[:, :1], _engine=eng)            # warm-up of both paths
        ls_spa(Xa, Xe, Ya[:, 0], Ye[:, 0], method="subsets", _engine=eng)
        reps = 3 if p <= 24 else 1
        call_multi = best(lambda: ls_spa_multi(Xa, Xe, Ya, Ye, _engine=eng), reps)
        eng.multi_load(Xa, Xe, Ya, Ye, 0.0)
        eng.multi_shapley()
        tm = eng.multi_timing()
        eng.multi_free()
        k = min(m, 20)
        call_loop = best(lambda: [ls_spa(Xa, Xe, Ya[:, r], Ye[:, r], method="subsets", _engine=eng) for r in range(k)],
                         reps) * m / k
        kernel_one = eng.subsets_timing()[0]
        row = {"p": p, "m": m, "call_multi_ms": 1e3 * call_multi, "call_loop_ms": 1e3 * call_loop,
               "call_ratio": call_loop / call_multi, "enum_multi_ms": 1e3 * tm["enumeration"],
               "enum_loop_ms": 1e3 * kernel_one * m, "enum_ratio": kernel_one * m / tm["enumeration"],
               "enum_multi_per_response_ms": 1e3 * tm["enumeration"] / m, "kernel_one_ms": 1e3 * kernel_one,
               "gram_ms": 1e3 * tm["gram"], "max_launch_ms": 1e3 * tm["max_launch"], "launches": tm["launches"]}
        rows.append(row)
        print(json.dumps(row), flush=True)
    eng.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
