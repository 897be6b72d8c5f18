"""Timing of ls_spa_multi_sampled against the one-response path, on one MI355X, alone in the process:

    python tools/multi_sampled_time.py [--json out.json]

Per (p, m), N = M = 10^4, batches of 256 antithetical samples: the load (the two Gram passes, lsspa_multi_lift_timing),
the device time of a batch's lift launches (lsspa_multi_lift_timing) and of its statistics launch, and in the same process
the device time of lsspa_lift_batch's kernels on ONE response at the same p and batch (lsspa_profile_get):
`ratio` is the batch time per response over the one-response batch time -- below 1 where carrying eight responses
through one pair of factorisations pays.  Each is measured `reps` times after a warm-up; the median is reported with the
spread (max - min) / median.  Then the whole call of ls_spa_multi_sampled against the loop of m ls_spa calls with the same
perms (the loop is timed over min(m, 20) calls and scaled)."""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ls-spa_amd"))

from ls_spa import ls_spa, ls_spa_multi_sampled          # noqa: E402
from ls_spa._engine import HipEngine                     # noqa: E402

CASES = [(40, 8), (40, 64), (100, 8), (100, 64)]
BATCH = 256


def problem(p, m, n=10000, rows=10000, seed=0):
    rng = np.random.default_rng(seed + p)
    Xa, Xe = rng.standard_normal((n, p)), rng.standard_normal((rows, p))
    W = rng.standard_normal((p, m)) / np.sqrt(p)
    return Xa, Xe, Xa @ W + rng.standard_normal((n, m)), Xe @ W + rng.standard_normal((rows, m))


def med_spread(v):
    v = np.asarray(v, dtype=np.float64)
    md = float(np.median(v))
    return md, float((v.max() - v.min()) / md) if md > 0 else 0.0


def one_response_batch_ms(eng, perms, reps):
    """Device ms of the kernels of lsspa_lift_batch (antithetical, no statistics) on the loaded one-response problem,
    from the library's own event profile (every kernel class that ran: at these p the fused small-problem kernel)."""
    out = []
    eng.profile(True)
    for i in range(reps + 2):
        eng.profile_reset()
        eng.run_batch(perms, True, want_lifts=False, accumulate=False)
        ms = sum(v[0] for v in eng.profile_read().values())
        if i >= 2:
            out.append(ms)
    eng.profile(False)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--cases", default=None, help="p:m,p:m,... instead of the default list")
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    cases = [tuple(int(v) for v in c.split(":")) for c in a.cases.split(",")] if a.cases else CASES
    eng = HipEngine(0)
    rows = []
    for p, m in cases:
        Xa, Xe, Ya, Ye = problem(p, m)
        rng = np.random.default_rng(p)
        perms = np.array([rng.permutation(p) for _ in range(BATCH)], dtype=np.int32)
        # this family: load, then batches (two warm-ups)
        gram = []
        for _ in range(3):
            eng.multi_lift_load(Xa, Xe, Ya, Ye, 0.0)
            gram.append(1e3 * eng.multi_lift_timing()["gram"])
        batch, stats = [], []
        for i in range(a.reps + 2):
            eng.multi_lift_batch(perms, True, want_lifts=False, accumulate=True)
            t = eng.multi_lift_timing()
            if i >= 2:
                batch.append(1e3 * t["batch"])
                stats.append(1e3 * t["stats"])
        eng.multi_lift_free()
        # the one-response path beside it: the same p and batch
        eng.load_data(Xa, Xe, Ya[:, 0], Ye[:, 0], 0.0)
        eng.full_fit()
        one = one_response_batch_ms(eng, perms, a.reps)
        b_md, b_sp = med_spread(batch)
        o_md, o_sp = med_spread(one)
        # whole calls
        kw = dict(perms=perms, antithetical=True)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            ls_spa_multi_sampled(Xa, Xe, Ya[:, :1], Ye[:, :1], _engine=eng, **kw)      # warm-up of both paths
            ls_spa(Xa, Xe, Ya[:, 0], Ye[:, 0], tolerance=0.0, _engine=eng, **kw)
            calls = []
            for _ in range(3):
                t = time.perf_counter()
                ls_spa_multi_sampled(Xa, Xe, Ya, Ye, _engine=eng, **kw)
                calls.append(time.perf_counter() - t)
            k = min(m, 20)
            loops = []
            for _ in range(3):
                t = time.perf_counter()
                for r in range(k):
                    ls_spa(Xa, Xe, Ya[:, r], Ye[:, r], tolerance=0.0, _engine=eng, **kw)
                loops.append((time.perf_counter() - t) * m / k)
        row = {"p": p, "m": m, "batch": BATCH, "load_ms": float(np.median(gram)), "batch_ms": b_md, "batch_spread": b_sp,
               "batch_per_response_ms": b_md / m, "stats_ms": float(np.median(stats)), "one_response_batch_ms": o_md,
               "one_response_spread": o_sp, "ratio": b_md / m / o_md, "call_multi_ms": 1e3 * min(calls),
               "call_loop_ms": 1e3 * min(loops), "call_ratio": min(loops) / min(calls)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    eng.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
