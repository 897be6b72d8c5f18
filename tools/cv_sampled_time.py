"""Time the sampled K-fold CV attribution (ls_spa_cv_sampled) on one GPU (developer tool).

    python tools/cv_sampled_time.py [--json out.json]

N = 10^4 rows, 256 antithetical samples a batch, medians of REPS repeats after a warm-up, each step alone in its process.
Shapes (p, K) = (40, 5), (100, 5), (120, 5), (40, 10).
1. The device time of a batch's lift launch (lsspa_cv_lift_timing) against K times the device time of lsspa_lift_batch's
   kernels (the profile's class of the fused small-problem kernel) on ONE fold problem with the same orderings, in the
   same process.  The work and the kernel body are the same: the ratio must stay at or below LIMIT at (40, 5) and
   (100, 5); the other shapes and the fold + statistics launches are reported.
2. The whole call against the route there was before: ls_spa_cv_sampled(perms=) beside K calls of ls_spa(perms=) on the
   folds' splits with the same orderings, both on a kept engine.  The ratio must be below 1 at every shape.
Every (section, shape) runs as a child process under a time limit of its own; the first one that fails ends the run.
Exit status 1 if a required ratio fails, 2 if a step failed."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ls-spa_amd"))

REPS = 7
LIMIT = 1.05
N, BATCH = 10000, 256
SHAPES = ((40, 5), (100, 5), (120, 5), (40, 10))
GATED = ((40, 5), (100, 5))
STEP_SECONDS = {"call": 300, "device": 180}


def setup(p, K):
    import numpy as np
    rng = np.random.default_rng(p + K)
    X = rng.standard_normal((N, p)) + 0.3 * rng.standard_normal((N, 1))
    beta = np.where(np.arange(p) % 3 == 0, 1.0 + 0.37 * np.arange(p), 0.05 * (1 + np.arange(p) % 5))
    y = X @ beta + 0.5 * rng.standard_normal(N)
    perms = np.array([rng.permutation(p) for _ in range(BATCH)], dtype=np.int32)
    return X, y, perms


def device_step(p, K):
    from ls_spa import cv_fold_ids
    from ls_spa._engine import HipEngine
    eng = HipEngine(0)
    X, y, perms = setup(p, K)
    ids, _ = cv_fold_ids(N, K)
    eng.cv_lift_load(X, y, ids, K, 0.0)
    eng.load_data(X[ids != 0], X[ids == 0], y[ids != 0], y[ids == 0], 0.0)
    eng.cv_lift_batch(perms, True, accumulate=True)
    eng.run_batch(perms, True, accumulate=False)
    cv_ms, rest_ms, one_ms = [], [], []
    eng.profile(True)
    for _ in range(REPS):
        eng.cv_lift_batch(perms, True, accumulate=True)
        t = eng.cv_lift_timing()
        cv_ms.append(t["batch"] * 1e3)
        rest_ms.append(t["stats"] * 1e3)
        eng.profile_reset()
        eng.run_batch(perms, True, accumulate=False)
        one_ms.append(eng.profile_read()["small_p"][0])
    info = eng.cv_lift_info()
    eng.cv_lift_free()
    eng.close()
    a, b = statistics.median(cv_ms), K * statistics.median(one_ms)
    print(json.dumps(dict(step="device", p=p, K=K, lift_ms=a, k_one_ms=b, ratio=a / b,
                          fold_stats_ms=statistics.median(rest_ms), not_pd=bool(info.any()))), flush=True)


def call_step(p, K):
    import warnings
    from ls_spa import cv_fold_ids, ls_spa, ls_spa_cv_sampled
    from ls_spa._engine import HipEngine
    eng = HipEngine(0)
    X, y, perms = setup(p, K)
    ids, _ = cv_fold_ids(N, K)

    def new():
        return ls_spa_cv_sampled(X, y, 0.0, ids, perms=perms, batch_size=BATCH, _engine=eng)

    def old():
        total = 0.0
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for f in range(K):
                tr, te = ids != f, ids == f
                r = ls_spa(X[tr], X[te], y[tr], y[te], perms=perms, batch_size=BATCH, tolerance=0.0, _engine=eng)
                total = total + r.attribution * (float(y[te] @ y[te]) / float(y @ y))
        return total

    new()
    old()
    new_s, old_s = [], []
    for _ in range(REPS):
        t = time.perf_counter()
        new()
        new_s.append(time.perf_counter() - t)
        t = time.perf_counter()
        old()
        old_s.append(time.perf_counter() - t)
    eng.close()
    a, b = statistics.median(new_s), statistics.median(old_s)
    print(json.dumps(dict(step="call", p=p, K=K, new_s=a, old_s=b, ratio=a / b)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEP_SECONDS), default=None, help="(internal) run one step in this process")
    ap.add_argument("--p", type=int, default=None)
    ap.add_argument("--K", type=int, default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.step:
        (call_step if a.step == "call" else device_step)(a.p, a.K)
        return 0
    rows = []
    for step in ("device", "call"):
        for p, K in SHAPES:
            cmd = ["timeout", "-k", "10", str(STEP_SECONDS[step]), sys.executable, os.path.abspath(__file__), "--step", step,
                   "--p", str(p), "--K", str(K)]
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            sys.stdout.write(r.stdout)
            sys.stdout.flush()
            rows += [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
            if r.returncode != 0:
                print(f"step {step} p = {p} K = {K} ended with status {r.returncode}: nothing more is started", flush=True)
                return 2
    ok = True
    print(f"{'p':>3} {'K':>3} {'lift ms':>9} {'K x one ms':>10} {'ratio':>6} {'fold+stats ms':>13}")
    for r in (r for r in rows if r["step"] == "device"):
        gated = (r["p"], r["K"]) in GATED
        ok = ok and (not gated or r["lift_ms"] <= LIMIT * r["k_one_ms"])
        print(f"{r['p']:>3} {r['K']:>3} {r['lift_ms']:>9.3f} {r['k_one_ms']:>10.3f} {r['ratio']:>6.3f} "
              f"{r['fold_stats_ms']:>13.3f}" + (f"  (gated <= {LIMIT})" if gated else "") + ("  NOT_PD" if r["not_pd"] else ""))
    print(f"{'p':>3} {'K':>3} {'ls_spa_cv_sampled s':>19} {'K x ls_spa s':>12} {'ratio':>6}")
    for r in (r for r in rows if r["step"] == "call"):
        ok = ok and r["new_s"] < r["old_s"]
        print(f"{r['p']:>3} {r['K']:>3} {r['new_s']:>19.4f} {r['old_s']:>12.4f} {r['ratio']:>6.3f}  (required < 1)")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
