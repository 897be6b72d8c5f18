"""Time the ridge path of the K-fold CV attribution (ls_spa_cv_path) on one GPU (developer tool).

    python tools/cv_path_time.py [--json out.json]

N = 10^4 rows, K = 5 folds, L = 32 ridge values (1e-4 .. 10, geometric), kept engine, medians of REPS alternating
repeats.  Shapes: p = 12, 16, 20 columns and (g, p) = (12, 64), (16, 48) groups of columns.
1. The whole call against the loop it replaces: ls_spa_cv_path(X, y, regs) beside L calls of ls_spa_cv(X, y, reg=r),
   both on the kept engine, both with their host refits.  The ratio must be below 1 at every shape.
2. The device time of the path's enumeration launches (lsspa_cv_timing after lsspa_cv_path_shapley /
   lsspa_cv_path_groups_shapley) against L times that of lsspa_cv_shapley / lsspa_cv_groups_shapley on the same loaded
   folds, in the same process.  At p = 20 and (16, 48) a problem fills the device on its own and the path is the same
   work through the same kernel: the ratio must stay at or below LIMIT.  Below those shapes it is reported: there the
   L K problems share grids that one call's K problems leave mostly empty.
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

REPS = 5
LIMIT = 1.05
N, FOLDS, NREGS = 10000, 5, 32
SHAPES = ((0, 12), (0, 16), (0, 20), (12, 64), (16, 48))      # (g, p); g = 0: the columns are the players
GATED = ((0, 20), (16, 48))
STEP_SECONDS = {"call": 300, "device": 180}


def data(p, n, seed):
    import numpy as np
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, p)) + 0.3 * rng.standard_normal((n, 1))
    beta = np.where(np.arange(p) % 3 == 0, 1.0 + 0.37 * np.arange(p), 0.05 * (1 + np.arange(p) % 5))
    return X, X @ beta + 0.5 * rng.standard_normal(n)


def setup(g, p):
    import numpy as np
    X, y = data(p, N, seed=p + g)
    regs = np.geomspace(1e-4, 10.0, NREGS)
    labels = (np.arange(p) % g).astype(np.int64) if g else None
    return X, y, regs, labels


def call_step(g, p):
    import numpy as np
    from ls_spa import ls_spa_cv, ls_spa_cv_path
    from ls_spa._engine import HipEngine
    eng = HipEngine(0)
    X, y, regs, labels = setup(g, p)
    res = ls_spa_cv_path(X, y, regs, FOLDS, groups=labels, _engine=eng)          # first calls of the shape: buffers
    one = ls_spa_cv(X, y, float(regs[3]), FOLDS, groups=labels, _engine=eng)
    assert np.array_equal(res.attribution[3], one.attribution)                    # the two routes compute the same bits
    path_s, loop_s = [], []
    for _ in range(REPS):
        t = time.perf_counter()
        ls_spa_cv_path(X, y, regs, FOLDS, groups=labels, _engine=eng)
        path_s.append(time.perf_counter() - t)
        t = time.perf_counter()
        for r in regs:
            ls_spa_cv(X, y, float(r), FOLDS, groups=labels, _engine=eng)
        loop_s.append(time.perf_counter() - t)
    eng.close()
    a, b = statistics.median(path_s), statistics.median(loop_s)
    print(json.dumps(dict(step="call", g=g, p=p, path_s=a, loop_s=b, ratio=a / b)), flush=True)


def device_step(g, p):
    from ls_spa import cv_fold_ids
    from ls_spa._engine import HipEngine
    eng = HipEngine(0)
    X, y, regs, labels = setup(g, p)
    ids, _ = cv_fold_ids(N, FOLDS)
    if g:
        eng.cv_groups_load(X, y, ids, FOLDS, float(regs[0]))
        path, one = (lambda: eng.cv_path_groups_shapley(labels, regs)), (lambda: eng.cv_groups_shapley(labels))
    else:
        eng.cv_load(X, y, ids, FOLDS, float(regs[0]))
        path, one = (lambda: eng.cv_path_shapley(regs)), eng.cv_shapley
    path()
    one()
    path_ms, one_ms, rest = [], [], []
    for _ in range(REPS):
        t = time.perf_counter()
        info = path()[-1]
        wall = time.perf_counter() - t
        tp = eng.cv_timing()
        path_ms.append(tp["enumeration"] * 1e3)
        rest.append((wall - tp["enumeration"]) * 1e3)
        one()
        to = eng.cv_timing()
        one_ms.append(to["enumeration"] * 1e3)
    eng.cv_free()
    eng.close()
    a, b = statistics.median(path_ms), NREGS * statistics.median(one_ms)
    print(json.dumps(dict(step="device", g=g, p=p, launches=tp["launches"], one_launches=to["launches"], path_ms=a,
                          loop_ms=b, ratio=a / b, max_launch_ms=tp["max_launch"] * 1e3,
                          rest_ms=statistics.median(rest), not_pd=bool(info.any()))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEP_SECONDS), default=None, help="(internal) run one step in this process")
    ap.add_argument("--g", type=int, default=0)
    ap.add_argument("--p", type=int, default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.step:
        (call_step if a.step == "call" else device_step)(a.g, a.p)
        return 0
    rows = []
    for step in ("device", "call"):
        for g, p in SHAPES:
            cmd = ["timeout", "-k", "10", str(STEP_SECONDS[step]), sys.executable, os.path.abspath(__file__), "--step", step,
                   "--g", str(g), "--p", str(p)]
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            sys.stdout.write(r.stdout)
            sys.stdout.flush()
            rows += [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
            if r.returncode != 0:
                print(f"step {step} g = {g} p = {p} ended with status {r.returncode}: nothing more is started", flush=True)
                return 2
    ok = True
    print(f"{'g':>3} {'p':>3} {'launches':>8} {'path ms':>9} {'L x one ms':>10} {'ratio':>6} {'longest ms':>10} {'rest ms':>8}")
    for r in (r for r in rows if r["step"] == "device"):
        gated = (r["g"], r["p"]) in GATED
        ok = ok and (not gated or r["path_ms"] <= LIMIT * r["loop_ms"])
        print(f"{r['g']:>3} {r['p']:>3} {r['launches']:>8} {r['path_ms']:>9.3f} {r['loop_ms']:>10.3f} {r['ratio']:>6.3f} "
              f"{r['max_launch_ms']:>10.3f} {r['rest_ms']:>8.3f}" + (f"  (gated <= {LIMIT})" if gated else "")
              + ("  NOT_PD" if r["not_pd"] else ""))
    print(f"{'g':>3} {'p':>3} {'ls_spa_cv_path s':>16} {'loop of ls_spa_cv s':>19} {'ratio':>6}")
    for r in (r for r in rows if r["step"] == "call"):
        ok = ok and r["path_s"] < r["loop_s"]
        print(f"{r['g']:>3} {r['p']:>3} {r['path_s']:>16.4f} {r['loop_s']:>19.4f} {r['ratio']:>6.3f}  (required < 1)")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
