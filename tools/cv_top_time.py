"""Time the top lists of the cross-validated selection (ls_spa_top_subsets_cv) on one GPU (developer tool).

    python tools/cv_top_time.py [--json out.json]

N = 10^4 rows, K = 5 folds, kept engine, medians of REPS alternating repeats.
1. Kernels against the sibling: per p and T the device time of lsspa_cv_top's enumeration launches beside that of
   lsspa_cv_best's on the same loaded folds, in the same process, both from lsspa_cv_timing.  The two kernels share the
   fold-step and the launch geometry and differ in the per-subset bookkeeping only.  The ratio at T = 1 must stay at or
   below LIMIT at p = 20 and 24; the other ratios are reported.  "rest ms" is the library call's wall time minus its
   enumeration launches: clearing the counts, the reduction over the units' lists, the listed models' per-fold values,
   the copies of the result.
2. The whole call against the route a user had before: ls_spa_top_subsets_cv(n_best = 10) beside debug_cv_values over
   all 2^p masks on loaded folds followed by a host argpartition per size.  The ratio must be below 1 at p = 20 and 24.
Every (section, p) runs as a child process under a time limit of its own; the first one that fails ends the run.
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
N, FOLDS = 10000, 5
SIZES = (16, 20, 24)
KERNEL_T = (1, 4, 16)
ROUTE_T = 10
STEP_SECONDS = {"kernel": 120, "route": 300}


def data(p, n, seed):
    import numpy as np
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, p)) + 0.3 * rng.standard_normal((n, 1))
    beta = np.where(np.arange(p) % 3 == 0, 1.0 + 0.37 * np.arange(p), 0.05 * (1 + np.arange(p) % 5))
    return X, X @ beta + 0.5 * rng.standard_normal(n)


def old_route(eng, p, T):
    """What a user could do before: every value through the debug hook, then the T largest of every size on the host."""
    import numpy as np
    masks = np.arange(1 << p, dtype=np.uint64)
    v, _ = eng.debug_cv_values(masks, folds=False)
    size = np.zeros(1 << p, dtype=np.uint8)
    for j in range(p):
        size += ((masks >> np.uint64(j)) & np.uint64(1)).astype(np.uint8)
    out = []
    for k in range(p + 1):
        sel = np.nonzero(size == k)[0]
        if len(sel) > T:
            sel = sel[np.argpartition(-v[sel], T - 1)[:T]]
        out.append(sel[np.argsort(-v[sel], kind="stable")])
    return out


def kernel_step(p):
    from ls_spa import cv_fold_ids
    from ls_spa._engine import HipEngine
    eng = HipEngine(0)
    X, y = data(p, N, seed=p)
    ids, _ = cv_fold_ids(N, FOLDS)
    eng.cv_load(X, y, ids, FOLDS, 0.0)
    eng.cv_best()
    for T in KERNEL_T:
        eng.cv_top(0, T)
        top_ms, best_ms, calls, rest = [], [], [], []
        for _ in range(REPS):
            t = time.perf_counter()
            _, _, _, _, info = eng.cv_top(0, T)
            wall = time.perf_counter() - t
            tm = eng.cv_timing()
            calls.append(wall)
            top_ms.append(tm["enumeration"] * 1e3)
            rest.append((wall - tm["enumeration"]) * 1e3)
            eng.cv_best()
            tb = eng.cv_timing()
            best_ms.append(tb["enumeration"] * 1e3)
            assert tb["launches"] == tm["launches"], (tb, tm)
        a, b = statistics.median(top_ms), statistics.median(best_ms)
        print(json.dumps(dict(step="kernel", p=p, T=T, launches=tm["launches"], top_ms=a, best_ms=b, ratio=a / b,
                              call_s=statistics.median(calls), rest_ms=statistics.median(rest),
                              not_pd=bool(info.any()))), flush=True)
    eng.cv_free()
    eng.close()


def route_step(p):
    import numpy as np
    from ls_spa import cv_fold_ids, ls_spa_top_subsets_cv
    from ls_spa._engine import HipEngine
    eng = HipEngine(0)
    X, y = data(p, N, seed=p)
    ids, _ = cv_fold_ids(N, FOLDS)
    res = ls_spa_top_subsets_cv(X, y, folds=FOLDS, n_best=ROUTE_T, _engine=eng)      # first call of the shape: buffers
    eng.cv_load(X, y, ids, FOLDS, 0.0)
    old = old_route(eng, p, ROUTE_T)
    for i, k in enumerate(res.sizes):                                  # the two routes list the same models
        got = [sum(1 << int(j) for j in np.nonzero(s)[0]) for s in res.subsets[i, :res.n_models[i]]]
        assert sorted(got) == sorted(old[k].tolist()), (p, k)
    new_s, old_s = [], []
    for _ in range(REPS):
        eng.cv_free()
        t = time.perf_counter()
        ls_spa_top_subsets_cv(X, y, folds=FOLDS, n_best=ROUTE_T, _engine=eng)      # loads, lists, refits, frees
        new_s.append(time.perf_counter() - t)
        eng.cv_load(X, y, ids, FOLDS, 0.0)
        t = time.perf_counter()
        old_route(eng, p, ROUTE_T)                                     # on loaded folds: the load is not counted
        old_s.append(time.perf_counter() - t)
    eng.cv_free()
    eng.close()
    a, b = statistics.median(new_s), statistics.median(old_s)
    print(json.dumps(dict(step="route", p=p, n_best=ROUTE_T, call_s=a, prior_route_s=b, ratio=a / b)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEP_SECONDS), default=None, help="(internal) run one step in this process")
    ap.add_argument("--p", type=int, default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.step:
        (kernel_step if a.step == "kernel" else route_step)(a.p)
        return 0
    rows = []
    for step in ("kernel", "route"):
        for p in SIZES:
            cmd = ["timeout", "-k", "10", str(STEP_SECONDS[step]), sys.executable, os.path.abspath(__file__), "--step", step,
                   "--p", str(p)]
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            sys.stdout.write(r.stdout)
            sys.stdout.flush()
            rows += [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
            if r.returncode != 0:
                print(f"step {step} p = {p} ended with status {r.returncode}: nothing more is started", flush=True)
                return 2
    ok = True
    print(f"{'p':>3} {'T':>3} {'launches':>8} {'top ms':>9} {'best ms':>9} {'ratio':>6} {'call s':>9} {'rest ms':>8}")
    for r in (r for r in rows if r["step"] == "kernel"):
        gated = r["T"] == 1 and r["p"] >= 20
        ok = ok and (not gated or r["top_ms"] <= LIMIT * r["best_ms"])
        print(f"{r['p']:>3} {r['T']:>3} {r['launches']:>8} {r['top_ms']:>9.3f} {r['best_ms']:>9.3f} {r['ratio']:>6.3f} "
              f"{r['call_s']:>9.4f} {r['rest_ms']:>8.3f}" + (f"  (gated <= {LIMIT})" if gated else "")
              + ("  NOT_PD" if r["not_pd"] else ""))
    print(f"{'p':>3} {'ls_spa_top_subsets_cv s':>23} {'debug values + argpartition s':>29} {'ratio':>6}")
    for r in (r for r in rows if r["step"] == "route"):
        required = r["p"] >= 20
        ok = ok and (not required or r["call_s"] < r["prior_route_s"])
        print(f"{r['p']:>3} {r['call_s']:>23.4f} {r['prior_route_s']:>29.4f} {r['ratio']:>6.3f}"
              + ("  (required < 1)" if required else ""))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
