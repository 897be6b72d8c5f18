"""Time the top lists of the cross-validated selection over groups of columns (ls_spa_top_group_subsets_cv) on
one GPU (developer tool).

    python tools/cv_groups_top_time.py [--json out.json]

N = 10^4 rows, K = 5 folds, (g, p) = (12, 64), (16, 48), (20, 60) with the labels of tools/cv_groups_time.py, kept
engine, medians of REPS alternating repeats.
1. Kernels against the sibling: per shape and T the device time of lsspa_cv_groups_top's enumeration launches beside
   that of lsspa_cv_groups_best's on the same loaded folds, in the same process, both from lsspa_cv_timing.  The two
   kernels share the fold-step and the launch geometry and differ in the per-subset bookkeeping and in their LDS (three
   workgroups a CU against two).  The ratio at T = 1 must stay at or below LIMIT at g = 16 and 20; the other ratios are
   reported.  "rest ms" is the library call's wall time minus its enumeration launches: the layout's upload, clearing
   the counts, the reduction over the units' lists, the listed models' per-fold values, the copies of the result.
2. The whole call against the route a user had before: ls_spa_top_group_subsets_cv(n_best = 10) beside
   debug_cv_group_values over all 2^g masks on loaded folds followed by a host argpartition per size.  Both routes must
   list the same models; the ratio must be below 1 at g = 16 and 20.
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
N, FOLDS = 10000, 5
SHAPES = ((12, 64), (16, 48), (20, 60))
KERNEL_T = (1, 4, 16)
ROUTE_T = 10
STEP_SECONDS = {"kernel": 180, "route": 300}


def problem(g, p):
    from cv_groups_time import labels_of
    from cv_time import data
    return data(p, N, seed=p + g) + (labels_of(g, p),)


def old_route(eng, labels, g, T):
    """What a user could do before: every value through the debug hook, then the T largest of every size on the host."""
    import numpy as np
    masks = np.arange(1 << g, dtype=np.uint64)
    u, _ = eng.debug_cv_group_values(labels, masks, folds=False)
    size = np.zeros(1 << g, dtype=np.uint8)
    for j in range(g):
        size += ((masks >> np.uint64(j)) & np.uint64(1)).astype(np.uint8)
    out = []
    for k in range(g + 1):
        sel = np.nonzero(size == k)[0]
        if len(sel) > T:
            sel = sel[np.argpartition(-u[sel], T - 1)[:T]]
        out.append(sel[np.argsort(-u[sel], kind="stable")])
    return out


def kernel_step(g, p):
    from ls_spa import cv_fold_ids
    from ls_spa._engine import HipEngine
    eng = HipEngine(0)
    X, y, labels = problem(g, p)
    ids, _ = cv_fold_ids(N, FOLDS)
    eng.cv_groups_load(X, y, ids, FOLDS, 0.0)
    eng.cv_groups_best(labels)
    for T in KERNEL_T:
        eng.cv_groups_top(labels, T)
        top_ms, best_ms, calls, rest = [], [], [], []
        for _ in range(REPS):
            t = time.perf_counter()
            _, _, _, _, info = eng.cv_groups_top(labels, T)
            wall = time.perf_counter() - t
            tm = eng.cv_timing()
            calls.append(wall)
            top_ms.append(tm["enumeration"] * 1e3)
            rest.append((wall - tm["enumeration"]) * 1e3)
            eng.cv_groups_best(labels)
            tb = eng.cv_timing()
            best_ms.append(tb["enumeration"] * 1e3)
            assert tb["launches"] == tm["launches"], (tb, tm)
        a, b = statistics.median(top_ms), statistics.median(best_ms)
        print(json.dumps(dict(step="kernel", g=g, p=p, T=T, launches=tm["launches"], top_ms=a, best_ms=b, ratio=a / b,
                              call_s=statistics.median(calls), rest_ms=statistics.median(rest),
                              not_pd=bool(info.any()))), flush=True)
    eng.cv_free()
    eng.close()


def route_step(g, p):
    import numpy as np
    from ls_spa import cv_fold_ids, ls_spa_top_group_subsets_cv
    from ls_spa._engine import HipEngine
    eng = HipEngine(0)
    X, y, labels = problem(g, p)
    ids, _ = cv_fold_ids(N, FOLDS)
    kw = dict(folds=FOLDS, n_best=ROUTE_T, _engine=eng)
    res = ls_spa_top_group_subsets_cv(X, y, labels, **kw)                            # first call of the shape: buffers
    eng.cv_groups_load(X, y, ids, FOLDS, 0.0)
    old = old_route(eng, labels, g, ROUTE_T)
    for k in res.sizes:                                                # the two routes list the same models
        got = [sum(1 << int(j) for j in np.nonzero(s)[0]) for s in res.group_subsets[k, :res.n_models[k]]]
        assert sorted(got) == sorted(old[k].tolist()), (g, p, k)
    new_s, old_s = [], []
    for _ in range(REPS):
        eng.cv_free()
        t = time.perf_counter()
        ls_spa_top_group_subsets_cv(X, y, labels, **kw)                              # loads, lists, refits, frees
        new_s.append(time.perf_counter() - t)
        eng.cv_groups_load(X, y, ids, FOLDS, 0.0)
        t = time.perf_counter()
        old_route(eng, labels, g, ROUTE_T)                             # on loaded folds: the load is not counted
        old_s.append(time.perf_counter() - t)
    eng.cv_free()
    eng.close()
    a, b = statistics.median(new_s), statistics.median(old_s)
    print(json.dumps(dict(step="route", g=g, p=p, n_best=ROUTE_T, call_s=a, prior_route_s=b, ratio=a / b)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEP_SECONDS), default=None, help="(internal) run one step in this process")
    ap.add_argument("--g", type=int, default=None)
    ap.add_argument("--p", type=int, default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.step:
        sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
        (kernel_step if a.step == "kernel" else route_step)(a.g, a.p)
        return 0
    rows = []
    for step in ("kernel", "route"):
        for g, p in SHAPES:
            cmd = ["timeout", "-k", "10", str(STEP_SECONDS[step]), sys.executable, os.path.abspath(__file__), "--step", step,
                   "--g", str(g), "--p", str(p)]
            r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            sys.stdout.write(r.stdout)
            sys.stdout.flush()
            rows += [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
            if r.returncode != 0:
                print(f"step {step} g = {g}, p = {p} ended with status {r.returncode}: nothing more is started",
                      flush=True)
                return 2
    ok = True
    print(f"{'g':>3} {'p':>3} {'T':>3} {'launches':>8} {'top ms':>9} {'best ms':>9} {'ratio':>6} {'call s':>9} "
          f"{'rest ms':>8}")
    for r in (r for r in rows if r["step"] == "kernel"):
        gated = r["T"] == 1 and r["g"] >= 16
        ok = ok and (not gated or r["top_ms"] <= LIMIT * r["best_ms"])
        print(f"{r['g']:>3} {r['p']:>3} {r['T']:>3} {r['launches']:>8} {r['top_ms']:>9.3f} {r['best_ms']:>9.3f} "
              f"{r['ratio']:>6.3f} {r['call_s']:>9.4f} {r['rest_ms']:>8.3f}"
              + (f"  (gated <= {LIMIT})" if gated else "") + ("  NOT_PD" if r["not_pd"] else ""))
    print(f"{'g':>3} {'p':>3} {'ls_spa_top_group_subsets_cv s':>32} {'debug values + argpartition s':>29} "
          f"{'ratio':>6}")
    for r in (r for r in rows if r["step"] == "route"):
        required = r["g"] >= 16
        ok = ok and (not required or r["call_s"] < r["prior_route_s"])
        print(f"{r['g']:>3} {r['p']:>3} {r['call_s']:>32.4f} {r['prior_route_s']:>29.4f} {r['ratio']:>6.3f}"
              + ("  (required < 1)" if required else ""))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
