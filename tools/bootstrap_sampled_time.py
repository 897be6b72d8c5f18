"""Time the bootstrap of the sampled attribution (ls_spa_bootstrap_sampled) on one GPU (developer tool).

    python tools/bootstrap_sampled_time.py [--json out.json]

N = M = 10^4 rows, medians of REPS repeats after a warm-up, each step alone in its process.
1. lift: the device time of a lift launch (lsspa_boot_lift_timing) per (ordering, replicate) -- 256 orderings x 8
   replicates -- against lsspa_cv_lift_batch's fold launch per (ordering, fold) -- 256 orderings x 8 folds -- at the same
   p and grid size in the same process.  It is the same instantiation: the ratio must stay at or below LIMIT at p = 40
   and 100.
2. call: the whole call at (p, n_boot, n_samples) = (40, 200, 1024), (100, 200, 1024), (120, 100, 512) against the route
   there was before: n_boot calls of ls_spa(perms=) on np.take-n host rows with the same orderings, timed over OLD_CALLS
   of them and scaled, both on a kept engine.  The ratio must be below 1 at every shape.
3. gram: the Gram side of a run of 64 replicates (counts to the finalised problems are timed apart) per replicate and per
   flop (2 (N + M) 256 pairs) at cb = 6 (p = 90) and cb = 8 (p = 127), beside the one-wave kernel of cb = 5 at p = 64.
   Reported, not gated.
Every (step, shape) runs as a child process under a time limit of its own; the first one that fails ends the run.
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
N = 10000
OLD_CALLS = 20
LIFT_P = (40, 100)
CALL_SHAPES = ((40, 200, 1024), (100, 200, 1024), (120, 100, 512))
GRAM_P = (64, 90, 127)
STEP_SECONDS = {"lift": 180, "call": 420, "gram": 180}


def setup(p, n_samples):
    import numpy as np
    rng = np.random.default_rng(p)
    X = rng.standard_normal((2 * N, p)) + 0.3 * rng.standard_normal((2 * N, 1))
    beta = np.where(np.arange(p) % 3 == 0, 1.0 + 0.37 * np.arange(p), 0.05 * (1 + np.arange(p) % 5))
    y = X @ beta + 0.5 * rng.standard_normal(2 * N)
    perms = np.array([rng.permutation(p) for _ in range(n_samples)], dtype=np.int32)
    return (X[:N], X[N:], y[:N], y[N:]), perms


def lift_step(p):
    import numpy as np
    from ls_spa._engine import HipEngine
    eng = HipEngine(0)
    data, perms = setup(p, 128)
    K = 8
    ids = (np.arange(N) % K).astype(np.int32)
    eng.cv_lift_load(data[0], data[2], ids, K, 0.0)
    eng.boot_lift_load(*data, 0.0)
    eng.boot_lift_set_orderings(perms, True)
    eng.cv_lift_batch(perms, True, accumulate=False)
    eng.boot_lift_run(K, 42)
    boot_ms, cv_ms = [], []
    for _ in range(REPS):
        eng.boot_lift_run(K, 42)
        t = eng.boot_lift_timing()
        assert t["launches"] == 1
        boot_ms.append(t["lift"] * 1e3)
        eng.cv_lift_batch(perms, True, accumulate=False)
        cv_ms.append(eng.cv_lift_timing()["batch"] * 1e3)
    eng.boot_lift_free()
    eng.cv_lift_free()
    eng.close()
    a, b = statistics.median(boot_ms), statistics.median(cv_ms)
    print(json.dumps(dict(step="lift", p=p, pairs=256 * K, boot_ms=a, cv_ms=b, ratio=a / b)), flush=True)


def call_step(p, n_boot, n_samples):
    import warnings
    import numpy as np
    from ls_spa import ls_spa, ls_spa_bootstrap_sampled
    from ls_spa._engine import HipEngine
    eng = HipEngine(0)
    data, perms = setup(p, n_samples)
    rng = np.random.default_rng(1)

    def new():
        return ls_spa_bootstrap_sampled(*data, n_boot=n_boot, perms=perms, _engine=eng)

    def old(calls):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for _ in range(calls):
                ia, ie = rng.integers(0, N, N), rng.integers(0, N, N)
                ls_spa(np.take(data[0], ia, axis=0), np.take(data[1], ie, axis=0), data[2][ia], data[3][ie], perms=perms,
                       batch_size=256, tolerance=0.0, _engine=eng)

    new()
    old(2)
    new_s = []
    for _ in range(3):
        t = time.perf_counter()
        new()
        new_s.append(time.perf_counter() - t)
    t = time.perf_counter()
    old(OLD_CALLS)
    old_s = (time.perf_counter() - t) * n_boot / OLD_CALLS
    eng.close()
    a = statistics.median(new_s)
    print(json.dumps(dict(step="call", p=p, n_boot=n_boot, n_samples=n_samples, new_s=a, old_s=old_s, ratio=a / old_s)),
          flush=True)


def gram_step(p):
    from ls_spa._engine import HipEngine, debug_boot_lift_plan
    eng = HipEngine(0)
    data, perms = setup(p, 2)
    R = 64
    plan = debug_boot_lift_plan(R, N, N, p, p, 2, False)
    eng.boot_lift_load(*data, 0.0)
    eng.boot_lift_set_orderings(perms, False)
    eng.boot_lift_run(R, 42)
    ms, lift = [], []
    for _ in range(REPS):
        eng.boot_lift_run(R, 42)
        t = eng.boot_lift_timing()
        ms.append(t["gram"] * 1e3)
        lift.append(t["counts"] * 1e3)
    eng.boot_lift_free()
    eng.close()
    a = statistics.median(ms)
    pairs = plan["cb"] * (plan["cb"] + 1) // 2
    flops = 2.0 * (2 * N) * pairs * 256 * R
    print(json.dumps(dict(step="gram", p=p, cb=plan["cb"], form=plan["gram_form"], block=plan["block"], gram_ms=a,
                          ms_per_replicate=a / R, tflops=flops / (a * 1e-3) / 1e12,
                          counts_ms=statistics.median(lift))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=sorted(STEP_SECONDS), default=None, help="(internal) run one step in this process")
    ap.add_argument("--shape", type=int, nargs="*", default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if a.step:
        {"lift": lift_step, "call": call_step, "gram": gram_step}[a.step](*a.shape)
        return 0
    rows = []
    jobs = [("lift", (p,)) for p in LIFT_P] + [("gram", (p,)) for p in GRAM_P] + [("call", s) for s in CALL_SHAPES]
    for step, shape in jobs:
        cmd = ["timeout", "-k", "10", str(STEP_SECONDS[step]), sys.executable, os.path.abspath(__file__), "--step", step,
               "--shape"] + [str(v) for v in shape]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        rows += [json.loads(line) for line in r.stdout.splitlines() if line.startswith("{")]
        if r.returncode != 0:
            print(f"step {step} {shape} ended with status {r.returncode}: nothing more is started", flush=True)
            return 2
    ok = True
    for r in rows:
        if r["step"] == "lift":
            ok = ok and r["boot_ms"] <= LIMIT * r["cv_ms"]
            print(f"lift p={r['p']:>3}: {r['boot_ms']:.3f} ms against the fold launch's {r['cv_ms']:.3f} ms for "
                  f"{r['pairs']} pairs, ratio {r['ratio']:.3f} (required <= {LIMIT})")
        elif r["step"] == "gram":
            print(f"gram p={r['p']:>3} cb={r['cb']} form={r['form']}: {r['ms_per_replicate']:.4f} ms a replicate, "
                  f"{r['tflops']:.2f} Tflop/s (counts {r['counts_ms']:.3f} ms a run)")
        else:
            ok = ok and r["new_s"] < r["old_s"]
            print(f"call p={r['p']:>3} n_boot={r['n_boot']} n_samples={r['n_samples']}: {r['new_s']:.3f} s against "
                  f"{r['old_s']:.3f} s, ratio {r['ratio']:.3f} (required < 1)")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
