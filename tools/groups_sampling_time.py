"""Time the sampled attribution over groups of columns (ls_spa_groups) beside ls_spa at the same p (developer tool, GPU box).

    python tools/groups_sampling_time.py [g:p[:f32] ...]     (default: 40:200 100:1000 250:1000 500:5000:f32)

Per shape, same build, same engine, same number of orderings per step (128 antithetical samples = 256 orderings,
method 'argsort'):  the whole ls_spa_groups() call and the whole ls_spa() call (second call of the shape, kept engine,
512 samples, tolerance 0);  then the step alone on a bare engine -- one launch + collect of 128 samples, accumulate = 2,
mean of `steps` steps after two warm-up steps, with the player map set (g groups, a baseline of p // 50 columns, the
rest dealt evenly) and without it -- and the share of the fold kernel's class (lift) in the grouped step."""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "ls-spa_amd"))
import numpy as np  # noqa: E402

from ls_spa import ls_spa, ls_spa_groups  # noqa: E402
from ls_spa._engine import HipEngine  # noqa: E402


def problem(p, seed=0):
    rng = np.random.default_rng(seed)
    Xa, Xe = rng.standard_normal((2 * p + 200, p)), rng.standard_normal((p + 100, p))
    w = rng.standard_normal(p) / np.sqrt(p)
    return Xa, Xe, Xa @ w + rng.standard_normal(len(Xa)), Xe @ w + rng.standard_normal(len(Xe))


def labels_for(g, p):
    b = p // 50
    return np.concatenate([np.full(b, -1), np.sort(np.arange(p - b) % g)]).astype(np.int32)


def step_ms(eng, dim, samples, steps, seed):
    rng = np.random.default_rng(seed)
    batches = [np.array([rng.permutation(dim) for _ in range(samples)], dtype=np.int32) for _ in range(4)]
    eng.reset_stats()
    for k in range(2):
        eng.run_batch(batches[k], True, accumulate=2)
    eng.synchronize()
    t = time.perf_counter()
    for k in range(steps):
        eng.run_batch(batches[k % 4], True, accumulate=2)
    eng.synchronize()
    return (time.perf_counter() - t) / steps * 1e3


def main(shapes, steps=10, samples=128):
    eng = HipEngine(0)
    print(f"{'g':>4} {'p':>5} {'prec':>7} {'groups call s':>13} {'ls_spa call s':>13} {'grouped ms/step':>15} "
          f"{'ungrouped ms/step':>17} {'ratio':>6} {'lift class ms (grouped / ungrouped)':>36}")
    for g, p, prec in shapes:
        d = problem(p)
        labels = labels_for(g, p)
        kw = dict(method="argsort", max_samples=512, batch_size=samples, tolerance=0.0, seed=1, precision=prec)
        whole = {}
        for name, call in (("groups", lambda: ls_spa_groups(*d, labels, **kw)), ("plain", lambda: ls_spa(*d, **kw))):
            call()
            t = time.perf_counter()
            call()
            whole[name] = time.perf_counter() - t
        eng.set_precision(prec)
        eng.load_data(*d, 0.0)
        eng.full_fit()
        out = {}
        for name in ("plain", "groups"):
            if name == "groups":
                eng.set_players(labels)
            ms = step_ms(eng, g if name == "groups" else p, samples, steps, seed=2)
            eng.profile(True)
            eng.profile_reset()
            step_ms(eng, g if name == "groups" else p, samples, 4, seed=3)
            prof = eng.profile_read()
            eng.profile(False)
            out[name] = (ms, prof["lift"][0] / 6.0)      # the profiled run: two warm-up steps and four
        eng.clear_players()
        print(f"{g:>4} {p:>5} {prec:>7} {whole['groups']:>13.4f} {whole['plain']:>13.4f} {out['groups'][0]:>15.3f} "
              f"{out['plain'][0]:>17.3f} {out['groups'][0] / out['plain'][0]:>6.3f} "
              f"{out['groups'][1]:>17.4f} / {out['plain'][1]:.4f}", flush=True)
    eng.close()


if __name__ == "__main__":
    todo = []
    for a in sys.argv[1:] or ["40:200", "100:1000", "250:1000", "500:5000:f32"]:
        f = a.split(":")
        todo.append((int(f[0]), int(f[1]), "float32" if len(f) > 2 and f[2] == "f32" else "float64"))
    main(todo)
