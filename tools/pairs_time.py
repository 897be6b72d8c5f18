"""Time a step of the sampled pairwise interactions (lsspa_pairs_batch) on one GPU (developer tool).

    python tools/pairs_time.py [d:B ...]        (default: 100:256 1000:256 4096:64)

Per shape, in one process: the step of pairs_batch on B samples (3 B orderings through the kernels, then the pair
kernels), beside it a plain launch + discard of the same 3 B unpaired orderings, and -- from a second pass under the
engine's per-launch event timing, one lane -- the share of the kernel class 'pairs' (Delta, per-pair statistics, lift
sum) in the device time of the step.  Steps are host-timed over REPS launches between two synchronisations."""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "ls-spa_amd"))
import numpy as np  # noqa: E402

from ls_spa._engine import HipEngine, debug_expand_pairs  # noqa: E402

REPS = 5


def problem(p, seed=0):
    rng = np.random.default_rng(seed)
    n, m = p + p // 2 + 64, p + p // 4 + 32
    Xa, Xe = rng.standard_normal((n, p), dtype=np.float32), rng.standard_normal((m, p), dtype=np.float32)
    w = (rng.standard_normal(p) / np.sqrt(p)).astype(np.float32)
    return Xa, Xe, Xa @ w + rng.standard_normal(n, dtype=np.float32), Xe @ w + rng.standard_normal(m, dtype=np.float32)


def timed(eng, fn):
    fn()                      # buffers, first launch
    eng.synchronize()
    t = time.perf_counter()
    for _ in range(REPS):
        fn()
    eng.synchronize()
    return (time.perf_counter() - t) / REPS


def main(shapes):
    eng = HipEngine(0)
    print(f"{'d':>5} {'B':>4} {'pairs step ms':>13} {'3B plain ms':>11} {'ratio':>6} {'pairs kernels ms':>16} {'share':>6}")
    for d, B in shapes:
        eng.load_data(*problem(d), 0.1)
        eng.full_fit()
        rng = np.random.default_rng(d)
        perms = np.array([rng.permutation(d) for _ in range(B)], dtype=np.int32)
        rows = debug_expand_pairs(perms)
        eng.pairs_enable(True)
        pairs = timed(eng, lambda: eng.pairs_batch(perms))
        plain = timed(eng, lambda: eng.discard_batch(eng.launch_batch(rows, False)))
        eng.profile(True)
        eng.profile_reset()
        for _ in range(REPS):
            eng.pairs_batch(perms)
        prof = eng.profile_read()
        eng.profile(False)
        eng.pairs_enable(False)
        total = sum(ms for ms, _ in prof.values())
        pk = prof["pairs"][0]
        print(f"{d:>5} {B:>4} {pairs * 1e3:>13.3f} {plain * 1e3:>11.3f} {pairs / plain:>6.3f} {pk / REPS:>16.3f} "
              f"{pk / total if total else float('nan'):>6.1%}", flush=True)
    eng.close()


if __name__ == "__main__":
    args = sys.argv[1:] or ["100:256", "1000:256", "4096:64"]
    main([tuple(int(x) for x in a.split(":")) for a in args])
