"""Time ls_spa_permutation_test against what a user could do before it existed, in one process on one GPU:
NumPy permutations -> explicit Y_train / Y_test -> ls_spa_multi (in calls small enough for its column limit and the
host's memory) -> the same p-values.

    python tools/permutation_time.py [--quick]

Per shape: the whole call (best of two), the four shares lsspa_perm_timing reports (drawing and uploading the index
rows are host times of the library's threads and overlap the GPU from the second block on), the alternative's whole
time, their ratio (the requirement: < 1 at every shape), and what perm_xty_kernel moves -- index rows, X once a
64-replicate workgroup row, y -- per second of its own time against the 6.29 TB/s an HBM copy reaches on this part
(8.0 TB/s spec).  Prints one JSON line per shape and a table.
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ls-spa_amd"))

from ls_spa import ls_spa_multi, ls_spa_permutation_test          # noqa: E402
from ls_spa._engine import HipEngine                               # noqa: E402
from ls_spa._results import PermutationTestResults                 # noqa: E402

HBM_COPY = 6.29e12
SHAPES = [(10 ** 4, 12, 1000, None), (10 ** 4, 16, 1000, None), (10 ** 4, 24, 200, None),
          (10 ** 5, 12, 1000, None), (10 ** 5, 16, 1000, None), (10 ** 5, 24, 200, None),
          (10 ** 5, 64, 1000, 12)]
CHUNK = 250          # responses per ls_spa_multi call of the alternative: 2 x 200 MB of Y at N = 10^5


def problem(n, p, seed=0):
    rng = np.random.default_rng(seed)
    Xa, Xe = rng.standard_normal((n, p)), rng.standard_normal((n, p))
    w = rng.standard_normal(p) * (rng.random(p) < 0.5)
    return Xa, Xe, Xa @ w + rng.standard_normal(n), Xe @ w + rng.standard_normal(n)


def by_hand(Xa, Xe, ya, ye, n_perm, groups, engine):
    rng = np.random.default_rng(42)
    obs = ls_spa_multi(Xa, Xe, ya, ye, groups=groups, _engine=engine)
    null, r2 = [], []
    for r0 in range(0, n_perm, CHUNK):
        nb = min(CHUNK, n_perm - r0)
        Ya = np.stack([ya[rng.permutation(len(ya))] for _ in range(nb)], axis=1)
        Ye = np.stack([ye[rng.permutation(len(ye))] for _ in range(nb)], axis=1)
        res = ls_spa_multi(Xa, Xe, Ya, Ye, groups=groups, _engine=engine)
        null.append(res.attribution)
        r2.append(res.r_squared)
    return PermutationTestResults.from_null(obs.attribution[0], obs.theta[0], obs.r_squared[0], np.concatenate(null),
                                            np.concatenate(r2))


def main():
    shapes = SHAPES[:1] if "--quick" in sys.argv else SHAPES
    engine = HipEngine(0)
    rows = []
    try:
        ls_spa_permutation_test(*problem(2000, 8), n_perm=64, _engine=engine)          # warm-up
        for n, p, n_perm, g in shapes:
            d = problem(n, p, seed=p)
            groups = None if g is None else np.arange(p) % g
            best = None
            for _ in range(2):
                t0 = time.perf_counter()
                res = ls_spa_permutation_test(*d, n_perm=n_perm, groups=groups, _engine=engine)
                dt = time.perf_counter() - t0
                if best is None or dt < best[0]:
                    best = (dt, dict(engine.perm_timing_last))
            t0 = time.perf_counter()
            ref = by_hand(*d, n_perm, groups, engine)
            alt = time.perf_counter() - t0
            whole, tm = best
            cb = (p + 15) // 16
            moved = 2 * n * n_perm * 4 + 2 * n * 8 * 16 * cb * ((n_perm + 63) // 64) + 2 * n * 8
            row = dict(N=n, M=n, p=p, g=g, n_perm=n_perm, whole_s=whole, **{k + "_s": v for k, v in tm.items()}, by_hand_s=alt,
                       ratio=whole / alt, xty_bytes=moved, xty_bytes_per_s=moved / max(tm["xty"], 1e-12),
                       xty_share_of_hbm_copy=moved / max(tm["xty"], 1e-12) / HBM_COPY,
                       min_p=float(res.p_values.min()), min_p_by_hand=float(ref.p_values.min()))
            rows.append(row)
            print(json.dumps(row), flush=True)
    finally:
        engine.close()
    print(f"{'N':>7} {'p':>3} {'g':>3} {'perms':>5} {'whole':>8} {'draw':>8} {'upload':>8} {'xty':>8} {'enum':>8} {'by hand':>8} "
          f"{'ratio':>6} {'xty TB/s':>8}")
    for r in rows:
        print(f"{r['N']:>7} {r['p']:>3} {r['g'] or 0:>3} {r['n_perm']:>5} {r['whole_s']:>8.3f} {r['draw_s']:>8.3f} "
              f"{r['upload_s']:>8.3f} {r['xty_s']:>8.4f} {r['enumeration_s']:>8.3f} {r['by_hand_s']:>8.3f} {r['ratio']:>6.3f} "
              f"{r['xty_bytes_per_s'] / 1e12:>8.3f}")
    return 0 if all(r["ratio"] < 1 for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
