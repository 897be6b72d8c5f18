"""Time the best-subset selection over groups of columns (ls_spa_best_subsets(groups=)) on one GPU (developer tool).

    python tools/group_best_time.py

Per (g, p): the whole ls_spa_best_subsets(groups=) call (reduction, full fit, enumeration, host refits; second call of
the shape, kept engine), the library call alone, the device time of its enumeration launches -- and beside it, in the
same process, on the same problem and labels, the device time of lsspa_groups_shapley's, both from lsspa_groups_timing.
The two kernels share group_values and the launch geometry and differ in the per-subset bookkeeping only (a
compare-select in LDS against phi's 32 weighted sums); the ratio of the two is the last column and must stay at or
below LIMIT.  Each side is timed REPS times alternately; the table shows the medians.  Exit status 1 if a ratio exceeds
LIMIT."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "ls-spa_amd"))
import numpy as np  # noqa: E402

from ls_spa import ls_spa_best_subsets  # noqa: E402
from ls_spa._engine import HipEngine  # noqa: E402

REPS = 5
LIMIT = 1.05
SHAPES = ((12, 64), (16, 48), (20, 60), (24, 64))


def problem(p, seed=0):
    rng = np.random.default_rng(seed)
    Xa, Xe = rng.standard_normal((4 * p + 100, p)), rng.standard_normal((2 * p + 50, p))
    w = rng.standard_normal(p) / np.sqrt(p)
    return Xa, Xe, Xa @ w + rng.standard_normal(len(Xa)), Xe @ w + rng.standard_normal(len(Xe))


def main():
    eng = HipEngine(0)
    ok = True
    print(f"{'g':>3} {'p':>3} {'ls_spa_best_subsets s':>21} {'call s':>9} {'launches':>8} {'longest ms':>10} "
          f"{'best ms':>9} {'phi ms':>9} {'ratio':>6}")
    for g, p in SHAPES:
        d = problem(p)
        labels = np.sort(np.arange(p) % g)                     # g groups of p // g or p // g + 1 columns, no baseline
        ls_spa_best_subsets(*d, groups=labels)                 # first call of the shape: engine, buffers
        t = time.perf_counter()
        ls_spa_best_subsets(*d, groups=labels)
        whole = time.perf_counter() - t
        eng.load_data(*d, 0.0)
        eng.groups_best(labels)
        eng.groups_shapley(labels)
        best_ms, phi_ms, calls = [], [], []
        for _ in range(REPS):
            t = time.perf_counter()
            _, _, _, info = eng.groups_best(labels)
            calls.append(time.perf_counter() - t)
            kernels, longest, launches = eng.groups_timing()
            best_ms.append(kernels * 1e3)
            eng.groups_shapley(labels)
            k_s, _, n = eng.groups_timing()
            phi_ms.append(k_s * 1e3)
            assert n == launches, (n, launches)
        b, r = statistics.median(best_ms), statistics.median(phi_ms)
        ok = ok and b <= LIMIT * r
        print(f"{g:>3} {p:>3} {whole:>21.4f} {statistics.median(calls):>9.4f} {launches:>8} {longest * 1e3:>10.2f} "
              f"{b:>9.3f} {r:>9.3f} {b / r:>6.3f}" + ("  NOT_PD" if info else ""), flush=True)
    eng.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
