"""Time the exact Owen values (ls_spa_owen) on one GPU (developer tool).

    python tools/owen_time.py

Per shape: the whole ls_spa_owen() call (reduction, full fit, every enumeration; second call of the shape, kept engine),
the library call alone, the device time of all its enumeration launches (lsspa_groups_timing) -- and beside it, in the
same process, the reference: lsspa_groups_shapley on the labels (the group game, which the Owen call runs too) and on
the refined labels of every group of two or more columns, the same subsets through the existing kernel.  The Owen
launches differ from the reference's by the weight lookup only; the ratio of the two sums is the last column.  Each
side is timed REPS times alternately; the table shows the medians."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "ls-spa_amd"))
import numpy as np  # noqa: E402

from ls_spa import ls_spa_owen  # noqa: E402
from ls_spa._engine import HipEngine  # noqa: E402

REPS = 5


def problem(p, seed=0):
    rng = np.random.default_rng(seed)
    Xa, Xe = rng.standard_normal((4 * p + 100, p)), rng.standard_normal((2 * p + 50, p))
    w = rng.standard_normal(p) / np.sqrt(p)
    return Xa, Xe, Xa @ w + rng.standard_normal(len(Xa)), Xe @ w + rng.standard_normal(len(Xe))


def labels_of(sizes, baseline=0):
    return np.concatenate([np.full(baseline, -1)] + [np.full(s, k) for k, s in enumerate(sizes)]).astype(np.int32)


def refined(labels, k):
    """The labels of group k's refined game in the library's numbering: the group's columns take its place."""
    b = int((labels == k).sum())
    ref = np.where(labels < k, labels, labels + b - 1)
    ref[labels == k] = k + np.arange(b)
    return ref.astype(np.int32)


SHAPES = [
    ("12 groups of 5, 4 baseline (p = 64)", labels_of([5] * 12, 4)),
    ("16 groups of 3 (p = 48)", labels_of([3] * 16)),
    ("14 groups of 4 and one of 8 (p = 64)", labels_of([4] * 14 + [8])),
    ("a 16-level factor among 8 singletons (p = 24)", labels_of([1] * 8 + [16])),
]


def main():
    eng = HipEngine(0)
    print(f"{'shape':<46} {'ls_spa_owen s':>13} {'call s':>9} {'launches':>8} {'longest ms':>10} {'owen ms':>9} "
          f"{'reference ms':>12} {'ratio':>6}")
    for name, labels in SHAPES:
        d = problem(len(labels))
        g = int(labels.max()) + 1
        ls_spa_owen(*d, labels)                                # first call of the shape: engine, buffers
        t = time.perf_counter()
        ls_spa_owen(*d, labels)
        whole = time.perf_counter() - t
        eng.load_data(*d, 0.0)
        games = [labels] + [refined(labels, k) for k in range(g) if (labels == k).sum() >= 2]
        eng.groups_owen(labels)
        for lab in games:
            eng.groups_shapley(lab)
        owen_ms, ref_ms, calls = [], [], []
        for _ in range(REPS):
            t = time.perf_counter()
            _, _, info = eng.groups_owen(labels)
            calls.append(time.perf_counter() - t)
            kernels, longest, launches = eng.groups_timing()
            owen_ms.append(kernels * 1e3)
            total, n_ref = 0.0, 0
            for lab in games:
                eng.groups_shapley(lab)
                k_s, _, n = eng.groups_timing()
                total += k_s * 1e3
                n_ref += n
            ref_ms.append(total)
            assert n_ref == launches, (n_ref, launches)
        o, r = statistics.median(owen_ms), statistics.median(ref_ms)
        print(f"{name:<46} {whole:>13.4f} {statistics.median(calls):>9.4f} {launches:>8} {longest * 1e3:>10.2f} "
              f"{o:>9.3f} {r:>12.3f} {o / r:>6.3f}" + ("  NOT_PD" if info else ""), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
