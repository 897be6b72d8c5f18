"""Time the exact attribution over groups of columns (ls_spa(method='subsets', groups=labels)) on one GPU (developer tool).

    python tools/groups_time.py [g:p ...]        (default: 12:64 16:48 20:60 24:64 24:24 28:56)

The p columns are dealt to the g groups as evenly as they go (the first p mod g groups get one more); g:p:b puts b
of the p columns into the baseline.  Per shape: the whole ls_spa() call (reduction, full fit, enumeration; second call
of the shape, kept engine), the library call alone, the device time of its enumeration launches, their number, the
longest one and |sum(phi) - (R^2 - R^2 of the baseline)|.  24:24 is also timed through the ungrouped call."""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "ls-spa_amd"))
import numpy as np  # noqa: E402

from ls_spa import ls_spa  # noqa: E402
from ls_spa._engine import HipEngine  # noqa: E402


def problem(p, seed=0):
    rng = np.random.default_rng(seed)
    Xa, Xe = rng.standard_normal((4 * p + 100, p)), rng.standard_normal((2 * p + 50, p))
    w = rng.standard_normal(p) / np.sqrt(p)
    return Xa, Xe, Xa @ w + rng.standard_normal(len(Xa)), Xe @ w + rng.standard_normal(len(Xe))


def labels_for(g, p, b):
    return np.concatenate([np.full(b, -1), np.sort(np.arange(p - b) % g)]).astype(np.int32)


def baseline_r2(d, labels):
    Xa, Xe, ya, ye = d
    B = np.nonzero(labels < 0)[0]
    if len(B) == 0:
        return 0.0
    th = np.linalg.solve(Xa[:, B].T @ Xa[:, B], Xa[:, B].T @ ya)
    r = ye - Xe[:, B] @ th
    return 1.0 - float(r @ r) / float(ye @ ye)


def main(shapes):
    eng = HipEngine(0)
    print(f"{'g':>3} {'p':>3} {'base':>4} {'ls_spa s':>10} {'call s':>10} {'kernels s':>10} {'launches':>8} "
          f"{'longest ms':>10} {'|sum-dR2|':>9}")
    for g, p, b in shapes:
        d = problem(p)
        labels = labels_for(g, p, b)
        ls_spa(*d, method="subsets", groups=labels)           # first call of the shape: engine, buffers
        t = time.perf_counter()
        res = ls_spa(*d, method="subsets", groups=labels)
        whole = time.perf_counter() - t
        eng.load_data(*d, 0.0)
        eng.groups_shapley(labels)
        t = time.perf_counter()
        phi, info = eng.groups_shapley(labels)
        call = time.perf_counter() - t
        kernels, longest, launches = eng.groups_timing()
        eff = abs(res.attribution.sum() - (res.r_squared - baseline_r2(d, labels)))
        print(f"{g:>3} {p:>3} {b:>4} {whole:>10.4f} {call:>10.4f} {kernels:>10.4f} {launches:>8} {longest * 1e3:>10.2f} "
              f"{eff:>9.1e}" + ("  NOT_PD" if info else ""), flush=True)
        if g == p and b == 0 and p <= 32:
            eng.subsets_shapley()
            t = time.perf_counter()
            eng.subsets_shapley()
            call = time.perf_counter() - t
            kernels, longest, launches = eng.subsets_timing()
            print(f"    ungrouped method='subsets' at p = {p}: call {call:.4f} s, kernels {kernels:.4f} s, "
                  f"{launches} launches, longest {longest * 1e3:.2f} ms", flush=True)
    eng.close()


if __name__ == "__main__":
    args = sys.argv[1:] or ["12:64", "16:48", "20:60", "24:64", "24:24", "28:56"]
    main([(tuple(int(x) for x in a.split(":")) + (0,))[:3] for a in args])
