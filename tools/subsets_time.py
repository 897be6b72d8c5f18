"""Time the exact attribution by subset enumeration (ls_spa(method='subsets')) on one GPU (developer tool).

    python tools/subsets_time.py [p ...]        (default: 16 20 24 28 30 32)

Per p: the whole ls_spa() call (reduction, full fit, enumeration; second call of the shape, kept engine), the
library call alone, the device time of its enumeration launches, their number and the longest one."""
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


def main(ps):
    eng = HipEngine(0)
    print(f"{'p':>3} {'ls_spa s':>10} {'call s':>10} {'kernels s':>10} {'launches':>8} {'longest ms':>10} {'|sum-R2|':>9}")
    for p in ps:
        d = problem(p)
        ls_spa(*d, method="subsets")                       # first call of the shape: engine, buffers
        t = time.perf_counter()
        res = ls_spa(*d, method="subsets")
        whole = time.perf_counter() - t
        eng.load_data(*d, 0.0)
        eng.subsets_shapley()
        t = time.perf_counter()
        phi, info = eng.subsets_shapley()
        call = time.perf_counter() - t
        kernels, longest, launches = eng.subsets_timing()
        eff = abs(res.attribution.sum() - res.r_squared)
        print(f"{p:>3} {whole:>10.4f} {call:>10.4f} {kernels:>10.4f} {launches:>8} {longest * 1e3:>10.2f} {eff:>9.1e}"
              + ("  NOT_PD" if info else ""), flush=True)
    eng.close()


if __name__ == "__main__":
    main([int(a) for a in sys.argv[1:]] or [16, 20, 24, 28, 30, 32])
