"""Time the exact pairwise interaction values (ls_spa_interactions) beside the attribution alone (developer tool).

    python tools/interactions_time.py [p ...]        (default: 16 20 24 28 30 32)

Per p, in one process on one engine: the whole ls_spa_interactions() call (reduction, full fit, enumeration; second call
of the shape, kept engine), the library call alone and the device time of its enumeration launches -- and the library
call and device time of subsets_shapley on the same problem, with the ratio of the two device times."""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "ls-spa_amd"))
import numpy as np  # noqa: E402

from ls_spa import ls_spa_interactions  # noqa: E402
from ls_spa._engine import HipEngine  # noqa: E402
from subsets_time import problem  # noqa: E402


def timed(call, timing):
    call()                                                  # first call of the shape: buffers
    t = time.perf_counter()
    out = call()
    return out, time.perf_counter() - t, timing()


def main(ps):
    eng = HipEngine(0)
    print(f"{'p':>3} {'public s':>9} {'call s':>9} {'kernels s':>10} {'launches':>8} {'longest ms':>10} "
          f"{'phi call s':>10} {'phi kern s':>10} {'ratio':>6} {'|sum-R2|':>9}")
    for p in ps:
        d = problem(p)
        ls_spa_interactions(*d)
        t = time.perf_counter()
        res = ls_spa_interactions(*d)
        whole = time.perf_counter() - t
        eng.load_data(*d, 0.0)
        (_, info), phi_call, (phi_kern, _, _) = timed(eng.subsets_shapley, eng.subsets_timing)
        (_, _, info2), call, (kern, longest, launches) = timed(eng.subsets_interactions, eng.subsets_timing)
        eff = abs(res.interactions.sum() - res.r_squared)
        print(f"{p:>3} {whole:>9.4f} {call:>9.4f} {kern:>10.4f} {launches:>8} {longest * 1e3:>10.2f} "
              f"{phi_call:>10.4f} {phi_kern:>10.4f} {kern / phi_kern:>6.2f} {eff:>9.1e}"
              + ("  NOT_PD" if (info | info2) else ""), flush=True)
    eng.close()


if __name__ == "__main__":
    main([int(a) for a in sys.argv[1:]] or [16, 20, 24, 28, 30, 32])
