"""Time the exact pairwise interaction values between groups of columns (ls_spa_interactions(groups=labels)) beside the
grouped attribution alone (developer tool).

    python tools/group_interactions_time.py [g:p ...]        (default: 12:64 16:48 20:60 24:64)

The shapes are those of tools/groups_time.py (g:p:b puts b of the p columns into the baseline).  Per shape, in one process
on one engine: the whole ls_spa_interactions() call (reduction, full fit, enumeration; second call of the shape, kept
engine), the library call alone and the device time of its enumeration launches -- and the library call and device time
of groups_shapley on the same problem, with the ratio of the two device times."""
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "ls-spa_amd"))
import numpy as np  # noqa: E402,F401

from ls_spa import ls_spa_interactions  # noqa: E402
from ls_spa._engine import HipEngine  # noqa: E402
from groups_time import baseline_r2, labels_for, problem  # noqa: E402
from interactions_time import timed  # noqa: E402


def main(shapes):
    eng = HipEngine(0)
    print(f"{'g':>3} {'p':>3} {'base':>4} {'public s':>9} {'call s':>9} {'kernels s':>10} {'launches':>8} "
          f"{'longest ms':>10} {'phi call s':>10} {'phi kern s':>10} {'ratio':>6} {'|sum-dR2|':>9}")
    for g, p, b in shapes:
        d = problem(p)
        labels = labels_for(g, p, b)
        ls_spa_interactions(*d, groups=labels)
        t = time.perf_counter()
        res = ls_spa_interactions(*d, groups=labels)
        whole = time.perf_counter() - t
        eng.load_data(*d, 0.0)
        (_, info), phi_call, (phi_kern, _, _) = timed(lambda: eng.groups_shapley(labels), eng.groups_timing)
        (_, _, info2), call, (kern, longest, launches) = timed(lambda: eng.groups_interactions(labels),
                                                               eng.groups_timing)
        eff = abs(res.interactions.sum() - (res.r_squared - baseline_r2(d, labels)))
        print(f"{g:>3} {p:>3} {b:>4} {whole:>9.4f} {call:>9.4f} {kern:>10.4f} {launches:>8} {longest * 1e3:>10.2f} "
              f"{phi_call:>10.4f} {phi_kern:>10.4f} {kern / phi_kern:>6.2f} {eff:>9.1e}"
              + ("  NOT_PD" if (info | info2) else ""), flush=True)
    eng.close()


if __name__ == "__main__":
    args = sys.argv[1:] or ["12:64", "16:48", "20:60", "24:64"]
    main([(tuple(int(x) for x in a.split(":")) + (0,))[:3] for a in args])
