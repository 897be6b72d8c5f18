"""Time the top-T list of best-subset selection over groups of columns (ls_spa_top_group_subsets) on one GPU (developer
tool).

    python tools/group_top_time.py

1. Kernels against the sibling: per (g, p) and T the device time of lsspa_groups_top's enumeration launches beside that
   of lsspa_groups_best's on the same problem and labels, in the same process, both from lsspa_groups_timing.  The two
   kernels share group_values and the launch geometry and differ in the per-subset bookkeeping only.  The ratio at T = 1
   must stay at or below LIMIT at g = 16, 20 and 24; the ratios at larger T are reported.  "rest ms" is the library
   call's wall time minus its enumeration launches: clearing the counts, the reduction kernel over the units' lists, the
   copies of the result.
2. The whole call against the route a user had before: ls_spa_top_group_subsets() beside debug_group_values over all 2^g
   masks followed by a host argpartition per size (kept engine, problem loaded).  The ratio must be below 1 at g = 16
   and 20.
Each side is timed REPS times alternately; the tables show the medians.  Exit status 1 if a required ratio fails."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "ls-spa_amd"))
import numpy as np  # noqa: E402

from ls_spa import ls_spa_top_group_subsets  # noqa: E402
from ls_spa._engine import HipEngine  # noqa: E402

REPS = 5
LIMIT = 1.05
SHAPES = ((12, 64), (16, 48), (20, 60), (24, 64))
KERNEL_T = (1, 4, 16)
GATED_G = (16, 20, 24)
ROUTE_G = (12, 16, 20)
REQUIRED_G = (16, 20)
ROUTE_T = 10


def problem(p, seed=0):
    rng = np.random.default_rng(seed)
    Xa, Xe = rng.standard_normal((4 * p + 100, p)), rng.standard_normal((2 * p + 50, p))
    w = rng.standard_normal(p) / np.sqrt(p)
    return Xa, Xe, Xa @ w + rng.standard_normal(len(Xa)), Xe @ w + rng.standard_normal(len(Xe))


def labels_of(g, p):
    return np.sort(np.arange(p) % g)                  # g groups of p // g or p // g + 1 columns, no baseline


def old_route(eng, labels, g, T):
    """What a user could do before: every value through the debug hook, then the T largest of every size on the host."""
    masks = np.arange(1 << g, dtype=np.uint64)
    u = eng.debug_group_values(labels, masks)
    size = np.zeros(1 << g, dtype=np.uint8)
    for j in range(g):
        size += ((masks >> np.uint64(j)) & np.uint64(1)).astype(np.uint8)
    out = []
    for k in range(g + 1):
        sel = np.nonzero(size == k)[0]
        if len(sel) > T:
            sel = sel[np.argpartition(-u[sel], T - 1)[:T]]
        out.append(sel[np.argsort(-u[sel], kind="stable")])
    return out


def kernels(eng):
    ok = True
    print(f"{'g':>3} {'p':>3} {'T':>3} {'launches':>8} {'top ms':>9} {'best ms':>9} {'ratio':>6} {'call s':>9} "
          f"{'rest ms':>8}")
    for g, p in SHAPES:
        labels = labels_of(g, p)
        eng.load_data(*problem(p), 0.0)
        eng.groups_best(labels)
        for T in KERNEL_T:
            eng.groups_top(labels, T)
            top_ms, best_ms, calls, rest = [], [], [], []
            for _ in range(REPS):
                t = time.perf_counter()
                _, _, _, info = eng.groups_top(labels, T)
                wall = time.perf_counter() - t
                k_s, _, launches = eng.groups_timing()
                calls.append(wall)
                top_ms.append(k_s * 1e3)
                rest.append((wall - k_s) * 1e3)
                eng.groups_best(labels)
                b_s, _, n = eng.groups_timing()
                best_ms.append(b_s * 1e3)
                assert n == launches, (n, launches)
            a, b = statistics.median(top_ms), statistics.median(best_ms)
            gated = T == 1 and g in GATED_G
            ok = ok and (not gated or a <= LIMIT * b)
            print(f"{g:>3} {p:>3} {T:>3} {launches:>8} {a:>9.3f} {b:>9.3f} {a / b:>6.3f} "
                  f"{statistics.median(calls):>9.4f} {statistics.median(rest):>8.3f}" + ("  (gated)" if gated else "")
                  + ("  NOT_PD" if info else ""), flush=True)
    return ok


def routes(eng):
    ok = True
    print(f"{'g':>3} {'p':>3} {'ls_spa_top_group_subsets s':>26} {'debug values + argpartition s':>29} {'ratio':>6}")
    for g, p in SHAPES:
        if g not in ROUTE_G:
            continue
        d, labels = problem(p), labels_of(g, p)
        res = ls_spa_top_group_subsets(*d, labels, n_best=ROUTE_T)     # first call of the shape: engine, buffers
        eng.load_data(*d, 0.0)
        old = old_route(eng, labels, g, ROUTE_T)
        for k in res.sizes:                                            # the two routes list the same models
            got = [sum(1 << int(j) for j in np.nonzero(s)[0]) for s in res.group_subsets[k, :res.n_models[k]]]
            assert sorted(got) == sorted(old[k].tolist()), (g, k)
        new_s, old_s = [], []
        for _ in range(REPS):
            t = time.perf_counter()
            ls_spa_top_group_subsets(*d, labels, n_best=ROUTE_T)
            new_s.append(time.perf_counter() - t)
            t = time.perf_counter()
            old_route(eng, labels, g, ROUTE_T)
            old_s.append(time.perf_counter() - t)
        a, b = statistics.median(new_s), statistics.median(old_s)
        required = g in REQUIRED_G
        ok = ok and (not required or a < b)
        print(f"{g:>3} {p:>3} {a:>26.4f} {b:>29.4f} {a / b:>6.3f}" + ("  (required < 1)" if required else ""),
              flush=True)
    return ok


def main():
    eng = HipEngine(0)
    ok = kernels(eng)
    ok = routes(eng) and ok
    eng.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
