"""Timing of ls_spa_multi_sampled(groups=) against the column kernel and against the loop of ls_spa_groups calls, on one
MI355X, alone in the process:

    python tools/multi_groups_sampled_time.py [--json out.json] [--no-calls]

Per (p, g, baseline columns, m), N = M = 10^4, batches of 256 antithetical samples: the device time of the grouped batch's
lift launches and of its statistics launch (lsspa_multi_lift_timing), and beside it, in the same process, the same two
figures for the call WITHOUT a player map on the same 512 expanded rows with antithetical = 0 -- the same factorisations
and lift scans, p instead of g numbers written per response.  Each is measured `reps` times after two warm-up batches; the
median is reported with the spread (max - min) / median.  REQUIRED (the exit status says so): the grouped lift launches
take <= 1.03 x the ungrouped ones, and the grouped statistics launch is no slower than the ungrouped one beyond that 3 %.
Then, reported only, the whole call of ls_spa_multi_sampled(groups=) against the loop of m ls_spa_groups(perms=) calls
(the loop is timed over min(m, 20) calls and scaled)."""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ls-spa_amd"))

from ls_spa import ls_spa_groups, ls_spa_multi_sampled   # noqa: E402
from ls_spa._engine import HipEngine                     # noqa: E402

SHAPES = [(40, 10, 0), (100, 12, 4)]                     # (p, g, baseline columns)
MS = (8, 64)
BATCH = 256
SPREAD = 1.03                                            # the kernel's documented run-to-run spread


def problem(p, m, n=10000, rows=10000, seed=0):
    rng = np.random.default_rng(seed + p)
    Xa, Xe = rng.standard_normal((n, p)), rng.standard_normal((rows, p))
    W = rng.standard_normal((p, m)) / np.sqrt(p)
    return Xa, Xe, Xa @ W + rng.standard_normal((n, m)), Xe @ W + rng.standard_normal((rows, m))


def labels_of(p, g, n_base):
    """The baseline's columns first, the others dealt to the g groups in turn (no group contiguous)."""
    return np.concatenate([np.full(n_base, -1), np.arange(p - n_base) % g]).astype(np.int32)


def expand(labels, gperm, reverse):
    order = gperm[::-1] if reverse else gperm
    return np.concatenate([np.nonzero(labels == -1)[0]] + [np.nonzero(labels == k)[0] for k in order]).astype(np.int32)


def med_spread(v):
    v = np.asarray(v, dtype=np.float64)
    md = float(np.median(v))
    return md, float((v.max() - v.min()) / md) if md > 0 else 0.0


def batches(eng, perms, anti, reps):
    """(lift launches' ms, statistics launch's ms) of `reps` accumulated batches after two warm-ups."""
    batch, stats = [], []
    for i in range(reps + 2):
        eng.multi_lift_batch(perms, anti, want_lifts=False, accumulate=True)
        t = eng.multi_lift_timing()
        if i >= 2:
            batch.append(1e3 * t["batch"])
            stats.append(1e3 * t["stats"])
    return batch, stats


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--no-calls", action="store_true", help="skip the whole-call comparison")
    a = ap.parse_args()
    eng = HipEngine(0)
    rows, ok = [], True
    for p, g, n_base in SHAPES:
        labels = labels_of(p, g, n_base)
        rng = np.random.default_rng(p)
        gperms = np.array([rng.permutation(g) for _ in range(BATCH)], dtype=np.int32)
        expanded = np.array([expand(labels, gp, rev) for gp in gperms for rev in (False, True)], dtype=np.int32)
        for m in MS:
            Xa, Xe, Ya, Ye = problem(p, m)
            eng.multi_lift_load(Xa, Xe, Ya, Ye, 0.0)
            eng.multi_lift_set_players(labels)
            gb, gs = batches(eng, gperms, True, a.reps)
            eng.multi_lift_clear_players()
            cb, cs = batches(eng, expanded, False, a.reps)
            eng.multi_lift_free()
            (gb_md, gb_sp), (cb_md, cb_sp) = med_spread(gb), med_spread(cb)
            (gs_md, gs_sp), (cs_md, cs_sp) = med_spread(gs), med_spread(cs)
            row = {"p": p, "g": g, "baseline": n_base, "m": m, "batch": BATCH,
                   "grouped_batch_ms": gb_md, "grouped_batch_spread": gb_sp,
                   "columns_batch_ms": cb_md, "columns_batch_spread": cb_sp, "batch_ratio": gb_md / cb_md,
                   "grouped_stats_ms": gs_md, "grouped_stats_spread": gs_sp,
                   "columns_stats_ms": cs_md, "columns_stats_spread": cs_sp, "stats_ratio": gs_md / cs_md}
            row["batch_ok"] = bool(gb_md <= SPREAD * cb_md)
            row["stats_ok"] = bool(gs_md <= SPREAD * cs_md)
            ok = ok and row["batch_ok"] and row["stats_ok"]
            if not a.no_calls:
                kw = dict(perms=gperms, antithetical=True)
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    ls_spa_multi_sampled(Xa, Xe, Ya[:, :1], Ye[:, :1], groups=labels, _engine=eng, **kw)     # warm-up
                    ls_spa_groups(Xa, Xe, Ya[:, 0], Ye[:, 0], labels, tolerance=0.0, _engine=eng, **kw)
                    calls = []
                    for _ in range(3):
                        t = time.perf_counter()
                        ls_spa_multi_sampled(Xa, Xe, Ya, Ye, groups=labels, _engine=eng, **kw)
                        calls.append(time.perf_counter() - t)
                    k = min(m, 20)
                    loops = []
                    for _ in range(3):
                        t = time.perf_counter()
                        for r in range(k):
                            ls_spa_groups(Xa, Xe, Ya[:, r], Ye[:, r], labels, tolerance=0.0, _engine=eng, **kw)
                        loops.append((time.perf_counter() - t) * m / k)
                row.update({"call_multi_ms": 1e3 * min(calls), "call_loop_ms": 1e3 * min(loops),
                            "call_ratio": min(loops) / min(calls)})
            rows.append(row)
            print(json.dumps(row), flush=True)
    eng.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)
    print("REQUIRED: grouped lift launches <= 1.03 x ungrouped, grouped statistics no slower beyond 3 %:",
          "met" if ok else "NOT MET", flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
