"""The estimator driver: ``ls_spa(...)`` with the reference's signature and semantics,
running every ordering on the HIP engine in batches.

Reference: cvxgrp/ls-spa ``ls_spa/ls_spa.py:122-253``.  What is kept exactly:

* the 12 positional parameters, their order and defaults (:122-133);
* input coercion through ``np.array`` and ``validate_data`` (:158-162);
* ordering source selection (:169-177): ``perms is None`` and p < 9 -> every ordering,
  ``batch_size`` forced to 256, ``antithetical`` forced off; ``perms is None`` and p >= 9 ->
  ``rng.permutation`` drawn lazily from the SAME generator the error estimator uses;
  ``perms`` given -> consumed lazily, no sample cap;
* the error-check trigger indices ``i % batch_size == 0 or i == max_samples - 1``, the
  ``p >= 9`` guard, the tolerance break and the trailing estimate (:222-236).  Because the
  generator is only touched by the sampler between two checks, drawing a whole chunk of
  orderings up to the next check index and evaluating it as one GPU batch leaves the
  generator's call sequence -- hence every later ordering -- unchanged;
* results: running mean = attribution, biased covariance scaled as in :223-224.

README-dialect keywords (README.md:96-106) are accepted on top: ``method``,
``num_batches``, ``return_history``.
"""
from __future__ import annotations

import contextlib
import functools
import json
import os
import warnings

import numpy as np

from . import _samplers as S
from ._native import LSSPANativeError
from ._results import (CVBestGroupSubsetsResults, CVBestSubsetsResults, CVGroupPathResults, CVGroupResults, CVPathResults,
                       CVResults, BestGroupSubsetsBootstrapResults, BestGroupSubsetsResults, BestSubsetsBootstrapResults, BestSubsetsResults, BootstrapResults, InteractionBootstrapResults, InteractionResults, MultiGroupResults,
                       SampledBootstrapGroupResults, SampledBootstrapResults,
                       SampledCVGroupResults, SampledCVResults, SampledMultiGroupResults, SampledMultiResults,
                       MultiResponseResults, OwenResults, PermutationTestResults,
                       SampledInteractionResults, ShapleyResults, SizeIncompatible, TopGroupSubsetsCVResults, TopGroupSubsetsResults, TopSubsetsCVResults,
                       TopSubsetsResults, validate_data)
from ._stats import error_estimates, error_estimates_lowrank

# problems up to this many features take the one-workgroup-per-ordering kernels (csrc/k_small.hip small_p_eligible:
# p + 1 <= 128): one lane, look-ahead groups of up to sixteen chunks, larger sampler blocks
SMALL_P_MAX = 127


def auto_lookahead(p, per_rank):
    """Chunks of `per_rank` samples launched as one batch when nobody says otherwise (lookahead='auto').

    A chunk of fewer than 64 samples per rank leaves most of an MI355X idle at p = 1000 -- as many
    chunks as make up 64, eight at most.  Smaller problems need more samples to fill the chip (the work of an ordering
    goes with p^3, its tiles with p^2; bench.py at 128 samples a step, one against the best look-ahead: p = 150 0.67 ->
    0.93 M orderings/s at 8, p = 200 0.65 -> 0.91 at 8, p = 300 0.39 -> 0.45 at 4, p = 500 0.21 -> 0.23 at 4, p = 700 +2 %,
    p = 1000 -1 %): 1024 samples up to p = 250, 512 up to p = 800.  Small problems (the one-workgroup-per-ordering
    kernels): a group costs the host one call and the GPU ~45 us of dependent launches around its lift kernel whatever
    its size (statistics, estimator and checks of all its chunks are five launches), against 25 us of kernel per chunk
    of 128 samples at p = 100 -- as many chunks as make up 2048 samples, sixteen at most; a chunk of 1024 samples fills
    the chip four times over by itself."""
    per_rank = max(int(per_rank), 1)
    if p <= SMALL_P_MAX:
        return 1 if per_rank >= 1024 else max(1, min(16, 2048 // per_rank))
    want = 1024 if p <= 250 else (512 if p <= 800 else 64)
    return max(1, min(8, want // per_rank))

_NO_CAP = 2 ** 100

# ---- engines kept between calls ------------------------------------------------------------------------------------
# ls_spa() needs a context on the GPU and, for large p, tens of GB of per-batch workspace (C5: 80 GB).  Creating and
# releasing that on every call cost 2.3 of a C5 call's 2.9 seconds (profiles/r03_bench_c5.json: first_call_seconds
# against 0.61 s of work).  One process per GPU is the deployment model and HBM is sized for it, so the engine of a
# device -- context, stream, workspace -- stays alive between calls of one process and the next call of the same shape
# finds its buffers in place (a different shape re-sizes them, as before).  ``release()`` frees everything at once;
# LSSPA_ENGINE_CACHE=0 restores an engine per call.  A kept engine that is busy (another thread inside ls_spa on the same
# device) is not shared: that call makes its own.  The reference keeps no state between calls either way: every
# call resets the statistics, the history and the flags it touches.
_engine_cache = {}
_engine_cache_lock = __import__("threading").Lock()     # guards the table itself (two threads, one new device)


def _acquire_engine(device):
    """(engine, lock or None): a kept engine of this device if it is free, else a fresh one (lock None: caller closes it)."""
    import threading
    from ._engine import HipEngine
    if os.environ.get("LSSPA_ENGINE_CACHE", "1") == "0":
        return HipEngine(device), None
    with _engine_cache_lock:
        slot = _engine_cache.get(device)
        if slot is None:
            if not _engine_cache:
                import atexit
                atexit.register(release)
            slot = _engine_cache[device] = {"engine": None, "lock": threading.Lock()}
    if not slot["lock"].acquire(blocking=False):
        return HipEngine(device), None
    try:
        if slot["engine"] is None or getattr(slot["engine"], "_h", None) is None:
            slot["engine"] = HipEngine(device)
        return slot["engine"], slot["lock"]
    except BaseException:
        slot["lock"].release()
        raise


def release(device=None):
    """Close the engines ls_spa() keeps between calls (all of them, or one device's): frees their HBM."""
    with _engine_cache_lock:
        slots = list(_engine_cache.items())
    for dev, slot in slots:
        if device is not None and dev != device:
            continue
        if slot["lock"].acquire(blocking=False):
            try:
                if slot["engine"] is not None:
                    slot["engine"].close()
                slot["engine"] = None
            finally:
                slot["lock"].release()


def _next_check(i, batch_size, max_samples):
    """Smallest index > i at which the reference evaluates the error estimate."""
    nxt = (i // batch_size + 1) * batch_size
    if i < max_samples - 1 < nxt:
        nxt = max_samples - 1
    return nxt


class _Comm:
    """Single-process communicator (world of one)."""
    rank, world = 0, 1

    def allreduce_pending(self, engine):
        return None

    def allreduce_draws(self, engine):
        return None

    def allreduce_reduction(self, engine):
        return None

    def sum_ints(self, values):
        return [int(v) for v in values]

    def gather_ints(self, values):
        return [[int(v) for v in values]]

    def gather_lifts(self, local, counts):
        return local


def gather_ints_by_sum(comm, values):
    """Every rank's integer vector, [world][k], through the one integer collective a communicator has to offer
    (sum_ints): each rank writes its own slot of a zero vector, the sum is the concatenation."""
    k = len(values)
    flat = [0] * (comm.world * k)
    flat[comm.rank * k:(comm.rank + 1) * k] = [int(v) for v in values]
    total = comm.sum_ints(flat)
    return [total[r * k:(r + 1) * k] for r in range(comm.world)]


def _singular_fit(engine, X_test, y_test):
    """theta and r^2 when the full model's Gram matrix is numerically singular (full_fit's info bit 1)."""
    G, g, _, _ = engine.gram()
    theta = _min_norm_theta(G, g)
    yy = engine.y_norm_sq
    if engine.tri:      # from the Gram side: also right when the test rows are sharded
        _, _, H, h = engine.gram()
        r_squared = float((2.0 * (h @ theta) - theta @ H @ theta) / yy)
    else:
        pred = X_test.astype(np.float64) @ theta
        r_squared = float((2.0 * (pred @ y_test) - pred @ pred) / yy)
    return theta, r_squared


def _min_norm_theta(G, g):
    """theta of minimal norm for a numerically singular Gram matrix (the reference gets it
    from lstsq on the triangular factor, ls_spa/ls_spa.py:240)."""
    from ._stats import host_blas_threads
    with host_blas_threads():
        w, Q = np.linalg.eigh(G)
    keep = w > w.max() * G.shape[0] * np.finfo(float).eps
    coef = np.zeros_like(w)
    coef[keep] = (Q.T @ g)[keep] / w[keep]
    return Q @ coef


# 3: the identity carries `history`, `precision` and `data`, the state `attribution_history` / `history_sum` (round 3);
# 4: the device estimator's state is its running sums (err_D, err_s) instead of the lift history (round 5);
# a file of another version is refused by name instead of failing on a missing key.  With return_attribution_history the
# whole n x p history is rewritten at every save (I/O quadratic in the run length): checkpoint long history runs sparsely.
_CKPT_VERSION = 4


def _ckpt_path(path, comm):
    return path if comm.world == 1 else f"{path}.rank{comm.rank}"


def _save_checkpoint(path, comm, state):
    """Atomic write (temp file + rename) of the estimator state; one file per rank.  The file it replaces is
    kept as ``<file>.prev``: the ranks write after the same check but not at the same instant, so a job killed
    between two ranks' renames leaves them one generation apart -- the older one is then the common state."""
    target = _ckpt_path(path, comm)
    tmp = target + ".tmp.npz"
    np.savez(tmp, **state)
    if os.path.exists(target):
        os.replace(target, target + ".prev")
    os.replace(tmp, target)


def _read_checkpoint(target, expect):
    if not os.path.exists(target):
        return None
    with np.load(target, allow_pickle=False) as z:
        st = {k: z[k] for k in z.files}
    if int(st["version"]) != _CKPT_VERSION:
        raise ValueError(f"checkpoint {target}: unsupported version {int(st['version'])}")
    for key, want in expect.items():
        have = st[key].item() if st[key].shape == () else st[key]
        if str(have) != str(want):
            raise ValueError(f"checkpoint {target} was written with {key}={have}, this run has {key}={want}")
    return st


def _load_checkpoint(path, comm, expect):
    """The state to resume from, or None.  With several ranks the ranks first agree on it: each reports the sample
    counts of the (at most two) generations it holds and all resume from the largest count EVERY rank holds;
    if there is none -- a rank without a file next to ranks with files, files of different runs -- every rank
    raises the same error instead of running chunks that no longer pair up in the collectives.

    Nothing raises before that exchange: a rank whose own file is unreadable or belongs to another run (other
    seed, data, sampler ...) reports it through the collective, and then ALL ranks raise -- a rank raising alone
    would leave the others waiting in the all-reduce.  A stale or foreign ``.prev`` next to a valid file is
    ignored (it is only ever the fallback generation)."""
    target = _ckpt_path(path, comm)
    gens, target_problem = [], None
    for k, f in enumerate((target, target + ".prev")):
        try:
            st = _read_checkpoint(f, expect)
        except Exception as exc:     # unreadable archive, missing key, version or ident mismatch
            st = None
            if k == 0:
                target_problem = f"{exc}"
        if st is not None:
            gens.append(st)
    if comm.world == 1:
        if target_problem is not None:
            raise ValueError(target_problem)
        return gens[0] if gens else None
    mine = ([int(st["n"]) for st in gens] + [-1, -1])[:2] + [0 if target_problem is None else 1]
    table = comm.gather_ints(mine)
    bad = [r for r, row in enumerate(table) if row[2]]
    if bad:
        raise ValueError(f"checkpoint {path}: the file of rank(s) {bad} is unreadable or was written by another run"
                         + (f" ({target_problem})" if target_problem is not None else "")
                         + "; remove the files to start over")
    held = [set(v for v in row[:2] if v >= 0) for row in table]
    if not any(held):
        return None
    common = set.intersection(*held)
    if not common:
        raise ValueError(f"checkpoint {path}: the ranks hold no common state (sample counts per rank: "
                         f"{[sorted(h) for h in held]}); remove the files to start over")
    n = max(common)
    return next(st for st in gens if int(st["n"]) == n)


def _data_fingerprint(engine):
    """A few numbers of the reduced problem that change with the data, the row count or reg."""
    G, g, _, _ = engine.gram()
    return f"{float(np.trace(G))!r}/{float(g @ g)!r}/{float(engine.y_norm_sq)!r}"


def prepare_sampling(p, *, max_samples, batch_size, seed, perms, antithetical, method, rank=0, world=1):
    """Generator and ordering source of a run, with the reference's overrides for small p applied
    (ls_spa/ls_spa.py:169-177).  Split from run_estimator so that ls_spa() can start it -- the QMC
    constructors work on a helper thread -- before the data reduction instead of after it."""
    rng = np.random.default_rng(seed)
    never_stop = False
    if perms is not None:
        if method is not None:
            raise ValueError("pass either perms= or method=, not both")
        source, max_samples = S.IterableSource(perms, p), _NO_CAP
    elif method is None:
        if p < 9:
            # the reference's loop runs over all p! orderings here; max_samples only ever enters
            # the (p >= 9)-guarded error check (:222), so it does not cap this case
            source, batch_size, antithetical, max_samples = S.exact_source(p), 2 ** 8, False, _NO_CAP
        else:
            source = S.RandomSource(rng, p, max_samples)
    elif method == "exact":
        source, batch_size, antithetical, never_stop = S.exact_source(p), 2 ** 8, False, True
        max_samples = _NO_CAP
    elif method == "random":
        source = S.RandomSource(rng, p, max_samples)
    elif method == "argsort":
        # a thread of the library draws the orderings ahead (no interpreter lock between it and this thread; SciPy's
        # engine still defines the stream); the Python source and its helper thread if that cannot be had
        source = (S.NativeArgsortSource.make(p, seed, max_samples, block=1024 if p <= SMALL_P_MAX else 256, rank=rank,
                                             world=world)
                  or S.ArgsortSource(p, seed, max_samples))
    elif method == "permutohedron":
        source = S.PermutohedronSource(p, seed, max_samples)
    else:
        raise ValueError(f"method must be one of {S.METHODS + ('subsets',)} or None")
    if source.independent:
        # the QMC samplers draw ahead of the loop on a helper thread (their stream is nobody else's), from now on --
        # in ls_spa() that is under the data reduction
        if not isinstance(source, S.NativeArgsortSource):
            source = S.PrefetchedSource(source, block=1024 if p <= SMALL_P_MAX else 256, rank=rank, world=world)
    return rng, source, batch_size, antithetical, max_samples, never_stop


def run_estimator(engine, p, *, max_samples, batch_size, tolerance, seed, perms, antithetical,
                  return_attribution_history, method, error_estimator, comm=None, chunk_cap=None,
                  checkpoint=None, prepared=None, lookahead=1, timings=None, defer=None, cost_p=None):
    """The sampling loop on an engine whose problem is already loaded.  Returns
    (attribution, attribution_errors, overall_error, error_history, attribution_history, n).

    p is the dimension of a sample.  With groups of columns as the players (ls_spa_groups: the engine carries a player
    map) that is the number of groups g, and cost_p is the number of columns: what an ordering costs, hence the sizes of
    the automatic look-ahead groups and the decision to defer checks, follows the columns.

    checkpoint: path of a state file.  Written after every error check (sample count, running mean and
    covariance, generator state, error history, the lift history the thin-form estimators need); if it
    exists when the call starts, the run continues from it -- the orderings, the estimator's draws and
    therefore every later number are those of the uninterrupted run.

    timings: optional dict; receives the host seconds spent drawing orderings ('sampler'), in the estimator calls
    ('estimator', reads of the statistics included) and in everything else of the loop ('sampling')."""
    import time as _time
    t_loop0 = _time.perf_counter()
    comm = comm or _Comm()
    if prepared is None:
        prepared = prepare_sampling(p, max_samples=max_samples, batch_size=batch_size, seed=seed, perms=perms,
                                    antithetical=antithetical, method=method, rank=comm.rank, world=comm.world)
    rng, source, batch_size, antithetical, max_samples, never_stop = prepared
    if batch_size < 1:
        raise ValueError("batch_size must be positive")
    try:
        return _run_estimator(engine, p, comm, rng, source, batch_size, antithetical, max_samples, never_stop,
                              tolerance=tolerance, seed=seed, return_attribution_history=return_attribution_history,
                              method=method, error_estimator=error_estimator, chunk_cap=chunk_cap,
                              checkpoint=checkpoint, lookahead=lookahead, timings=timings, defer=defer,
                              t_loop0=t_loop0, cost_p=p if cost_p is None else int(cost_p))
    finally:
        if hasattr(source, "close"):
            source.close()


def _run_estimator(engine, p, comm, rng, source, batch_size, antithetical, max_samples, never_stop, *, tolerance, seed,
                   return_attribution_history, method, error_estimator, chunk_cap, checkpoint, lookahead, timings,
                   defer, t_loop0, cost_p):
    import time as _time
    t_sampler = t_estimator = 0.0

    estimate = p >= 9
    keep_lifts = return_attribution_history or error_estimator == "lowrank"
    # one rank: nothing to all-reduce between a chunk's moments and their merge -- the engine folds the chunk into the
    # running statistics at once (accumulate = 2; one launch instead of two plus the merge call for small p)
    single = comm.world == 1 and not getattr(comm, "_force", False)
    acc_mode = 2 if single else True
    engine.reset_stats()
    on_device = error_estimator == "device" and estimate
    if on_device:
        # the running form (include/lsspa.h): D = Xi L and s = Xi 1 stay in HBM, Xi a function of (seed, sample, draw)
        engine.error_running_enable(int(np.random.SeedSequence(seed).generate_state(1, np.uint64)[0]))
    feat_err, total_err = np.zeros(p), 0.0
    err_hist, hist_parts, lift_parts = [], [], []
    hist_sum = np.zeros(p)
    i, pending, stop = 0, False, False
    mean = np.zeros(p)
    cov = None

    ident = {"p": p, "seed": seed, "method": str(method), "batch_size": batch_size,
             "antithetical": bool(antithetical), "error_estimator": error_estimator, "world": comm.world}
    if checkpoint is not None:
        ident["history"] = bool(return_attribution_history)
        ident["precision"] = str(getattr(engine, "precision", "float64"))
        ident["data"] = _data_fingerprint(engine)
        st = _load_checkpoint(checkpoint, comm, ident)
        if st is not None:
            i = int(st["n"])
            mean = st["mean"]
            engine.set_stats(i, mean, st["cov_biased"])
            rng.bit_generator.state = json.loads(str(st["rng_state"]))
            source.skip(i)
            err_hist = [float(v) for v in st["error_history"]]
            feat_err, total_err = st["feature_errors"], float(st["overall_error"])
            if return_attribution_history:
                hist_parts.append(st["attribution_history"])
                hist_sum = st["history_sum"]
            if error_estimator == "lowrank":
                lift_parts.append(st["lifts"])
            elif on_device:
                engine.set_error_state(st["err_D"], st["err_s"])
            if (i >= max_samples or (estimate and err_hist and total_err < tolerance and not never_stop)):
                stop = True   # the saved run had already finished

    def save_now(n):
        state = dict(ident, version=_CKPT_VERSION, n=n, rng_state=json.dumps(rng.bit_generator.state),
                     error_history=np.array(err_hist), feature_errors=feat_err, overall_error=total_err)
        _, state["mean"], state["cov_biased"] = engine.stats(want_cov=True)
        if return_attribution_history:
            state["attribution_history"] = np.concatenate(hist_parts) if hist_parts else np.zeros((0, p))
            state["history_sum"] = hist_sum
        if error_estimator == "lowrank":
            state["lifts"] = np.concatenate(lift_parts) if lift_parts else np.zeros((0, p))
        elif on_device:
            state["err_D"], state["err_s"] = engine.error_state()
        _save_checkpoint(checkpoint, comm, state)

    # lookahead > 1 (QMC samplers only: their stream is nobody else's): the orderings of several chunks are launched
    # as ONE batch -- a chunk of batch_size / world samples may fill a fraction of the GPU -- and then accumulated,
    # all-reduced and checked chunk by chunk in the reference's order (ls_spa/ls_spa.py:212-230).  When the stop
    # rule fires, the chunks launched beyond it are dropped: nothing of them ever reaches the statistics.  With a
    # host-side estimator the next group is launched AFTER the statistics of the group's last chunk have been read
    # back and BEFORE the host's estimate and decision, so the GPU works while the host computes (a stop then
    # wastes up to k chunks of GPU work, which only the final read-back waits for).  With the device-side estimator the
    # checks are enqueued behind the chunks' statistics and read late (below): the next group is launched when the
    # current one has been taken up, whatever its checks will say.
    ramp = None
    if lookahead == "auto":
        lookahead = auto_lookahead(cost_p, -(-int(batch_size) // comm.world))
        # the automatic groups grow: 1, 2, 4, ... chunks up to the size above.  A run that stops at one of its first checks
        # -- the usual run to a tolerance -- then has its answer after about as many chunks as it needed, not after a
        # whole group (its kernels are one launch: none of its checks is known before all of its chunks have run); a long
        # run is at the full size after log2 of it groups.  An explicit lookahead = k is k from the first group on.
        ramp = [1]
    group = max(1, int(lookahead)) if (hasattr(engine, "launch_batch") and source.independent and not chunk_cap) else 1
    # The device estimator's checks are ENQUEUED, not waited for: x = (D - s mean^T) / sqrt(n (n - 1)), the all-reduce of
    # the per-rank x, the quantile kernels and a copy of (errors, running mean, n) into a pinned slot run on the context's
    # stream behind the chunk's statistics.  `defer` checks may be outstanding: the stop rule of check k is evaluated
    # when check k + defer has been enqueued -- the samples in between are already running and are dropped on a stop,
    # the results are those of check k (its own copy of the running mean) -- so the host never waits for the newest
    # work and the estimator is off the critical path.  The FIRST check of a run is always waited
    # for (a run on easy data ends there with nothing wasted), and a chunk that takes tens of milliseconds is too
    # (the round trip of a check is 0.2 ms: nothing to hide, and up to defer + 1 such chunks would run for nothing).
    # The point at which a check is resolved depends on counts only, never on timing: every rank takes the same decisions.
    outstanding = []     # (sample count, slot), oldest first
    slot_turn = [0]
    can_defer = on_device and checkpoint is None and source.independent and not chunk_cap
    if defer is None:
        per_rank = -(-min(int(batch_size), max_samples) // comm.world) * (2 if antithetical else 1)
        # a chunk's kernels, at 40 TFLOP/s, under 50 ms; the chunks of a look-ahead group are checked without waiting
        # in between (their kernels were one launch)
        defer = min(max(1, group), engine.RESULT_SLOTS - 2) if (can_defer and per_rank * float(cost_p) ** 3 / 4e13 < 0.05) else 0
    defer = int(defer) if can_defer else 0
    if not 0 <= defer < engine.RESULT_SLOTS - 1 if on_device else False:
        raise ValueError("defer must be between 0 and the number of result slots - 2")

    def enqueue_check(n):
        slot = slot_turn[0]
        slot_turn[0] = (slot + 1) % engine.RESULT_SLOTS
        if single and hasattr(engine, "error_check_enqueue"):
            engine.error_check_enqueue(n, slot)      # one rank: nothing to all-reduce, the draws are never written
        else:
            engine.error_running_draws(n)
            comm.allreduce_draws(engine)
            engine.error_quantiles_enqueue(slot)
        outstanding.append((n, slot))

    def estimate_now(n, cov_b=None):
        nonlocal feat_err, total_err, t_estimator
        t_e0 = _time.perf_counter()
        with np.errstate(divide="ignore", invalid="ignore"):
            if error_estimator == "lowrank":
                centred = np.concatenate(lift_parts) - mean
                feat_err, total_err = error_estimates_lowrank(rng, centred, n)
            elif on_device:
                enqueue_check(n)
                feat_err, total_err, _, _ = engine.error_result(outstanding.pop()[1], wait=True)
            else:
                if cov_b is None:
                    _, _, cov_b = engine.stats(want_cov=True)
                feat_err, total_err = error_estimates(rng, cov_b * n / (n - 1) / n)
        err_hist.append(total_err)
        t_estimator += _time.perf_counter() - t_e0

    # Two lanes (engine.lanes == 2, set by ls_spa() on the general path for the QMC samplers): successive groups run on
    # two workspaces and two streams, the statistics on the context's own.  The next group is then launched as soon as
    # the current one's last chunk is taken up -- BEFORE its statistics are read back: the read-back waits for the
    # context's stream only, and the next group's kernels start when the current group's are half way (6.25 against
    # 6.45 ms a step at the C3 shape).  A stop wastes at most that one group, which is discarded.
    prefetch = (getattr(engine, "lanes", 1) == 2 and hasattr(engine, "launch_batch") and source.independent
                and not chunk_cap)
    # ... and a chunk goes to the engine as two half-chunks, each its own launch sequence on its own lane, once a half
    # still fills the chip (>= 32 samples = 64 orderings per rank): a finer-grained pipeline (6.18 against 6.37 ms a
    # step at the C3 shape).  The check indices are untouched -- a half-chunk that ends between two of them triggers
    # nothing -- and the statistics are folded in half-chunk by half-chunk, in order: the results differ from the
    # one-lane run's by the rounding of that grouping (1e-16 relative), nothing else.
    sub_cap = None
    if prefetch and group == 1 and -(-(int(batch_size) + 1) // 2 // comm.world) >= 32:
        sub_cap = (int(batch_size) + 1) // 2
    queue = []
    group_of = {}      # id(ticket) -> chunks launched with it: as many checks may be outstanding behind one of them

    def allowed(ticket):
        """Checks that may stay unread once a check of this ticket's group has been enqueued: the group's own (their
        kernels were one launch), `defer` at most."""
        return defer if (ramp is None or ticket is None) else max(min(defer, group_of.get(id(ticket), defer)), 1 if defer else 0)

    def refill(i_now):
        nonlocal t_sampler
        entries, cursor = [], i_now
        size = group
        if ramp is not None:
            size = min(group, ramp[0])
            ramp[0] *= 2
        for _ in range(size):
            if cursor >= max_samples:
                break
            target = _next_check(cursor, batch_size, max_samples)
            want = min(target, max_samples) - cursor
            if chunk_cap:
                want = min(want, chunk_cap)
            if sub_cap:
                want = min(want, sub_cap)
            t_s0 = _time.perf_counter()
            # sample number g of the run belongs to rank g mod world (round 5; up to round 4 the dealing restarted with
            # every chunk): a QMC source then draws -- ahead of the loop -- this rank's orderings only
            n_got, mine_rows = source.take_share(want, cursor, comm.rank, comm.world)
            t_sampler += _time.perf_counter() - t_s0
            if n_got == 0:
                break
            entries.append([n_got, mine_rows, want])
            cursor += n_got
            if n_got < want:
                break
        ticket = None
        if (group > 1 or prefetch) and entries:
            mine_all = np.concatenate([e[1] for e in entries])
            if len(mine_all):
                ticket = engine.launch_batch(mine_all, antithetical)
        first = 0
        for e in entries:
            e += [ticket, first]
            first += len(e[1])
        if ticket is not None:
            group_of[id(ticket)] = len(entries)
        queue.extend(entries)

    # the whole group in one library call: device estimator with its checks deferred by a group at least, nothing that
    # needs a chunk's lift vectors on the host, and moments that travel through the engine's own communicator (or not
    # at all)
    fast_group = (on_device and defer >= group and defer > 0 and not keep_lifts and checkpoint is None
                  and hasattr(engine, "group_collect")
                  and (single or getattr(comm, "_engine", None) is engine))
    stopped_at = None      # (mean, n) of the check whose stop rule fired (device estimator)
    resolved = [0]

    def resolve_due(limit):
        """Read the oldest outstanding checks until at most `limit` are left (the first check of a run is always read,
        whatever the limit); True if one of them stops the run."""
        nonlocal feat_err, total_err, stopped_at, t_estimator
        while outstanding and (len(outstanding) > limit or not resolved[0]):
            t_e0 = _time.perf_counter()
            n_k, slot = outstanding.pop(0)
            feat_err, total_err, mean_k, _ = engine.error_result(slot, wait=True)
            err_hist.append(total_err)
            resolved[0] += 1
            t_estimator += _time.perf_counter() - t_e0
            if total_err < tolerance and not never_stop:
                stopped_at = (mean_k, n_k)
                outstanding.clear()      # later checks: of samples the reference would never have drawn
                return True
        return False

    while not stop:
        if not queue:
            refill(i)
        if not queue:
            break
        n_new, mine, want, ticket, first = queue.pop(0)
        if fast_group and ticket is not None:
            # every chunk of the launched group in ONE call into the library (lsspa_group_collect): collect, all-reduce
            # and merge, fold into the estimator, enqueue the check -- per chunk, in the reference's order; at p = 100 a
            # chunk is 37 us of GPU work and this loop's own calls were what a run waited for
            members = [(n_new, mine, want, ticket, first)]
            while queue and queue[0][3] is ticket:
                members.append(tuple(queue.pop(0)))
            if (all(m[0] == m[2] for m in members)
                    and len(outstanding) + len(members) < engine.RESULT_SLOTS):
                t_g0 = _time.perf_counter()
                cursor = i
                if prefetch and not queue:
                    refill(i + sum(m[0] for m in members))      # the next group, on the other lane
                firsts, counts, ids, n_after, slots = [], [], [], [], []
                for n_ch, mn, _, _, fs in members:
                    firsts.append(fs)
                    counts.append(len(mn))
                    ids.append(cursor + (comm.rank - cursor) % comm.world)      # this rank's first sample of the chunk
                    cursor += n_ch
                    due = estimate and (cursor % batch_size == 0 or cursor == max_samples - 1)
                    n_after.append(cursor if due else 0)
                    slots.append(slot_turn[0] if due else 0)
                    if due:
                        slot_turn[0] = (slot_turn[0] + 1) % engine.RESULT_SLOTS
                engine.group_collect(ticket, firsts, counts, ids, comm.world, n_after, slots)
                outstanding.extend((n_a, sl) for n_a, sl in zip(n_after, slots) if n_a)
                i, pending = cursor, n_after[-1] == 0
                halt = resolve_due(allowed(ticket))
                if timings is not None and "check_s" in timings:
                    k = max(1, sum(1 for v in n_after if v))
                    timings["check_s"].extend([(_time.perf_counter() - t_g0) / k] * k)
                if halt or i >= max_samples:
                    break
                continue
            for m in reversed(members[1:]):      # a chunk cut short by a dry source: chunk by chunk below
                queue.insert(0, list(m))
        if prefetch and not queue and ticket is not None and n_new == want:
            refill(i + n_new)      # the next group, on the other lane
        local = None
        if len(mine):
            if ticket is not None:
                local = engine.collect_batch(ticket, want_lifts=keep_lifts, accumulate=acc_mode, first=first,
                                             count=len(mine))
            else:
                local = engine.run_batch(mine, antithetical, want_lifts=keep_lifts, accumulate=acc_mode)
            if on_device:
                # this rank's samples of the chunk: every world-th sample of the run from its first one at or after i
                engine.error_advance(i + (comm.rank - i) % comm.world, comm.world)
        if not single:
            comm.allreduce_pending(engine)
            engine.merge()
        if keep_lifts:
            offs = [(r - i) % comm.world for r in range(comm.world)]      # rank r's first position in this chunk
            counts = [len(range(offs[r], n_new, comm.world)) for r in range(comm.world)]
            parts = comm.gather_lifts(local if local is not None else np.empty((0, p)), counts)
            if comm.world > 1:
                full = np.empty((n_new, p))
                for r in range(comm.world):
                    full[offs[r]::comm.world] = parts[r]
            else:
                full = parts
            if return_attribution_history:
                run = hist_sum + np.cumsum(full, axis=0)
                hist_parts.append(run / np.arange(i + 1, i + n_new + 1)[:, None])
                hist_sum = run[-1]
            if error_estimator == "lowrank":
                lift_parts.append(full)
        i += n_new
        pending = True
        if n_new < want and not chunk_cap:
            stop = True  # the source ran dry inside a chunk
        check = estimate and (i % batch_size == 0 or i == max_samples - 1)
        if check and on_device:
            t_e0 = _time.perf_counter()
            enqueue_check(i)
            t_estimator += _time.perf_counter() - t_e0
            pending = False
            halt = resolve_due(allowed(ticket))
            if timings is not None and "check_s" in timings:
                timings["check_s"].append(_time.perf_counter() - t_e0)
            if halt:
                break
            if checkpoint is not None:       # (defer is 0 with a checkpoint: the engine's state is check i's)
                _, mean, _ = engine.stats(want_cov=False)
                save_now(i)
        elif check:
            t_e0 = _time.perf_counter()
            _, mean, cov_now = engine.stats(want_cov=error_estimator == "reference")
            t_estimator += _time.perf_counter() - t_e0
            if group > 1 and not queue and not stop and i < max_samples:
                refill(i)      # in flight while the host evaluates the stop rule below
            estimate_now(i, cov_now)
            pending = False
            if checkpoint is not None:
                save_now(i)
            if total_err < tolerance and not never_stop:
                break
        if i >= max_samples:
            break
    for tk in {id(e[3]): e[3] for e in queue if e[3] is not None}.values():
        engine.discard_batch(tk)     # launched, never accumulated

    if stopped_at is None:
        resolve_due(0)               # the run ended with checks still outstanding: they are read in order
    if stopped_at is not None:
        # the engine's statistics may have moved on by up to `defer` checks' samples: the run's results are the
        # stopping check's own copies
        mean, n = stopped_at
        if return_attribution_history and hist_parts:
            hist_parts = [np.concatenate(hist_parts)[:n]]
    else:
        n, mean, _ = engine.stats(want_cov=False)
        if estimate and pending and n > 0:
            estimate_now(n)
    history = None
    if return_attribution_history:
        history = np.concatenate(hist_parts) if hist_parts else np.zeros((0, p))
    if timings is not None:
        timings["sampler"] = timings.get("sampler", 0.0) + t_sampler
        timings["estimator"] = timings.get("estimator", 0.0) + t_estimator
        timings["sampling"] = timings.get("sampling", 0.0) + (_time.perf_counter() - t_loop0) - t_sampler - t_estimator
    return mean, feat_err, total_err, np.array(err_hist), history, n


# ---- what every entry point does round its GPU work ------------------------------------------------------------------
def _coerce_data(X_train, X_test, y_train, y_test):
    """The four arrays as ndarrays, their shapes checked.  The reference coerces with np.array (a copy,
    ls_spa/ls_spa.py:158-161); the inputs are never written here, so asarray gives the same result without copying
    1.6 GB at the C3 shape."""
    X_train, X_test = np.asarray(X_train), np.asarray(X_test)
    y_train, y_test = np.asarray(y_train), np.asarray(y_test)
    validate_data(X_train, X_test, y_train, y_test)
    if y_train.ndim != 1 or y_test.ndim != 1:
        raise ValueError("y_train and y_test must be one-dimensional")  # reference: concatenate error, :312
    return X_train, X_test, y_train, y_test


def _sampling_options(method, perms, p, error_estimator=None, lookahead=None, lanes="auto"):
    """(error_estimator, lookahead, lanes) of a sampling call of ls_spa with what the caller left open filled in: the
    defaults ls_spa's docstring gives, keyed on whether the orderings come from a QMC method; p is the number of
    columns.  ValueError for a value that is none of the documented ones."""
    qmc = perms is None and method in ("argsort", "permutohedron")
    if error_estimator is None:
        error_estimator = "device" if qmc else "reference"
    if error_estimator not in ("reference", "lowrank", "device"):
        raise ValueError("error_estimator must be None, 'reference', 'lowrank' or 'device'")
    if lookahead is None:
        # the device estimator's checks never make the loop wait: launching the chunks of a thin batch together costs
        # nothing but the samples already in flight at a stop
        lookahead = "auto" if (error_estimator == "device" and qmc) else 1
    if lookahead != "auto" and int(lookahead) < 1:
        raise ValueError("lookahead must be >= 1 or 'auto'")
    if lanes == "auto":
        lanes = 2 if (qmc and p > SMALL_P_MAX) else 1
    if int(lanes) not in (1, 2):
        raise ValueError("lanes must be 1, 2 or 'auto'")
    return error_estimator, lookahead, int(lanes)


def _stopwatch(tm):
    """lap(key): the host seconds since the last lap are added to tm[key]; lap() only starts the next one."""
    from time import perf_counter
    mark = [perf_counter()]

    def lap(key=None):
        if key is not None:
            tm[key] = tm.get(key, 0.0) + (perf_counter() - mark[0])
        mark[0] = perf_counter()
    return lap


def _close_source(source):
    if hasattr(source, "close"):
        source.close()


@contextlib.contextmanager
def _engine_call(engine, device, comm=None, undo=(), lap=lambda key=None: None):
    """The engine of one call of an entry point: the caller's (`engine`), else the device's kept engine or one made for
    the call (_acquire_engine), with `comm` bound to it.  undo: (function, always) pairs, a list the body may extend,
    called in order on the way out: all of them after success, after an exception those marked `always`.  An engine that
    is not the caller's then loses its communicator and is reset for the next call -- a kept one, if neither the body nor
    an undo step raised -- or closed; its lock is released whatever the teardown does.  lap: ls_spa's stopwatch."""
    owns, lock, ok = engine is None, None, False
    try:
        if owns:
            engine, lock = _acquire_engine(device)
        lap("engine_create")
        if comm is not None and hasattr(comm, "bind"):
            comm.bind(engine)      # RCCL communicator on this engine's GPU and stream (collective)
        yield engine
        ok = True
    finally:
        lap()
        try:
            try:
                for step, always in undo:
                    if ok or always:
                        step()
            except BaseException:
                ok = False      # what may still carry a player map or pair tables is not handed to the next call
                raise
            finally:
                if owns and engine is not None:
                    if comm is not None and hasattr(comm, "close"):
                        comm.close()       # the communicator lives on the engine's context
                    if lock is None or not ok:
                        engine.close()     # a kept engine an exception went through is not trusted with another call
                    else:
                        engine.set_flags(0)
                        if engine.p:                  # (no problem loaded -- ls_spa_multi on a fresh engine --: no history)
                            engine.history_enable(0)  # (the lanes stay as they are: the next call sets what it needs)
        finally:
            if lock is not None:
                lock.release()
        lap("teardown")


def _load_and_fit(engine, data, reg, row_sharded, comm, lap=lambda key=None: None):
    """The data reduction (of this rank's rows, with row_sharded), then the full fit: (theta, r_squared, info)."""
    if row_sharded:
        engine.load_data_sharded(*data, reg, comm or _Comm(), shard_test=row_sharded != "train")
    else:
        engine.load_data(*data, reg)
    lap("reduction_h2d_gram")
    fit = engine.full_fit()
    lap("final_fit")
    return fit


def _engine_fault(bits):
    """LSSPA_INFO_SCAN_WAIT (4): a hand-over inside a panel launch timed out; LSSPA_INFO_SUM (8): a sample's lifts did
    not sum to the R^2 of the full model (every ordering's must, ls_spa/ls_spa.py:284-285).  Either way the lift vectors
    of the run are not valid (with a pivot that broke down, bit 1, they are meaningless anyway)."""
    return bool(bits & 12) and not bits & 1


def _info_verdict(bits, stacklevel):
    """What the info bits of a finished run mean to the caller: LSSPANativeError for an engine fault, a RuntimeWarning
    (attributed `stacklevel` frames above the function that asks) for a Gram matrix that was not positive definite."""
    if _engine_fault(bits):
        raise LSSPANativeError(
            ("the fused lift scan gave up waiting for a row of its panel" if bits & 4 else
             "a sample's lifts did not sum to the R^2 of the full model")
            + f" (info bits {bits}): the lift vectors of this run are not valid (engine fault)")
    if bits & 1:
        warnings.warn("a permuted Gram matrix was not numerically positive definite; the attribution "
                      "of collinear features is not meaningful (the reference's is not either)",
                      RuntimeWarning, stacklevel=stacklevel + 1)


def _shap_matrix(phi, index):
    """SHAP's matrix of an interaction index: half the index off the diagonal, the main effect
    phi_i - sum_{j != i} Phi_ij on it, so that row i sums to phi_i."""
    Phi = 0.5 * np.asarray(index, dtype=np.float64)
    np.fill_diagonal(Phi, 0.0)
    np.fill_diagonal(Phi, phi - Phi.sum(axis=1))
    return Phi


def ls_spa(X_train, X_test, y_train, y_test, reg=0., max_samples=2 ** 13, batch_size=2 ** 8,
           tolerance=1e-2, seed=42, perms=None, antithetical=True, return_attribution_history=False, *,
           method=None, num_batches=None, return_history=None, device=0, error_estimator=None,
           precision="float64", row_sharded=False, checkpoint=None, comm=None, lookahead=None, lanes="auto",
           groups=None, _engine=None, _comm=None, _timings=None, _defer=None, _players=None):
    """Estimates the Shapley attribution of the out-of-sample R^2 of a least-squares fit.

    Positional parameters, defaults and behaviour follow cvxgrp/ls-spa
    (``ls_spa/ls_spa.py:122-253``).  One difference in what stays behind: the engine of the device -- its context, stream
    and per-batch workspace in HBM (gigabytes for large p) -- is kept alive between calls of a process, so that the
    next call of the same shape starts at once; ``ls_spa.release()`` (or ``release(device)``) frees it, and
    ``LSSPA_ENGINE_CACHE=0`` in the environment makes every call create and free its own.  Keyword-only additions:

    method:  None (reference behaviour), 'exact', 'random', 'argsort', 'permutohedron' or 'subsets'.
        'subsets' (p <= 32): the exact attribution from the R^2 of all 2^p feature subsets, enumerated on the GPU in
        fp64 (include/lsspa.h, lsspa_subsets_shapley; ``ls_spa_interactions`` adds the pairwise interaction values
        from the same enumeration) -- no orderings, no sampling loop; overall_error 0,
        attribution_errors zeros, error_history empty, as the reference's exact path gives them.  The sampling
        parameters (max_samples, batch_size, num_batches, tolerance, seed, antithetical, lookahead, lanes,
        error_estimator, precision) are ignored -- phi, theta and r_squared are fp64 whatever an earlier call of the
        process set; return_attribution_history and checkpoint raise ValueError (there is
        no history and nothing to resume).  With comm= every rank enumerates by itself after the shared reduction.
    groups:  with method='subsets' only: a length-p sequence of integer labels, one per column, that makes GROUPS of
        columns the players of the game (a categorical variable's one-hot columns, a numeric one's spline columns).
        Label k in 0 .. g-1 puts the column into group k (every group needs a column); label -1 puts it into the
        baseline, the columns of every model (an intercept, controls), which get no attribution.  ``attribution`` then
        has length g: the exact Shapley values of u(S) = R^2 of the baseline plus the columns of the groups in S
        (include/lsspa.h, lsspa_groups_shapley).  They sum to r_squared minus the R^2 of the baseline alone, and are
        not the per-column attributions summed over a group.  theta (length p) and r_squared are those of the full
        fit.  Limits: g <= 32 groups and p <= 64 columns, the baseline's included; the p <= 32 limit of the ungrouped
        call does not apply.  The cost is set by g (2^g group subsets), not p: on one MI355X the whole call
        takes 1.5 ms at g = 12 / p = 64, 26 ms at g = 20 / p = 60, 0.21 s at g = 24 / p = 64 and 2.7 s at g = 28 /
        p = 56; it grows 16-fold per four groups, so expect about a minute at g = 32 (projected, not measured).
        With any other method (None and perms= too) groups raises ValueError: grouped attribution exists for the
        exact path only.  ``ls_spa_groups`` is the sampled counterpart, for any number of groups and columns.
    num_batches:  if given, ``max_samples = batch_size * num_batches`` (README dialect).
    return_history:  alias of ``return_attribution_history``.
    device:  GPU index.
    error_estimator:  'reference' (host, same generator call order as the reference),
        'lowrank' (same distribution, O(n p) instead of an O(p^3) factorisation, on the host) or
        'device' (the low-rank form on the GPU: the lift vectors never leave HBM; same numbers as
        'lowrank' for the same seed up to summation order).  None (default) lets the method decide:
        'reference' wherever the reference's code has a behaviour to mirror -- ``method`` None / 'random' / 'exact' and
        every call with ``perms=``: there the estimator shares the generator with the ordering source and its
        normal draws are observable in what is drawn next (ls_spa/ls_spa.py:168-175, :224) -- and 'device' for the
        QMC methods 'argsort' / 'permutohedron', which the reference's code does not implement (only its README
        names them): the estimator is then statistically the reference's (same 0.95-quantile definition of draws
        with covariance C_unbiased / n, ls_spa/ls_spa.py:321-341) without its p x p factorisation on the host, which at
        p = 5000 is 7 of the call's 9 seconds.
    precision:  'float64' (default, the reference's arithmetic) or 'float32' for the per-ordering
        factorisation work (about half the time; lifts agree to ~1e-5 on well-conditioned data;
        the Gram reduction, lift accumulation and statistics stay float64).
    checkpoint:  path of a state file, written after every error check and resumed from if it exists
        (same data, seed and sampler required); with several ranks every rank keeps ``<path>.rank<r>``.
    lookahead:  QMC samplers ('argsort', 'permutohedron') only.  k > 1 launches the orderings of k chunks as one GPU
        batch (a chunk of batch_size / n_gpus samples may fill a fraction of the GPU), accumulates and checks them
        chunk by chunk in the reference's order and drops the chunks beyond a stop.  Same results; at most k
        chunks of wasted GPU work at the end of a run.  'auto' (auto_lookahead): as many chunks as make up 64 samples
        per rank (512 up to p = 800, 1024 up to p = 250: smaller problems need more samples to fill the chip), eight
        at most; 2048 and sixteen for p <= 127, the one-workgroup-per-ordering kernels.  Default:
        'auto' for the QMC methods with the device estimator (whose checks the loop does not wait for), else 1.
    lanes:  1, 2 or 'auto'.  2: successive chunk groups alternate between two workspaces on two HIP streams, the next
        group's kernels starting when the current group's are half way, its orderings drawn and uploaded before the
        current group's statistics are read back; a chunk of 64 samples or more per rank goes as two half-chunks (QMC
        samplers only, as for lookahead; same results up to the rounding of the half-chunk grouping of the statistics;
        a stop wastes at most one group of GPU work).  'auto': 2 for the QMC methods when p > 127 (the fused small-p
        kernel gains nothing from it), else 1.
    comm:  several GPUs, one process each: the communicator every rank passes -- ``NativeComm.from_env()``
        (RCCL through the C ABI, no PyTorch) or ``TorchComm()`` (torch.distributed: RCCL, or gloo on CPU in
        the tests).  Sample number g of the run belongs to rank g mod world (a QMC method then draws a rank's own
        orderings only); the only data-path collective is one all-reduce of the packed batch moments per chunk.
    row_sharded:  several ranks only (``comm``).  False: every rank passes the whole data set.
        True: the four arrays are this rank's ROWS of the training and test sets; the ranks reduce
        their rows and sum the Gram matrices with one all-reduce.  'train': only the training rows are
        sharded, every rank passes all test rows (needed when there are fewer than p test rows).
    """
    data = _coerce_data(X_train, X_test, y_train, y_test)
    p = data[0].shape[1]
    # _players = (labels, g), ls_spa_groups only: the players of the game are g groups of columns.  Orderings, statistics,
    # estimator and results then have dimension g (`dim`); what follows the cost of an ordering keeps p.
    dim = p if _players is None else int(_players[1])
    if return_history is not None:
        return_attribution_history = bool(return_history)
    if num_batches is not None:
        max_samples = int(batch_size) * int(num_batches)
    if groups is not None and (method != "subsets" or perms is not None):
        raise ValueError("groups= is grouped attribution, which exists for the exact path only: pass method='subsets' "
                         "(no sampling method and no perms=)")
    comm = comm if comm is not None else _comm
    if method == "subsets":
        return _ls_spa_subsets(*data, reg, perms=perms, groups=groups,
                               return_attribution_history=return_attribution_history, device=device,
                               row_sharded=row_sharded, checkpoint=checkpoint, comm=comm, engine=_engine)
    error_estimator, lookahead, lanes = _sampling_options(method, perms, p, error_estimator, lookahead, lanes)
    tm = _timings if _timings is not None else {}   # bench.py's e2e_breakdown: host seconds per phase of this call
    lap = _stopwatch(tm)

    def prepare():
        share = dict(rank=comm.rank, world=comm.world) if comm is not None else {}
        return prepare_sampling(dim, max_samples=max_samples, batch_size=batch_size, seed=seed, perms=perms,
                                antithetical=antithetical, method=method, **share)

    # The ordering source first: a QMC source starts its helper thread here -- the first `import scipy.stats` of a process
    # (0.26 s; 1.3 s on a cold box), the Sobol' constructor (18 ms at p = 1000) and the first block of orderings then run
    # under the engine's creation and the data reduction instead of in front of the sampling loop.
    prepared = prepare()
    lap("sampler_start")
    # on the way out: the sampler's helper thread (already ended by a run that got as far as its loop)
    undo = [(lambda: _close_source(prepared[1]), True)]
    with _engine_call(_engine, device, comm, undo, lap) as engine:
        if precision != "float64" or getattr(engine, "precision", "float64") != "float64":
            engine.set_precision(precision)
        if hasattr(engine, "set_lanes") and getattr(engine, "lanes", 1) != lanes:
            engine.set_lanes(lanes)
        lap("setup")
        # theta and r^2 (ls_spa/ls_spa.py:240-243) depend on the reduced problem only: computed BEFORE the sampling loop,
        # so that the call does not end behind whatever the loop launched ahead of a stop and never collected
        theta, r_squared, info = _load_and_fit(engine, data, reg, row_sharded, comm, lap)
        if _timings is not None and hasattr(engine, "reduce_timing"):
            # the library's own split of the reduction: chunked copies + Gram kernels, finalize (the page-locking parts
            # are zero since round 4); what is left of the phase is host-side coercion and the call itself
            parts = engine.reduce_timing()
            whole = tm.pop("reduction_h2d_gram")
            tm["reduction_pin"], tm["reduction_copy_gram"] = parts["pin"], parts["h2d_gram"]
            tm["reduction_unpin"], tm["reduction_finalize"] = parts["unpin"], parts["finalize"]
            tm["reduction_host"] = whole - sum(parts.values())
        if _players is not None:
            engine.set_players(_players[0])      # after the full fit: that one is about the columns
            if hasattr(engine, "clear_players"):      # the caller's engine too: the map never outlives this call
                undo.append((engine.clear_players, False))

        def sampling_run(prep):
            out = run_estimator(
                engine, dim, cost_p=p, max_samples=max_samples, batch_size=batch_size, tolerance=tolerance, seed=seed,
                perms=perms, antithetical=antithetical, return_attribution_history=return_attribution_history,
                method=method, error_estimator=error_estimator, comm=comm, checkpoint=checkpoint, prepared=prep,
                lookahead=lookahead, timings=tm, defer=_defer)
            return out, info | (engine.info_collected() if hasattr(engine, "info_collected") else engine.info())

        (attribution, feat_err, total_err, err_hist, history, _), bits = sampling_run(prepared)
        lap()
        if _engine_fault(bits) and perms is None and checkpoint is None and hasattr(engine, "set_flags"):
            # An ordering source that can be drawn again (seed or QMC method; not the caller's iterable): the run is
            # repeated ONCE on the conservative path -- the lift kernel of its own reads V^T back, nothing is handed over
            # inside a launch (developer flag 512) -- instead of being lost.
            warnings.warn(f"engine fault in the fused lift scan (info bits {bits}): the run is repeated with the lift "
                          "kernel of its own", RuntimeWarning, stacklevel=2)
            engine.set_flags(512)
            _close_source(prepared[1])
            prepared = prepare()
            (attribution, feat_err, total_err, err_hist, history, _), bits = sampling_run(prepared)
        _info_verdict(bits, stacklevel=2)
        if info & 1:
            theta, r_squared = _singular_fit(engine, data[1], data[3])
        lap("final_fit")
    return ShapleyResults(attribution=attribution, theta=theta, overall_error=total_err,
                          attribution_errors=feat_err, r_squared=r_squared, error_history=err_hist,
                          attribution_history=history)


SUBSETS_MAX_P = 32     # include/lsspa.h, lsspa_subsets_shapley
GROUPS_MAX_G = 32      # include/lsspa.h, lsspa_groups_shapley
GROUPS_MAX_P = 64
OWEN_MAX_PLAYERS = 32  # include/lsspa.h, lsspa_groups_owen


def group_labels(groups, p, max_groups=GROUPS_MAX_G, max_players=None):
    """(labels as int32, g) of ls_spa(groups=) and ls_spa_groups: a label per column, -1 the baseline, 0 .. g-1 the
    groups, none of them empty.  max_groups: the enumeration's limit (None for the sampled methods, whose only limit is
    g <= p, which labels of length p cannot break).  max_players (ls_spa_owen): the limit on the players of a group's
    refined game, the other g - 1 groups and the group's own columns.  ValueError names what is wrong."""
    labels = np.asarray(groups)
    if labels.ndim != 1 or len(labels) != p:
        raise ValueError(f"groups must have one label per column: length p = {p}, got shape {labels.shape}")
    if labels.dtype.kind not in "iu":
        raise ValueError(f"groups must hold integer labels (-1: baseline, 0 .. g-1: group), got dtype {labels.dtype}")
    labels = labels.astype(np.int64)
    if labels.min() < -1:
        raise ValueError(f"groups holds a label below -1 ({labels.min()}); -1 is the baseline, groups count from 0")
    g = int(labels.max()) + 1
    if g < 1:
        raise ValueError("groups names no group at all (every label is -1): there is nothing to attribute to")
    if max_groups is not None and g > max_groups:
        raise ValueError(f"grouped attribution enumerates all 2^g group subsets and takes at most g = {max_groups} "
                         f"groups (groups= names {g})")
    missing = np.setdiff1d(np.arange(g), labels)
    if len(missing):
        raise ValueError(f"groups has a gap in its numbering: no column carries label {int(missing[0])} "
                         f"(labels run to {g - 1})")
    if max_players is not None:
        size = np.bincount(labels[labels >= 0], minlength=g)
        over = np.nonzero(g - 1 + size > max_players)[0]
        if len(over):
            k = int(over[0])
            raise ValueError(f"the Owen value enumerates the refined game of every group, the other g - 1 groups and "
                             f"the group's own columns, and takes at most {max_players} players: group {k} has "
                             f"{int(size[k])} columns beside {g - 1} other groups ({g - 1 + int(size[k])} players)")
    return np.ascontiguousarray(labels, dtype=np.int32), g


def _ls_spa_subsets(X_train, X_test, y_train, y_test, reg, *, perms, return_attribution_history, device, row_sharded,
                    checkpoint, comm, engine, groups=None, interactions=False):
    """ls_spa(method='subsets'): the data reduction as for every method, then the exact attribution over all 2^p
    subsets -- with groups=, over all 2^g subsets of the groups of columns -- on the engine.  No ordering source,
    generator or sampling loop exists in this call.  interactions (ls_spa_interactions): the same call with the
    pairwise interaction index between the players, features or groups, from the same enumeration, returned as
    InteractionResults."""
    p = X_train.shape[1]
    if perms is not None:
        raise ValueError("pass either perms= or method=, not both")
    labels = None
    if groups is not None:
        if p > GROUPS_MAX_P:
            raise ValueError(f"grouped attribution takes at most p = {GROUPS_MAX_P} columns, the baseline's included "
                             f"(this problem has p = {p})")
        labels, n_players = group_labels(groups, p)
    elif p > SUBSETS_MAX_P:
        raise ValueError(f"method='subsets' enumerates all 2^p feature subsets and takes at most p = {SUBSETS_MAX_P} "
                         f"features (this problem has p = {p}); use a sampling method")
    if return_attribution_history:
        raise ValueError("method='subsets' computes no attribution history (there are no samples)")
    if checkpoint is not None:
        raise ValueError("method='subsets' has no state to checkpoint or resume")
    with _engine_call(engine, device, comm) as engine:
        # precision stays set on a kept engine: theta and r_squared come from its fp64 factorisation, like phi
        if getattr(engine, "precision", "float64") != "float64":
            engine.set_precision("float64")
        theta, r_squared, info = _load_and_fit(engine, (X_train, X_test, y_train, y_test), reg, row_sharded, comm)
        if interactions:
            phi, raw, bits = engine.subsets_interactions() if labels is None else engine.groups_interactions(labels)
        else:
            phi, bits = engine.subsets_shapley() if labels is None else engine.groups_shapley(labels)
        _info_verdict((bits | info) & 1, stacklevel=3)      # (an enumeration reports a broken pivot, nothing else)
        if info & 1:
            theta, r_squared = _singular_fit(engine, X_test, y_test)
    if interactions:
        return InteractionResults(interactions=_shap_matrix(phi, raw), attribution=phi, theta=theta,
                                  r_squared=r_squared)
    return ShapleyResults(attribution=phi, theta=theta, overall_error=0.0,
                          attribution_errors=np.zeros(p if labels is None else n_players),
                          r_squared=r_squared, error_history=np.zeros(0), attribution_history=None)


def ls_spa_interactions(X_train, X_test, y_train, y_test, reg=0., *, groups=None, device=0, row_sharded=False,
                        comm=None, _engine=None):
    """Exact pairwise Shapley interaction values of the out-of-sample R^2, between features (p <= 32) or, with
    ``groups=``, between groups of columns (g <= 32 groups over p <= 64 columns).

    The game is that of ``ls_spa``: v(S) is the out-of-sample R^2 of the model fitted on the features in S.  From the
    same enumeration of all 2^p subsets on the GPU that ``ls_spa(method='subsets')`` runs (fp64, bitwise reproducible;
    include/lsspa.h, lsspa_subsets_interactions) comes, beside the attribution, the Shapley interaction index

        I_ij = sum over S without i and j of |S|! (p - 2 - |S|)! / (p - 1)! (v(S+i+j) - v(S+i) - v(S+j) + v(S)),

    positive where two features create R^2 together (complements), negative where they share it (correlated
    regressors).  Returns ``InteractionResults``: ``interactions`` is the p x p matrix Phi in SHAP's convention --
    Phi_ij = I_ij / 2 for i != j, Phi_ii = phi_i - sum_{j != i} Phi_ij -- so Phi is symmetric, row i sums to
    ``attribution[i]`` and the whole matrix to ``r_squared``; at p = 1 it is [[phi_0]].  ``attribution``, ``theta`` and
    ``r_squared`` are exactly those of ``ls_spa(method='subsets')``, as are ``reg``, ``device``, ``row_sharded``,
    ``comm`` and the RuntimeWarning for a Gram matrix that is not numerically positive definite.  p > 32 raises
    ValueError.

    groups:  a length-p sequence of integer labels, one per column, as for ``ls_spa(method='subsets', groups=)``: k in
        0 .. g-1 puts the column into group k, -1 into the always-included baseline.  The players are then the g groups
        -- the variables, where a one-hot factor or a spline basis is several columns -- and the game is that call's
        u(S) = R^2 of the baseline plus the columns of the groups in S (include/lsspa.h, lsspa_groups_interactions).
        ``interactions`` is g x g in the same convention: row k sums to ``attribution[k]``, the group's Shapley value as
        ``ls_spa(method='subsets', groups=)`` returns it, and the whole matrix to ``r_squared`` minus the R^2 of the
        baseline alone.  ``theta`` keeps length p.  The limits and errors are that call's: g <= 32, p <= 64 (the
        p <= 32 limit does not apply), labels refused with ValueError before any GPU work."""
    data = _coerce_data(X_train, X_test, y_train, y_test)
    return _ls_spa_subsets(*data, reg, perms=None, return_attribution_history=False,
                           device=device, row_sharded=row_sharded, checkpoint=None, comm=comm, engine=_engine,
                           groups=groups, interactions=True)


def _baseline_r_squared(engine, labels, X_test, y_test):
    """The out-of-sample R^2 of the baseline columns (label -1) alone from the engine's reduced problem, as
    _singular_fit forms the full model's; 0.0 without a baseline."""
    base = np.nonzero(np.asarray(labels) == -1)[0]
    if len(base) == 0:
        return 0.0
    G, g, H, h = engine.gram()
    sub = np.ix_(base, base)
    try:
        theta = np.linalg.solve(G[sub], g[base])
    except np.linalg.LinAlgError:
        theta = _min_norm_theta(G[sub], g[base])
    if engine.tri:      # from the Gram side: also right when the test rows are sharded
        return float((2.0 * (h[base] @ theta) - theta @ H[sub] @ theta) / engine.y_norm_sq)
    pred = X_test[:, base].astype(np.float64) @ theta
    return float((2.0 * (pred @ y_test) - pred @ pred) / engine.y_norm_sq)


def ls_spa_owen(X_train, X_test, y_train, y_test, groups, reg=0., *, device=0, row_sharded=False, comm=None,
                _engine=None):
    """Exact Owen values of the out-of-sample R^2: the attribution of every column when the columns form groups (g <= 32
    groups over p <= 64 columns, g - 1 + the largest group's size <= 32).

    ``ls_spa(method='subsets', groups=)`` says what a variable -- a one-hot factor, a spline basis -- earns of the R^2;
    this call says which of its columns earn it.  The Owen value is the two-level Shapley value under the coalition
    structure ``groups``: the mean of a column's lift over exactly those orderings in which the baseline comes first and
    every group's columns are contiguous.  (The ungrouped ``ls_spa(method='subsets')`` lets a factor's levels compete
    with every other column one by one: another game, with other numbers.)  Per group of two or more columns the GPU
    enumerates that group's refined game -- the other groups whole, its own columns as singletons -- in fp64, bitwise
    reproducibly (include/lsspa.h, lsspa_groups_owen).

    groups:  one integer label per column as ``ls_spa(method='subsets', groups=)`` takes them: k in 0 .. g-1 puts the
        column into group k, -1 into a baseline that every model includes and that gets no attribution.

    Returns ``OwenResults``: ``attribution`` [p], the Owen values (0.0 on baseline columns); ``group_attribution`` [g],
    bitwise what ``ls_spa(method='subsets', groups=)`` returns; ``theta`` [p], ``r_squared`` and
    ``baseline_r_squared``, the R^2 of the baseline alone (0 without one).  ``attribution[labels == k].sum()`` is
    ``group_attribution[k]`` and ``attribution.sum()`` is ``r_squared - baseline_r_squared``, up to rounding.
    All-singleton groups give the ungrouped exact attribution; one group gives the exact attribution of its columns
    with the baseline eliminated.

    p > 64, g > 32, a group whose refined game has more than 32 players and bad labels raise ValueError before any GPU
    work.  ``reg``, ``device``, ``row_sharded``, ``comm`` and the RuntimeWarning for a Gram matrix that is not
    numerically positive definite are those of ``ls_spa(method='subsets')``."""
    X_train, X_test, y_train, y_test = _coerce_data(X_train, X_test, y_train, y_test)
    p = X_train.shape[1]
    if p > GROUPS_MAX_P:
        raise ValueError(f"grouped attribution takes at most p = {GROUPS_MAX_P} columns, the baseline's included "
                         f"(this problem has p = {p})")
    labels, _ = group_labels(groups, p, max_players=OWEN_MAX_PLAYERS)
    with _engine_call(_engine, device, comm) as engine:
        # precision stays set on a kept engine: theta and r_squared come from its fp64 factorisation, like the values
        if getattr(engine, "precision", "float64") != "float64":
            engine.set_precision("float64")
        theta, r_squared, info = _load_and_fit(engine, (X_train, X_test, y_train, y_test), reg, row_sharded, comm)
        owen, phi, bits = engine.groups_owen(labels)
        _info_verdict((bits | info) & 1, stacklevel=2)      # (an enumeration reports a broken pivot, nothing else)
        if info & 1:
            theta, r_squared = _singular_fit(engine, X_test, y_test)
        base = _baseline_r_squared(engine, labels, X_test, y_test)
    return OwenResults(attribution=owen, group_attribution=phi, theta=theta, r_squared=r_squared,
                       baseline_r_squared=base)


def include_mask(include, p):
    """The columns every model must contain as lsspa_subsets_best's mask (bit j = column j) and as a sorted index
    array; ValueError names what is wrong with them.  Needs no engine."""
    if include is None:
        return 0, np.zeros(0, dtype=np.int64)
    try:
        raw = None if isinstance(include, (str, bytes)) else np.asarray(list(include))
    except TypeError:
        raw = None
    if raw is None or raw.ndim != 1:
        raise ValueError("include must be an iterable of column indices")
    if raw.size == 0:
        return 0, np.zeros(0, dtype=np.int64)
    cols = raw.astype(np.int64)
    if raw.dtype == bool or not np.array_equal(cols, raw):
        raise ValueError("include must hold integer column indices")
    if cols.min() < 0 or cols.max() >= p:
        raise ValueError(f"include names a column outside 0 .. {p - 1}")
    if len(np.unique(cols)) != len(cols):
        raise ValueError("include names a column twice")
    cols = np.sort(cols)
    return sum(1 << int(j) for j in cols), cols


def _subset_fit(G, g, cols):
    """theta [p] of the model on the columns `cols` from the reduced problem: G_KK theta_K = g_K, exactly 0.0
    elsewhere."""
    theta = np.zeros(len(g))
    if len(cols):
        sub = np.ix_(cols, cols)
        try:
            theta[cols] = np.linalg.solve(G[sub], g[cols])
        except np.linalg.LinAlgError:
            theta[cols] = _min_norm_theta(G[sub], g[cols])
    return theta


def _best_group_subsets(data, reg, labels, g, device, _engine):
    """ls_spa_best_subsets(groups=): the best set of groups of every size 0 .. g on the engine (groups_best), each
    winner refitted on the host on the baseline's and its groups' columns."""
    p = data[0].shape[1]
    with _engine_call(_engine, device) as engine:
        # precision stays set on a kept engine: theta and r_squared come from its fp64 factorisation, like the values
        if getattr(engine, "precision", "float64") != "float64":
            engine.set_precision("float64")
        _, full_r_squared, info = _load_and_fit(engine, data, reg, False, None)
        u, masks, found, bits = engine.groups_best(labels)
        if info & 1:
            _, full_r_squared = _singular_fit(engine, data[1], data[3])
        G, gv, _, _ = engine.gram()
    _info_verdict((bits | info) & 1, stacklevel=3)      # (an enumeration reports a broken pivot, nothing else)
    sizes = np.arange(g + 1)
    group_subsets = np.zeros((g + 1, g), dtype=bool)
    subsets = np.zeros((g + 1, p), dtype=bool)
    r_squared = np.full(g + 1, np.nan)
    theta = np.full((g + 1, p), np.nan)
    for k in sizes:
        if found[k]:
            group_subsets[k] = (int(masks[k]) >> np.arange(g)) & 1
            subsets[k] = (labels < 0) | group_subsets[k][np.maximum(labels, 0)]
            r_squared[k] = u[k]
            theta[k] = _subset_fit(G, gv, np.nonzero(subsets[k])[0])
    best_size, best_groups, best_subset = -1, np.zeros(g, dtype=bool), np.zeros(p, dtype=bool)
    if not np.all(np.isnan(r_squared)):
        best_size = int(np.nanargmax(r_squared))      # the first of equal maxima: the smallest size
        best_groups, best_subset = group_subsets[best_size].copy(), subsets[best_size].copy()
    return BestGroupSubsetsResults(sizes=sizes, group_subsets=group_subsets, subsets=subsets,
                                   n_columns=subsets.sum(axis=1), r_squared=r_squared, theta=theta,
                                   best_size=best_size, best_group_subset=best_groups, best_subset=best_subset,
                                   full_r_squared=float(full_r_squared), baseline_r_squared=float(r_squared[0]))


def ls_spa_best_subsets(X_train, X_test, y_train, y_test, reg=0., *, include=None, groups=None, device=0,
                        _engine=None):
    """Exhaustive best-subset selection by out-of-sample R^2: the best model of every size over all 2^p feature subsets
    (p <= 32) or, with ``groups=``, over all 2^g subsets of groups of columns (g <= 32 groups over p <= 64 columns).

    ``ls_spa`` says who earns the R^2; this call says which model to keep.  v(S), the out-of-sample R^2 of the model
    fitted on the features in S, is not monotone in S -- the best model is usually not the full one, and no
    branch-and-bound rule applies -- so the GPU evaluates every subset, in the enumeration that
    ``ls_spa(method='subsets')`` runs (fp64, bitwise reproducible; include/lsspa.h, lsspa_subsets_best), and keeps per
    size the largest value and its subset.  On equal values the subset with the smaller mask (bit j = feature j) wins.

    include:  an iterable of column indices that every model must contain (an intercept, controls); the sizes then
        start at len(include).

    groups:  a length-p sequence of integer labels, one per column, as for ``ls_spa(method='subsets', groups=)``: k in
        0 .. g-1 puts the column into group k, -1 into the always-included baseline.  A one-hot factor or a spline
        basis then goes in or out whole: the models are the 2^g sets of groups (each with the baseline's columns), a
        model's size is its number of groups, 0 .. g, and the cost is set by g, not by p (include/lsspa.h,
        lsspa_groups_best).  On equal values the set with the smaller mask (bit k = group k) wins.  The p <= 32 limit
        does not apply; the limits and label errors are that call's, g <= 32 and p <= 64.  ``include=`` cannot be
        combined with it: label those columns -1, the baseline is the include set.  Returns
        ``BestGroupSubsetsResults``: ``sizes`` 0 .. g, ``group_subsets`` [n][g] bool, ``subsets`` [n][p] bool (the
        baseline's and the winners' columns), ``n_columns`` [n], ``r_squared``, ``theta``, ``best_size``,
        ``best_group_subset``, ``best_subset``, ``full_r_squared`` (``ls_spa(method='subsets', groups=).r_squared``)
        and ``baseline_r_squared``, which is ``r_squared[0]``.

    Returns ``BestSubsetsResults``: ``sizes``, ``subsets`` [n][p] bool, ``r_squared`` [n], ``theta`` [n][p] (each
    winner refitted on the host in fp64, exactly 0.0 outside its subset), ``best_size``, ``best_subset`` and
    ``full_r_squared``, which is ``ls_spa(method='subsets').r_squared``.

    p > 32, an ``include`` out of range or with duplicates, shapes that do not fit and a ``y_test`` that is identically
    zero are refused before any GPU work.  A subset whose Gram matrix is not numerically positive definite is no
    candidate and raises the RuntimeWarning of ``ls_spa(method='subsets')``; a size without any candidate is a NaN
    row.  ``reg`` and ``device`` are that call's."""
    data = _coerce_data(X_train, X_test, y_train, y_test)
    p = data[0].shape[1]
    if groups is not None:
        if include is not None:
            raise ValueError("include= cannot be combined with groups=: label the columns every model must contain "
                             "-1, the baseline is the include set")
        if p > GROUPS_MAX_P:
            raise ValueError(f"grouped attribution takes at most p = {GROUPS_MAX_P} columns, the baseline's included "
                             f"(this problem has p = {p})")
        labels, n_groups = group_labels(groups, p)
        if data[1].shape[0] < 1:
            raise ValueError(f"ls_spa_best_subsets needs M >= 1 test rows (M = {data[1].shape[0]})")
        if not np.any(data[3]):
            raise ValueError("y_test is identically zero: the out-of-sample R^2 is not defined")
        return _best_group_subsets(data, reg, labels, n_groups, device, _engine)
    if p > SUBSETS_MAX_P:
        raise ValueError(f"ls_spa_best_subsets enumerates all 2^p feature subsets and takes at most p = {SUBSETS_MAX_P} "
                         f"features (this problem has p = {p})")
    if p < 1 or data[1].shape[0] < 1:
        raise ValueError(f"ls_spa_best_subsets needs p >= 1 features and M >= 1 test rows (p = {p}, "
                         f"M = {data[1].shape[0]})")
    mask, inc = include_mask(include, p)
    if not np.any(data[3]):
        raise ValueError("y_test is identically zero: the out-of-sample R^2 is not defined")
    with _engine_call(_engine, device) as engine:
        # precision stays set on a kept engine: theta and r_squared come from its fp64 factorisation, like the values
        if getattr(engine, "precision", "float64") != "float64":
            engine.set_precision("float64")
        _, full_r_squared, info = _load_and_fit(engine, data, reg, False, None)
        v, masks, found, bits = engine.subsets_best(mask)
        if info & 1:
            _, full_r_squared = _singular_fit(engine, data[1], data[3])
        G, g, _, _ = engine.gram()
    _info_verdict((bits | info) & 1, stacklevel=2)      # (an enumeration reports a broken pivot, nothing else)
    sizes = np.arange(len(inc), p + 1)
    n = len(sizes)
    subsets = np.zeros((n, p), dtype=bool)
    r_squared = np.full(n, np.nan)
    theta = np.full((n, p), np.nan)
    for i, k in enumerate(sizes):
        if found[k]:
            subsets[i] = (int(masks[k]) >> np.arange(p)) & 1
            r_squared[i] = v[k]
            theta[i] = _subset_fit(G, g, np.nonzero(subsets[i])[0])
    best_size, best_subset = -1, np.zeros(p, dtype=bool)
    if not np.all(np.isnan(r_squared)):
        i = int(np.nanargmax(r_squared))      # the first of equal maxima: the smallest size
        best_size, best_subset = int(sizes[i]), subsets[i].copy()
    return BestSubsetsResults(sizes=sizes, subsets=subsets, r_squared=r_squared, theta=theta, best_size=best_size,
                              best_subset=best_subset, full_r_squared=float(full_r_squared))


CV_MAX_FOLDS = 32          # include/lsspa.h, lsspa_cv_load


def cv_fold_ids(n, folds=5, *, seed=42, shuffle=True):
    """(fold_ids [n] int32, K): the fold of every row.  ``folds`` an int K: with ``shuffle`` row pi[i] goes to fold
    i mod K, pi the host permutation of (seed, replicate 0, side 0, n) that ``ls_spa_permutation_test`` draws (a pure
    function of (seed, n): include/lsspa.h, lsspa_debug_perm_indices); without, row i goes to fold i mod K.  ``folds`` an
    integer array [n] of labels 0 .. K-1 is taken as given, K = its largest label + 1.  ValueError names what is wrong:
    K outside 2 .. 32, a label outside 0 .. K-1, an empty fold.  Needs no GPU."""
    n = int(n)
    if np.ndim(folds) == 0:
        if isinstance(folds, (bool, np.bool_)) or int(folds) != folds:
            raise ValueError("folds must be an integer number of folds or an integer array of fold labels")
        K = int(folds)
        if K < 2 or K > CV_MAX_FOLDS:
            raise ValueError(f"cross-validation takes 2 .. {CV_MAX_FOLDS} folds (folds = {K})")
        if K > n:
            raise ValueError(f"fold {n} of {K} would be empty: there are only N = {n} rows")
        ids = np.empty(n, dtype=np.int32)
        if shuffle:
            from ._engine import debug_perm_indices
            order = debug_perm_indices(int(seed), 0, 0, n).astype(np.int64)
        else:
            order = np.arange(n)
        ids[order] = np.arange(n) % K
        return ids, K
    raw = np.asarray(folds)
    if raw.shape != (n,):
        raise ValueError(f"fold labels must have shape ({n},), got {raw.shape}")
    if raw.dtype == bool or not np.issubdtype(raw.dtype, np.number) or not np.array_equal(raw.astype(np.int64), raw):
        raise ValueError("fold labels must be integers")
    lab = raw.astype(np.int64)
    if lab.min() < 0:
        raise ValueError(f"fold labels must be 0 .. K-1 (label {int(lab.min())} given)")
    K = int(lab.max()) + 1
    if K < 2 or K > CV_MAX_FOLDS:
        raise ValueError(f"cross-validation takes 2 .. {CV_MAX_FOLDS} folds (the labels name {K})")
    counts = np.bincount(lab, minlength=K)
    if (counts == 0).any():
        raise ValueError(f"fold {int(np.argmin(counts != 0))} of {K} is empty: every fold needs at least one row")
    return lab.astype(np.int32), K


def _cv_data(name, X, y, folds, seed, shuffle, grouped=False):
    """The checks every cross-validation call makes before it touches an engine: (X, y, fold_ids, K).  grouped: the
    column limit is that of ``ls_spa(groups=)``."""
    X, y = np.asarray(X), np.asarray(y)
    if X.ndim != 2 or y.ndim != 1:
        raise ValueError(f"{name}: X must be two-dimensional and y one-dimensional")
    if X.shape[0] != y.shape[0]:
        raise SizeIncompatible(f"X has {X.shape[0]} rows, y has {y.shape[0]}")
    n, p = X.shape
    if grouped:
        if p > GROUPS_MAX_P:
            raise ValueError(f"grouped attribution takes at most p = {GROUPS_MAX_P} columns, the baseline's included "
                             f"(this problem has p = {p})")
    elif p > SUBSETS_MAX_P:
        raise ValueError(f"{name} enumerates all 2^p feature subsets and takes at most p = {SUBSETS_MAX_P} features "
                         f"(this problem has p = {p})")
    if p < 1 or n < 2:
        raise ValueError(f"{name} needs p >= 1 features and N >= 2 rows (p = {p}, N = {n})")
    ids, K = cv_fold_ids(n, folds, seed=seed, shuffle=shuffle)
    if not np.any(y):
        raise ValueError("y is identically zero: the cross-validated R^2 is not defined")
    return X, y, ids, K


def _cv_full_problem(X, y, reg):
    """G = X^T X / N + reg I and g = X^T y / N of all rows, fp64 on the host: what the coefficients are refitted on."""
    Xd, yd = np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n, p = Xd.shape
    return Xd.T @ Xd / n + reg * np.eye(p), Xd.T @ yd / n


def _cv_verdict(info, stacklevel):
    """The RuntimeWarning of a cross-validation call whose fold problems met a broken pivot, naming the folds."""
    bad = [int(f) for f in np.nonzero(np.asarray(info) & 1)[0]]
    if bad:
        warnings.warn(f"a Gram matrix of the training rows of fold(s) {', '.join(map(str, bad))} was not numerically "
                      "positive definite; subsets of collinear features are no candidates there and their attribution "
                      "is not meaningful", RuntimeWarning, stacklevel=stacklevel + 1)


def _seq_sum(rows):
    """The fp64 sum of the rows in ascending order, as the device forms it."""
    total = np.array(rows[0], dtype=np.float64, copy=True)
    for r in rows[1:]:
        total = total + r
    return total


def _cv_group_verdict(info, stacklevel):
    """_cv_verdict for the grouped calls: the folds by name, sets of groups instead of subsets of features."""
    bad = [int(f) for f in np.nonzero(np.asarray(info) & 1)[0]]
    if bad:
        warnings.warn(f"a Gram matrix of the training rows of fold(s) {', '.join(map(str, bad))} was not numerically "
                      "positive definite; sets of groups with collinear columns are no candidates there and their "
                      "attribution is not meaningful", RuntimeWarning, stacklevel=stacklevel + 1)


def _cv_groups(X, y, reg, ids, K, labels, g, device, _engine):
    """ls_spa_cv(groups=): the attribution of the cross-validated R^2 to the g groups (cv_groups_shapley)."""
    with _engine_call(_engine, device) as engine:
        engine.cv_groups_load(X, y, ids, K, reg)
        try:
            phi, phi_fold, r2_fold, base_fold, info = engine.cv_groups_shapley(labels)
        finally:
            engine.cv_free()
    _cv_group_verdict(info, stacklevel=3)
    G, gv = _cv_full_problem(X, y, reg)
    return CVGroupResults(attribution=phi, fold_attribution=phi_fold, r_squared=float(_seq_sum(list(r2_fold))),
                          fold_r_squared=np.asarray(r2_fold), baseline_r_squared=float(_seq_sum(list(base_fold))),
                          fold_baseline_r_squared=np.asarray(base_fold),
                          theta=_subset_fit(G, gv, np.arange(X.shape[1])), fold_ids=ids)


def _cv_best_group_subsets(X, y, reg, ids, K, labels, g, device, _engine):
    """ls_spa_best_subsets_cv(groups=): the best set of groups of every size 0 .. g by the cross-validated value
    (cv_groups_best), each winner refitted on all rows on the host on the baseline's and its groups' columns."""
    p = X.shape[1]
    with _engine_call(_engine, device) as engine:
        engine.cv_groups_load(X, y, ids, K, reg)
        try:
            u, masks, found, u_fold, info = engine.cv_groups_best(labels)
            full, _ = engine.debug_cv_group_values(labels, np.array([(1 << g) - 1], dtype=np.uint64), folds=False)
        finally:
            engine.cv_free()
    _cv_group_verdict(info, stacklevel=3)
    G, gv = _cv_full_problem(X, y, reg)
    sizes = np.arange(g + 1)
    group_subsets = np.zeros((g + 1, g), dtype=bool)
    subsets = np.zeros((g + 1, p), dtype=bool)
    r_squared = np.full(g + 1, np.nan)
    fold_r_squared = np.full((g + 1, K), np.nan)
    theta = np.full((g + 1, p), np.nan)
    for k in sizes:
        if found[k]:
            group_subsets[k] = (int(masks[k]) >> np.arange(g)) & 1
            subsets[k] = (labels < 0) | group_subsets[k][np.maximum(labels, 0)]
            r_squared[k] = u[k]
            fold_r_squared[k] = u_fold[k]
            theta[k] = _subset_fit(G, gv, np.nonzero(subsets[k])[0])
    best_size, best_groups, best_subset = -1, np.zeros(g, dtype=bool), np.zeros(p, dtype=bool)
    if not np.all(np.isnan(r_squared)):
        best_size = int(np.nanargmax(r_squared))      # the first of equal maxima: the smallest size
        best_groups, best_subset = group_subsets[best_size].copy(), subsets[best_size].copy()
    return CVBestGroupSubsetsResults(sizes=sizes, group_subsets=group_subsets, subsets=subsets,
                                     n_columns=subsets.sum(axis=1), r_squared=r_squared,
                                     fold_r_squared=fold_r_squared, theta=theta, best_size=best_size,
                                     best_group_subset=best_groups, best_subset=best_subset,
                                     full_r_squared=float(full[0]), baseline_r_squared=float(r_squared[0]),
                                     fold_ids=ids)


def ls_spa_cv(X, y, reg=0., folds=5, *, groups=None, seed=42, shuffle=True, device=0, _engine=None):
    """Exact Shapley attribution of the K-fold cross-validated out-of-sample R^2 (p <= 32): one data set, no split to
    choose.

    Fold f is predicted by the model fitted on the other folds' rows; with the pooled denominator ||y||^2 the folds'
    values add up to the cross-validated R^2, 1 - sum_f ||y_f - X_f theta^(-f)||^2 / ||y||^2, and since the Shapley value
    is linear in the game its attribution is the sum of the folds' attributions.  The rows go to the GPU once, the K
    per-fold Grams come from one weighted pass, and the K fold problems are enumerated as ``ls_spa(method='subsets')``
    enumerates one (fp64, bitwise reproducible; include/lsspa.h, lsspa_cv_shapley).

    folds:  the number of folds K (2 .. 32) -- with ``shuffle`` the rows are dealt by a permutation that is a pure
        function of (seed, N), without it row i goes to fold i mod K -- or an integer array [N] of labels 0 .. K-1.

    Returns ``CVResults``: ``attribution`` [p], ``fold_attribution`` [K][p] (its rows sum to ``attribution``),
    ``r_squared`` (the cross-validated R^2 of the full model, what ``attribution`` sums to), ``fold_r_squared`` [K]
    (each fold's share, summing to ``r_squared``), ``theta`` [p] (fitted on all rows) and ``fold_ids`` [N].

    Shapes that do not fit, p > 32, K outside 2 .. 32, a label outside 0 .. K-1, an empty fold and a y that is
    identically zero are refused before any GPU work.  A fold whose training rows give a Gram matrix that is not
    numerically positive definite raises a RuntimeWarning that names the fold.

    groups:  a length-p sequence of integer labels, one per column, as for ``ls_spa(method='subsets', groups=)``: k in
        0 .. g-1 puts the column into group k, -1 into the always-included baseline (an intercept, controls).  The
        players are then the g groups -- a one-hot factor or a spline basis is attributed as one variable --, the cost
        is set by g, not by p, and the limits are g <= 32 groups over p <= 64 columns (include/lsspa.h,
        lsspa_cv_groups_shapley); the label errors are that call's.  Returns ``CVGroupResults``: ``attribution`` [g],
        ``fold_attribution`` [K][g], ``r_squared``, ``fold_r_squared`` [K], ``baseline_r_squared`` (the cross-validated
        R^2 of the baseline's columns alone; ``attribution`` sums to ``r_squared - baseline_r_squared``),
        ``fold_baseline_r_squared`` [K], ``theta`` [p] and ``fold_ids``."""
    if groups is not None:
        X, y, ids, K = _cv_data("ls_spa_cv", X, y, folds, seed, shuffle, grouped=True)
        labels, n_groups = group_labels(groups, X.shape[1])
        return _cv_groups(X, y, reg, ids, K, labels, n_groups, device, _engine)
    X, y, ids, K = _cv_data("ls_spa_cv", X, y, folds, seed, shuffle)
    with _engine_call(_engine, device) as engine:
        engine.cv_load(X, y, ids, K, reg)
        try:
            phi, phi_fold, r2_fold, info = engine.cv_shapley()
        finally:
            engine.cv_free()
    _cv_verdict(info, stacklevel=2)
    G, g = _cv_full_problem(X, y, reg)
    return CVResults(attribution=phi, fold_attribution=phi_fold, r_squared=float(_seq_sum(list(r2_fold))),
                     fold_r_squared=np.asarray(r2_fold), theta=_subset_fit(G, g, np.arange(X.shape[1])), fold_ids=ids)


CV_LIFT_MAX_P = 127        # include/lsspa.h, LSSPA_CV_LIFT_MAX_P


def _cv_fold_values(problems, cols):
    """[K]: fold f's value (2 h^T theta - theta^T H theta) / ||y||^2 of the model on the columns `cols`, theta fitted on
    fold problem f = (G, g, H, h, inv_yy); 0 for no columns."""
    out = np.zeros(len(problems))
    for f, (G, g, H, h, inv_yy) in enumerate(problems):
        th = _subset_fit(G, g, cols)
        out[f] = (2.0 * (h @ th) - th @ H @ th) * inv_yy
    return out


def _sampled_arguments(p, groups, perms, method, max_samples, batch_size, seed, antithetical):
    """What the sampled families' public functions do with ``groups``, ``perms``, ``method`` and the sample counts, in
    this order: the labels (None without groups) and d, the dimension of a sample; perms and method refused together;
    the counts positive; the ordering source in dimension d.
    Returns (labels, d, source, batch_size, antithetical, max_samples, never_stop)."""
    labels, d = None, p
    if groups is not None:
        labels, d = group_labels(groups, p, max_groups=None)
    if perms is not None:
        if method != "random":
            raise ValueError("pass either perms= or method=, not both")
        method = None
    elif method not in S.METHODS:
        raise ValueError(f"method must be one of {tuple(S.METHODS)}")
    if int(batch_size) < 1 or int(max_samples) < 1:
        raise ValueError("batch_size and max_samples must be positive")
    _, source, batch_size, antithetical, max_samples, never_stop = prepare_sampling(
        d, max_samples=int(max_samples), batch_size=int(batch_size), seed=seed, perms=perms,
        antithetical=bool(antithetical), method=method)
    return labels, d, source, batch_size, antithetical, max_samples, never_stop


def _sample_until(source, batch, get, worst_error, batch_size, max_samples, tolerance):
    """Draw batches of orderings from source through batch(rows) until max_samples, the source's end or -- with a
    tolerance, from two samples on -- worst_error(state) <= tolerance.  Returns the state get() gives (n first), read
    once per batch; no ordering at all is a ValueError."""
    n, state = 0, None
    while n < max_samples:
        rows = source.take(min(batch_size, max_samples - n))
        if len(rows) == 0:
            break
        batch(rows)
        n += len(rows)
        state = None
        if tolerance is not None and n >= 2:
            state = get()
            if worst_error(state) <= tolerance:
                break
    if n == 0:
        raise ValueError("no ordering to sample: perms is empty")
    return state if state is not None else get()


def ls_spa_cv_sampled(X, y, reg=0., folds=5, max_samples=2 ** 13, batch_size=2 ** 8, tolerance=None, seed=42,
                      perms=None, *, groups=None, method="random", antithetical=True, fold_seed=42, shuffle=True,
                      device=0, _engine=None):
    """Sampled Shapley attribution of the K-fold cross-validated out-of-sample R^2 (p <= 127): what ``ls_spa_cv`` gives
    exactly for p <= 32, estimated from sampled orderings beyond that -- one data set, no split to choose.

    The game is ``ls_spa_cv``'s: fold f is predicted by the model fitted on the other folds' rows, and every fold
    divides by the pooled ||y||^2.  A sample's lift vector is the sum over the folds of the lift vectors of ONE ordering
    shared by all folds; one launch runs a batch's orderings through the K fold problems at once (include/lsspa.h,
    lsspa_cv_lift_batch).  fp64 throughout; two calls agree bitwise.

    folds, fold_seed, shuffle:  what ``folds``, ``seed`` and ``shuffle`` are to ``ls_spa_cv`` (``cv_fold_ids``; an integer
        array [N] of labels is taken as given).  K is 2 .. 32, and every fold needs at least p rows.
    max_samples, batch_size, tolerance, seed, method, perms, antithetical:  as in ``ls_spa_multi_sampled``; ``seed`` seeds
        the ordering source.  With ``tolerance`` sampling stops after the first batch with n >= 2 whose largest
        standard error of the SUMMED attribution is <= tolerance.
    groups:  one integer label per column as ``ls_spa_groups`` takes them (-1: the baseline, 0 .. g-1, any 1 <= g <= p).
        The players are then the groups, the sources run in dimension g, ``perms`` are group orderings, and the result
        is a ``SampledCVGroupResults``.

    Returns ``SampledCVResults``: ``attribution`` [d] (sums to ``r_squared``, over groups to ``r_squared -
    baseline_r_squared``), ``attribution_errors`` [d], ``fold_attribution`` [K][d] (its rows sum to ``attribution``),
    ``fold_attribution_errors`` [K][d], ``r_squared``, ``fold_r_squared`` [K], ``theta`` [p] (fitted on all rows),
    ``fold_ids`` and ``n_samples``.

    Shapes that do not fit, p > 127, K outside 2 .. 32, a label out of range, an empty fold, a fold with fewer than p
    rows, a y that is identically zero, bad group labels and ``perms`` together with ``method`` are refused before any
    GPU work.  A fold problem that is not numerically positive definite raises a RuntimeWarning that names the folds.
    Several ranks, checkpoints, fp32, the device error estimator and the history are not part of this function."""
    X, y = np.asarray(X), np.asarray(y)
    if X.ndim != 2 or y.ndim != 1:
        raise ValueError("ls_spa_cv_sampled: X must be two-dimensional and y one-dimensional")
    if X.shape[0] != y.shape[0]:
        raise SizeIncompatible(f"X has {X.shape[0]} rows, y has {y.shape[0]}")
    n_rows, p = X.shape
    if p > CV_LIFT_MAX_P:
        raise ValueError(f"ls_spa_cv_sampled takes at most p = {CV_LIFT_MAX_P} features (this problem has p = {p})")
    if p < 1 or n_rows < 2:
        raise ValueError(f"ls_spa_cv_sampled needs p >= 1 features and N >= 2 rows (p = {p}, N = {n_rows})")
    ids, K = cv_fold_ids(n_rows, folds, seed=fold_seed, shuffle=shuffle)
    sizes = np.bincount(ids, minlength=K)
    if (sizes < p).any():
        f = int(np.argmax(sizes < p))
        raise ValueError(f"fold {f} of {K} has {int(sizes[f])} rows, fewer than p = {p}: the Gram matrix of a fold's own "
                         "rows must have a Cholesky factor")
    if not np.any(y):
        raise ValueError("y is identically zero: the cross-validated R^2 is not defined")
    labels, d, source, batch_size, antithetical, max_samples, never_stop = _sampled_arguments(
        p, groups, perms, method, max_samples, batch_size, seed, antithetical)
    if never_stop:
        tolerance = None
    undo = [(lambda: _close_source(source), True)]
    with _engine_call(_engine, device, undo=undo) as engine:
        undo.append((engine.cv_lift_free, True))
        engine.cv_lift_load(X, y, ids, K, reg)
        if labels is not None:
            engine.cv_lift_set_players(labels)      # (cv_lift_free drops the map with everything else)
        n, mean, m2 = _sample_until(source, lambda rows: engine.cv_lift_batch(rows, antithetical), engine.cv_lift_get,
                                    lambda state: _multi_standard_errors(state[0], state[2][K]).max(), batch_size,
                                    max_samples, tolerance)
        info = engine.cv_lift_info()
        problems = [engine.cv_lift_problem(f) for f in range(K)]
    r2_fold = _cv_fold_values(problems, np.arange(p))
    base_cols = np.zeros(0, dtype=np.int64) if labels is None else np.nonzero(np.asarray(labels) == -1)[0]
    base_fold = _cv_fold_values(problems, base_cols)
    r_squared, base = float(_seq_sum(list(r2_fold))), float(_seq_sum(list(base_fold)))
    _cv_verdict(info, stacklevel=2)
    # every sample's lifts of fold f telescope from the baseline's value to the full model's, so the mean of the sums
    # does (the bound of LSSPA_INFO_SUM for well-conditioned data)
    if not (np.asarray(info) & 1).any() and not abs(mean[K].sum() - (r_squared - base)) <= 1e-9 * max(1.0, abs(r_squared)):
        _info_verdict(8, stacklevel=2)
    errors = _multi_standard_errors(n, m2)
    G, g = _cv_full_problem(X, y, reg)
    common = dict(attribution=mean[K], attribution_errors=errors[K], fold_attribution=mean[:K],
                  fold_attribution_errors=errors[:K], r_squared=r_squared, fold_r_squared=r2_fold,
                  theta=_subset_fit(G, g, np.arange(p)), fold_ids=ids, n_samples=int(n))
    if labels is not None:
        return SampledCVGroupResults(baseline_r_squared=base, fold_baseline_r_squared=base_fold, **common)
    return SampledCVResults(**common)


CV_PATH_MAX_REGS = 256     # include/lsspa.h, lsspa_cv_path_shapley


def _cv_path_regs(regs):
    """The ridge values of ``ls_spa_cv_path`` as a float64 array [L], or the ValueError that names what is wrong."""
    try:
        r = np.asarray(regs, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError("regs must be a one-dimensional sequence of numbers") from None
    if r.ndim != 1:
        raise ValueError(f"regs must be one-dimensional (got {r.ndim} dimensions)")
    if not 1 <= r.shape[0] <= CV_PATH_MAX_REGS:
        raise ValueError(f"ls_spa_cv_path takes 1 .. {CV_PATH_MAX_REGS} ridge values (got {r.shape[0]})")
    bad = np.nonzero(~np.isfinite(r) | (r < 0))[0]
    if len(bad):
        raise ValueError(f"regs[{int(bad[0])}] = {float(r[bad[0]])!r}: a ridge value must be finite and >= 0")
    return np.ascontiguousarray(r)


def _cv_path_verdict(info, regs, what, stacklevel):
    """_cv_verdict / _cv_group_verdict for a path: the RuntimeWarning names the ridge values and, for each, the folds.
    what: the words of the one-value warning for what is no candidate."""
    info = np.asarray(info)
    rows = [l for l in range(info.shape[0]) if (info[l] & 1).any()]
    if rows:
        named = "; ".join(f"ridge value {regs[l]:g} (regs[{l}]): fold(s) "
                          f"{', '.join(str(int(f)) for f in np.nonzero(info[l] & 1)[0])}" for l in rows)
        warnings.warn(f"a Gram matrix of the training rows was not numerically positive definite at {named}; {what} "
                      "are no candidates there and their attribution is not meaningful", RuntimeWarning,
                      stacklevel=stacklevel + 1)


def _cv_path_choice(regs, r_squared, fold_r_squared):
    """(best_index, best_reg, best_gap [L], best_gap_std_error [L], within_one_se [L], one_se_index, one_se_reg) of a
    path, in fp64 on the host from the per-fold values alone.  The best row: the largest r_squared, on equal values
    the larger ridge value (then the earlier row), NaN rows skipped; -1 and NaN if there is none.  Against it
    d_f = fold[best][f] - fold[l][f]: their sum, sqrt(K) std(d, ddof=1), and the largest ridge value whose sum is
    within that (``ls_spa_top_subsets_cv``'s rule, with the stronger penalty in the place of the smaller model)."""
    L, K = fold_r_squared.shape
    best_gap, std_error, within = np.full(L, np.nan), np.full(L, np.nan), np.zeros(L, dtype=bool)
    valid = np.nonzero(~np.isnan(r_squared))[0]
    if not len(valid):
        return -1, float("nan"), best_gap, std_error, within, -1, float("nan")
    top = valid[r_squared[valid] == r_squared[valid].max()]
    best = int(top[np.argmax(regs[top])])
    d = fold_r_squared[best][None, :] - fold_r_squared
    best_gap[valid] = d.sum(axis=1)[valid]
    std_error[valid] = (np.sqrt(K) * np.std(d, axis=1, ddof=1))[valid]
    within[valid] = best_gap[valid] <= std_error[valid]
    ok = np.nonzero(within)[0]                   # never empty: the best row's gap and error are both 0
    one_se = int(ok[np.argmax(regs[ok])])
    return best, float(regs[best]), best_gap, std_error, within, one_se, float(regs[one_se])


def ls_spa_cv_path(X, y, regs, folds=5, *, groups=None, seed=42, shuffle=True, device=0, _engine=None):
    """``ls_spa_cv`` along a path of ridge values: the exact Shapley attribution of the K-fold cross-validated R^2 for
    every ``regs[l]``, and which of them the folds prefer.

    The cross-validated R^2 and the attribution both move with the ridge parameter -- with collinear columns credit
    moves between correlated features as it grows -- and none of the other calls helps choose it.  The parameter enters
    a fold problem only as + reg on the diagonal of its training Gram, so the path is ONE load and ONE weighted Gram
    pass: the L K fold problems are written from the kept per-fold Grams on the device and enumerated as replicates
    of shared grids (include/lsspa.h, lsspa_cv_path_shapley).  Row l of every per-value field is what
    ``ls_spa_cv(X, y, reg=regs[l], ...)`` returns, bit for bit, whatever L and the position of l.

    regs:  1 .. 256 finite ridge values >= 0, in any order (repeats allowed).
    folds, groups, seed, shuffle:  as for ``ls_spa_cv``.

    Returns ``CVPathResults``: ``regs`` [L] in the caller's order, ``attribution`` [L][p], ``fold_attribution``
    [L][K][p], ``r_squared`` [L], ``fold_r_squared`` [L][K], ``theta`` [L][p] (each row refitted on all rows on the host
    in fp64) and ``fold_ids`` [N]; with ``groups=`` ``CVGroupPathResults``: the attributions over the g groups, plus
    ``baseline_r_squared`` [L] and ``fold_baseline_r_squared`` [L][K] (a row of ``attribution`` sums to ``r_squared -
    baseline_r_squared``).

    The choice of the parameter, computed on the host in fp64 from ``fold_r_squared`` alone: ``best_index`` /
    ``best_reg``, the largest ``r_squared`` (on equal values the larger ridge value; NaN rows are skipped); with
    d_f = fold_r_squared[best][f] - fold_r_squared[l][f] -- paired differences, every fold over the same pooled
    ||y||^2 -- ``best_gap`` [L] = their sum, ``best_gap_std_error`` [L] = sqrt(K) std(d, ddof=1), ``within_one_se``
    [L] = best_gap <= best_gap_std_error, and ``one_se_index`` / ``one_se_reg``, the largest ridge value within one
    standard error of the best (the best itself always is).  K folds are few and their training sets overlap, so the
    d_f are neither many nor independent: this is the usual one-standard-error heuristic for preferring the stronger
    penalty, not a test, and no p-value should be read from it.

    The refusals of ``ls_spa_cv`` (of ``ls_spa_cv(groups=)``) and a ``regs`` that is not one-dimensional, has no or
    more than 256 entries or a negative or non-finite one -- the ValueError names the entry -- come before any GPU
    work.  A fold problem whose training Gram is not numerically positive definite raises a RuntimeWarning that names
    the ridge values and their folds; the other rows are not affected.  Not built: a path of the selection and
    top-list calls, interactions, a bootstrap over the folds."""
    grouped = groups is not None
    X, y, ids, K = _cv_data("ls_spa_cv_path", X, y, folds, seed, shuffle, grouped=grouped)
    p = X.shape[1]
    if grouped:
        labels, n_groups = group_labels(groups, p)
    regs = _cv_path_regs(regs)
    with _engine_call(_engine, device) as engine:
        if grouped:
            engine.cv_groups_load(X, y, ids, K, float(regs[0]))
        else:
            engine.cv_load(X, y, ids, K, float(regs[0]))
        try:
            if grouped:
                phi, phi_fold, r2_fold, base_fold, info = engine.cv_path_groups_shapley(labels, regs)
            else:
                phi, phi_fold, r2_fold, info = engine.cv_path_shapley(regs)
        finally:
            engine.cv_free()
    _cv_path_verdict(info, regs, "sets of groups with collinear columns" if grouped else
                     "subsets of collinear features", stacklevel=2)
    r2_fold = np.asarray(r2_fold)
    r_squared = np.array([float(_seq_sum(list(row))) for row in r2_fold])
    theta = np.empty((len(regs), p))
    for l, r in enumerate(regs):
        G, g = _cv_full_problem(X, y, float(r))
        theta[l] = _subset_fit(G, g, np.arange(p))
    best, best_reg, best_gap, std_error, within, one_se, one_se_reg = _cv_path_choice(regs, r_squared, r2_fold)
    choice = dict(best_index=best, best_reg=best_reg, best_gap=best_gap, best_gap_std_error=std_error,
                  within_one_se=within, one_se_index=one_se, one_se_reg=one_se_reg)
    if grouped:
        base_fold = np.asarray(base_fold)
        return CVGroupPathResults(regs=regs, attribution=phi, fold_attribution=phi_fold, r_squared=r_squared,
                                  fold_r_squared=r2_fold,
                                  baseline_r_squared=np.array([float(_seq_sum(list(row))) for row in base_fold]),
                                  fold_baseline_r_squared=base_fold, theta=theta, fold_ids=ids, **choice)
    return CVPathResults(regs=regs, attribution=phi, fold_attribution=phi_fold, r_squared=r_squared,
                         fold_r_squared=r2_fold, theta=theta, fold_ids=ids, **choice)


def ls_spa_best_subsets_cv(X, y, reg=0., folds=5, *, include=None, groups=None, seed=42, shuffle=True, device=0,
                           _engine=None):
    """Exhaustive best-subset selection by the K-fold cross-validated R^2: the best model of every size over all 2^p
    feature subsets (p <= 32), judged not by one split but by all K.

    ``ls_spa_best_subsets`` keeps the model that wins on one train / test split, and
    ``ls_spa_best_subsets_bootstrap`` shows how unstable that choice is.  Here a subset's value is
    v_cv(S) = sum_f v_f(S), fold f predicted by the model on S fitted on the other folds' rows, every fold over the
    pooled ||y||^2.  Selection is not linear in the game: the K values of a subset have to be added before the
    comparison, so a kernel of its own evaluates every subset on all K fold problems and keeps per size the largest
    sum and its subset (fp64, the folds added in ascending order, bitwise reproducible; include/lsspa.h,
    lsspa_cv_best).  On equal values the subset with the smaller mask (bit j = feature j) wins.

    folds, seed, shuffle:  as for ``ls_spa_cv``.   include:  as for ``ls_spa_best_subsets``.

    Returns ``CVBestSubsetsResults``: ``sizes``, ``subsets`` [n][p] bool, ``r_squared`` [n] (the cross-validated value),
    ``fold_r_squared`` [n][K] (the winner's per-fold values, summing to it), ``theta`` [n][p] (each winner refitted on
    ALL rows on the host in fp64, exactly 0.0 outside its subset), ``best_size`` (the smallest size on ties, NaN rows
    skipped), ``best_subset``, ``full_r_squared`` (the cross-validated R^2 of all p columns) and ``fold_ids``.

    The refusals of ``ls_spa_cv`` and those of ``include`` come before any GPU work.  A subset with a pivot that failed
    in any fold is no candidate and raises a RuntimeWarning that names the folds; a size without a candidate is a NaN
    row.

    groups:  labels as for ``ls_spa_cv(groups=)``.  The models are then the 2^g sets of groups, each with the baseline's
        columns, a model's size is its number of groups, 0 .. g (size 0 is the baseline alone), and on equal values the
        set with the smaller mask (bit k = group k) wins (include/lsspa.h, lsspa_cv_groups_best; g <= 32, p <= 64).
        ``include=`` cannot be combined with it: label those columns -1.  Returns ``CVBestGroupSubsetsResults``: the
        fields of ``BestGroupSubsetsResults`` with the cross-validated value, and ``fold_r_squared`` [g + 1][K] and
        ``fold_ids``."""
    if groups is not None:
        if include is not None:
            raise ValueError("include= cannot be combined with groups=: label the columns every model must contain "
                             "-1, the baseline is the include set")
        X, y, ids, K = _cv_data("ls_spa_best_subsets_cv", X, y, folds, seed, shuffle, grouped=True)
        labels, n_groups = group_labels(groups, X.shape[1])
        return _cv_best_group_subsets(X, y, reg, ids, K, labels, n_groups, device, _engine)
    X, y, ids, K = _cv_data("ls_spa_best_subsets_cv", X, y, folds, seed, shuffle)
    p = X.shape[1]
    mask, inc = include_mask(include, p)
    with _engine_call(_engine, device) as engine:
        engine.cv_load(X, y, ids, K, reg)
        try:
            v, masks, found, v_fold, info = engine.cv_best(mask)
            full, _ = engine.debug_cv_values(np.array([(1 << p) - 1], dtype=np.uint64), folds=False)
        finally:
            engine.cv_free()
    _cv_verdict(info, stacklevel=2)
    G, g = _cv_full_problem(X, y, reg)
    sizes = np.arange(len(inc), p + 1)
    n = len(sizes)
    subsets = np.zeros((n, p), dtype=bool)
    r_squared = np.full(n, np.nan)
    fold_r_squared = np.full((n, K), np.nan)
    theta = np.full((n, p), np.nan)
    for i, k in enumerate(sizes):
        if found[k]:
            subsets[i] = (int(masks[k]) >> np.arange(p)) & 1
            r_squared[i] = v[k]
            fold_r_squared[i] = v_fold[k]
            theta[i] = _subset_fit(G, g, np.nonzero(subsets[i])[0])
    best_size, best_subset = -1, np.zeros(p, dtype=bool)
    if not np.all(np.isnan(r_squared)):
        i = int(np.nanargmax(r_squared))      # the first of equal maxima: the smallest size
        best_size, best_subset = int(sizes[i]), subsets[i].copy()
    return CVBestSubsetsResults(sizes=sizes, subsets=subsets, r_squared=r_squared, fold_r_squared=fold_r_squared,
                                theta=theta, best_size=best_size, best_subset=best_subset,
                                full_r_squared=float(full[0]), fold_ids=ids)


SUBSETS_TOP_MAX = 16       # include/lsspa.h, lsspa_subsets_top: ranks per size


def ls_spa_top_subsets(X_train, X_test, y_train, y_test, reg=0., n_best=10, *, include=None, device=0, _engine=None):
    """The ``n_best`` best models of every size by out-of-sample R^2, over all 2^p feature subsets (p <= 32): how much
    worse is the next model?

    ``ls_spa_best_subsets`` names one winner per size; with collinear regressors the runner-up often differs from it
    by one swapped feature and 1e-4 of R^2.  This call runs the same enumeration (fp64, bitwise reproducible;
    include/lsspa.h, lsspa_subsets_top) and keeps per size the ``n_best`` (1 .. 16) best subsets, best first: the
    larger R^2, on equal values the subset with the smaller mask (bit j = feature j).  Rank 0 of every size is
    ``ls_spa_best_subsets``'s winner, bit for bit.

    include:  an iterable of column indices that every model must contain, as for ``ls_spa_best_subsets``; the sizes
        then start at len(include).

    Returns ``TopSubsetsResults``: ``sizes`` [n], ``n_models`` [n] (the valid ranks of a size: min(n_best, the number
    of subsets of that size)), ``subsets`` [n][n_best][p] bool, ``r_squared`` [n][n_best] (descending along a row),
    ``theta`` [n][n_best][p] (each listed model refitted on the host in fp64, exactly 0.0 outside its subset), ``gap``
    [n][n_best] (``r_squared[:, :1] - r_squared``: the price of each alternative), ``top_sizes``, ``top_subsets``,
    ``top_r_squared`` (the n_best best models over all sizes) and ``best_size``, ``best_subset``, ``full_r_squared``,
    which are ``ls_spa_best_subsets``'s.  Ranks past ``n_models`` are NaN (False in ``subsets``).

    p > 32, an ``n_best`` that is not an integer in 1 .. 16, an ``include`` out of range or with duplicates, shapes that
    do not fit and a ``y_test`` that is identically zero are refused before any GPU work.  A subset whose Gram matrix
    is not numerically positive definite is no candidate and raises the RuntimeWarning of ``ls_spa(method='subsets')``.
    ``reg`` and ``device`` are that call's.  Top lists over groups of columns (a one-hot factor, a spline basis; more
    than 32 columns) are a call of their own, ``ls_spa_top_group_subsets``.  Not built: a bootstrap of the top list."""
    data = _coerce_data(X_train, X_test, y_train, y_test)
    p = data[0].shape[1]
    if p > SUBSETS_MAX_P:
        raise ValueError(f"ls_spa_top_subsets enumerates all 2^p feature subsets and takes at most p = {SUBSETS_MAX_P} "
                         f"features (this problem has p = {p})")
    if p < 1 or data[1].shape[0] < 1:
        raise ValueError(f"ls_spa_top_subsets needs p >= 1 features and M >= 1 test rows (p = {p}, "
                         f"M = {data[1].shape[0]})")
    if isinstance(n_best, (bool, np.bool_)) or not isinstance(n_best, (int, np.integer)) \
            or not 1 <= n_best <= SUBSETS_TOP_MAX:
        raise ValueError(f"n_best must be an integer in 1 .. {SUBSETS_TOP_MAX} (got {n_best!r})")
    T = int(n_best)
    mask, inc = include_mask(include, p)
    if not np.any(data[3]):
        raise ValueError("y_test is identically zero: the out-of-sample R^2 is not defined")
    with _engine_call(_engine, device) as engine:
        # precision stays set on a kept engine: theta and r_squared come from its fp64 factorisation, like the values
        if getattr(engine, "precision", "float64") != "float64":
            engine.set_precision("float64")
        _, full_r_squared, info = _load_and_fit(engine, data, reg, False, None)
        v, masks, count, bits = engine.subsets_top(mask, T)
        if info & 1:
            _, full_r_squared = _singular_fit(engine, data[1], data[3])
        G, g, _, _ = engine.gram()
    _info_verdict((bits | info) & 1, stacklevel=2)      # (an enumeration reports a broken pivot, nothing else)
    sizes = np.arange(len(inc), p + 1)
    n = len(sizes)
    n_models = np.asarray(count)[sizes].astype(np.int64)
    subsets = np.zeros((n, T, p), dtype=bool)
    r_squared = np.full((n, T), np.nan)
    theta = np.full((n, T, p), np.nan)
    for i, k in enumerate(sizes):
        for r in range(n_models[i]):
            subsets[i, r] = (int(masks[k, r]) >> np.arange(p)) & 1
            r_squared[i, r] = v[k, r]
            theta[i, r] = _subset_fit(G, g, np.nonzero(subsets[i, r])[0])
    # the best over all sizes lie inside the per-size lists: a merge under the same order, larger value then smaller mask
    ii, rr = np.nonzero(np.arange(T)[None, :] < n_models[:, None])
    order = np.lexsort((np.asarray(masks)[sizes[ii], rr], -r_squared[ii, rr]))[:T]
    best_size, best_subset = -1, np.zeros(p, dtype=bool)
    if n_models.any():
        i = int(np.nanargmax(r_squared[:, 0]))      # the first of equal maxima: the smallest size
        best_size, best_subset = int(sizes[i]), subsets[i, 0].copy()
    return TopSubsetsResults(sizes=sizes, n_models=n_models, subsets=subsets, r_squared=r_squared, theta=theta,
                             gap=r_squared[:, :1] - r_squared, top_sizes=sizes[ii[order]],
                             top_subsets=subsets[ii[order], rr[order]], top_r_squared=r_squared[ii[order], rr[order]],
                             best_size=best_size, best_subset=best_subset, full_r_squared=float(full_r_squared))


def _one_se_fields(r_squared, fold_r_squared, n_models, best_row):
    """(best_gap, best_gap_std_error, within_one_se) [n][T] of the listed models against the overall best one, rank 0 of
    row ``best_row`` (-1: no model at all), in fp64 from the per-fold values alone: d_f = fold[b][f] - fold[i, r][f],
    the standard error of their sum over K folds is sqrt(K) std(d, ddof=1)."""
    n, T, K = fold_r_squared.shape
    best_gap = np.full((n, T), np.nan)
    std_error = np.full((n, T), np.nan)
    within = np.zeros((n, T), dtype=bool)
    if best_row < 0:
        return best_gap, std_error, within
    listed = np.arange(T)[None, :] < np.asarray(n_models)[:, None]
    d = fold_r_squared[best_row, 0][None, None, :] - fold_r_squared
    best_gap[listed] = (r_squared[best_row, 0] - r_squared)[listed]
    std_error[listed] = (np.sqrt(K) * np.std(d, axis=2, ddof=1))[listed]
    within[listed] = best_gap[listed] <= std_error[listed]
    return best_gap, std_error, within


def ls_spa_top_group_subsets_cv(X, y, groups, reg=0., folds=5, n_best=10, *, seed=42, shuffle=True, device=0,
                                _engine=None):
    """The ``n_best`` best models of every size by the K-fold cross-validated R^2, over all 2^g sets of groups of columns
    (g <= 32 groups over p <= 64 columns): ``ls_spa_top_subsets_cv`` for a design matrix with an intercept, a one-hot
    factor or a spline basis among its columns -- there the column call cannot be used correctly: the intercept
    competes as a feature, a factor's dummies are listed one by one, and p <= 32 is a hard wall.

    ``ls_spa_top_group_subsets`` lists the near-best sets of groups of one train / test split,
    ``ls_spa_best_subsets_cv(groups=)`` names one winner per size by u_cv(S) = sum_f u_f(S).  This call is their
    product: the enumeration takes every set of groups through all K fold problems, adds the K values in ascending
    order and keeps per size the ``n_best`` (1 .. 16) largest sums, best first, on equal values the set with the smaller
    mask (bit k = group k) first (fp64, bitwise reproducible; include/lsspa.h, lsspa_cv_groups_top).  Rank 0 of every
    size is ``ls_spa_best_subsets_cv(groups=)``'s winner, bit for bit.  K calls of ``ls_spa_top_group_subsets`` could
    not be merged into this: a set that is 17th in every fold can be first in the sum.

    groups:  one label per column as ``ls_spa_cv(groups=)`` takes them: k in 0 .. g-1 puts the column into group k, -1
        into the baseline that every model contains.  There is no ``include=``: the baseline is the include set.
    folds, seed, shuffle:  as for ``ls_spa_cv``.   n_best:  as for ``ls_spa_top_group_subsets``.

    Returns ``TopGroupSubsetsCVResults``: the fields of ``TopGroupSubsetsResults`` with the cross-validated value --
    ``sizes`` 0 .. g (size 0 is the baseline alone), ``n_models`` [n], ``group_subsets`` [n][n_best][g] bool, ``subsets``
    [n][n_best][p] bool (the baseline's and the listed groups' columns), ``n_columns``, ``r_squared`` [n][n_best],
    ``theta`` [n][n_best][p] (each listed model refitted on ALL rows on the host in fp64, exactly 0.0 outside its
    columns), ``gap``, ``top_sizes``, ``top_group_subsets``, ``top_subsets``, ``top_r_squared``, ``best_size``,
    ``best_group_subset``, ``best_subset``, ``full_r_squared``, ``baseline_r_squared`` -- plus ``fold_r_squared``
    [n][n_best][K], ``fold_ids`` [N] and the one-standard-error fields of ``ls_spa_top_subsets_cv``, computed the same
    way from ``fold_r_squared`` alone: ``best_gap``, ``best_gap_std_error``, ``within_one_se``, ``one_se_size``,
    ``one_se_group_subset`` and ``one_se_subset``.  Ranks past ``n_models`` are NaN (False in the subsets, 0 in
    ``n_columns``).

    The refusals of ``ls_spa_cv(groups=)`` (shapes, p > 64, folds, a zero y, bad labels, g > 32) and that of ``n_best``
    come before any GPU work.  A set of groups with a pivot that failed in any fold is no candidate and raises a
    RuntimeWarning that names the folds.  Not built: a bootstrap of the list."""
    X, y, ids, K = _cv_data("ls_spa_top_group_subsets_cv", X, y, folds, seed, shuffle, grouped=True)
    p = X.shape[1]
    labels, g = group_labels(groups, p)
    if isinstance(n_best, (bool, np.bool_)) or not isinstance(n_best, (int, np.integer)) \
            or not 1 <= n_best <= GROUPS_TOP_MAX:
        raise ValueError(f"n_best must be an integer in 1 .. {GROUPS_TOP_MAX} (got {n_best!r})")
    T = int(n_best)
    with _engine_call(_engine, device) as engine:
        engine.cv_groups_load(X, y, ids, K, reg)
        try:
            u, masks, count, u_fold, info = engine.cv_groups_top(labels, T)
            full, _ = engine.debug_cv_group_values(labels, np.array([(1 << g) - 1], dtype=np.uint64), folds=False)
        finally:
            engine.cv_free()
    _cv_group_verdict(info, stacklevel=2)
    G, gv = _cv_full_problem(X, y, reg)
    sizes = np.arange(g + 1)
    n = g + 1
    n_models = np.asarray(count).astype(np.int64)
    group_subsets = np.zeros((n, T, g), dtype=bool)
    subsets = np.zeros((n, T, p), dtype=bool)
    r_squared = np.full((n, T), np.nan)
    fold_r_squared = np.full((n, T, K), np.nan)
    theta = np.full((n, T, p), np.nan)
    for k in sizes:
        for r in range(n_models[k]):
            group_subsets[k, r] = (int(masks[k, r]) >> np.arange(g)) & 1
            subsets[k, r] = (labels < 0) | group_subsets[k, r][np.maximum(labels, 0)]
            r_squared[k, r] = u[k, r]
            fold_r_squared[k, r] = u_fold[k, r]
            theta[k, r] = _subset_fit(G, gv, np.nonzero(subsets[k, r])[0])
    # the best over all sizes lie inside the per-size lists: a merge under the same order, larger value then smaller mask
    ii, rr = np.nonzero(np.arange(T)[None, :] < n_models[:, None])
    order = np.lexsort((np.asarray(masks)[ii, rr], -r_squared[ii, rr]))[:T]
    best_size, best_groups, best_subset = -1, np.zeros(g, dtype=bool), np.zeros(p, dtype=bool)
    if n_models.any():
        best_size = int(np.nanargmax(r_squared[:, 0]))      # the first of equal maxima: the smallest size
        best_groups, best_subset = group_subsets[best_size, 0].copy(), subsets[best_size, 0].copy()
    best_gap, std_error, within = _one_se_fields(r_squared, fold_r_squared, n_models, best_size)
    one_se_size, one_se_groups, one_se_subset = -1, np.zeros(g, dtype=bool), np.zeros(p, dtype=bool)
    if best_size >= 0:
        one_se_size = int(np.argmax(within[:, 0]))          # the first size that qualifies; best_size's own row does
        one_se_groups, one_se_subset = group_subsets[one_se_size, 0].copy(), subsets[one_se_size, 0].copy()
    return TopGroupSubsetsCVResults(sizes=sizes, n_models=n_models, group_subsets=group_subsets, subsets=subsets,
                                    n_columns=subsets.sum(axis=2), r_squared=r_squared,
                                    fold_r_squared=fold_r_squared, theta=theta, gap=r_squared[:, :1] - r_squared,
                                    top_sizes=sizes[ii[order]], top_group_subsets=group_subsets[ii[order], rr[order]],
                                    top_subsets=subsets[ii[order], rr[order]],
                                    top_r_squared=r_squared[ii[order], rr[order]], best_size=best_size,
                                    best_group_subset=best_groups, best_subset=best_subset,
                                    full_r_squared=float(full[0]), baseline_r_squared=float(r_squared[0, 0]),
                                    best_gap=best_gap, best_gap_std_error=std_error, within_one_se=within,
                                    one_se_size=one_se_size, one_se_group_subset=one_se_groups,
                                    one_se_subset=one_se_subset, fold_ids=ids)


def ls_spa_top_subsets_cv(X, y, reg=0., folds=5, n_best=10, *, include=None, seed=42, shuffle=True, device=0,
                          _engine=None):
    """The ``n_best`` best models of every size by the K-fold cross-validated R^2, over all 2^p feature subsets
    (p <= 32): how much worse is the next model when all K folds judge -- and can the folds tell them apart at all?

    ``ls_spa_top_subsets`` lists the near-best models of one train / test split, ``ls_spa_best_subsets_cv`` names one
    winner per size by v_cv(S) = sum_f v_f(S).  This call is their product: the enumeration evaluates every subset on
    all K fold problems, adds the K values in ascending order and keeps per size the ``n_best`` (1 .. 16) largest sums,
    best first, on equal values the subset with the smaller mask (bit j = feature j) first (fp64, bitwise
    reproducible; include/lsspa.h, lsspa_cv_top).  Rank 0 of every size is ``ls_spa_best_subsets_cv``'s winner, bit for
    bit.  K calls of ``ls_spa_top_subsets`` could not be merged into this: a subset that is 17th in every fold can be
    first in the sum.

    folds, seed, shuffle:  as for ``ls_spa_cv``.   n_best, include:  as for ``ls_spa_top_subsets``.

    Returns ``TopSubsetsCVResults``: the fields of ``TopSubsetsResults`` with the cross-validated value -- ``sizes`` [n],
    ``n_models`` [n], ``subsets`` [n][n_best][p] bool, ``r_squared`` [n][n_best], ``theta`` [n][n_best][p] (each listed
    model refitted on ALL rows on the host in fp64, exactly 0.0 outside its subset), ``gap`` [n][n_best]
    (``r_squared[:, :1] - r_squared``), ``top_sizes``, ``top_subsets``, ``top_r_squared``, ``best_size``,
    ``best_subset``, ``full_r_squared`` (the cross-validated R^2 of all p columns) -- plus ``fold_r_squared``
    [n][n_best][K] (a listed model's per-fold values, summing to its ``r_squared``) and ``fold_ids`` [N].  Ranks past
    ``n_models`` are NaN (False in ``subsets``).

    What the folds add, computed on the host in fp64 from ``fold_r_squared`` alone.  With b the overall best model
    (rank 0 of ``best_size``) and d_f = fold_r_squared[b][f] - fold_r_squared[i, r][f] -- paired differences, every
    fold over the same pooled ||y||^2 --: ``best_gap`` [n][n_best] = r_squared[b] - r_squared[i, r],
    ``best_gap_std_error`` [n][n_best] = sqrt(K) std(d, ddof=1), ``within_one_se`` [n][n_best] = best_gap <=
    best_gap_std_error (False past ``n_models``), ``one_se_size``: the smallest size whose rank 0 is within one
    standard error of the best (``best_size`` always qualifies) and ``one_se_subset``, that size's rank-0 subset.
    K folds are few and their training sets overlap, so the d_f are neither many nor independent: this is the usual
    one-standard-error heuristic for preferring the smaller model, not a test, and no p-value should be read from it.

    The refusals of ``ls_spa_cv`` and those of ``n_best`` and ``include`` come before any GPU work.  A subset with a
    pivot that failed in any fold is no candidate and raises a RuntimeWarning that names the folds.  There is no
    ``groups=``: top lists of the cross-validated value over groups of columns (a one-hot factor, a spline basis; more
    than 32 columns) are a call of their own, ``ls_spa_top_group_subsets_cv``.  Not built: a bootstrap of the list."""
    X, y, ids, K = _cv_data("ls_spa_top_subsets_cv", X, y, folds, seed, shuffle)
    p = X.shape[1]
    if isinstance(n_best, (bool, np.bool_)) or not isinstance(n_best, (int, np.integer)) \
            or not 1 <= n_best <= SUBSETS_TOP_MAX:
        raise ValueError(f"n_best must be an integer in 1 .. {SUBSETS_TOP_MAX} (got {n_best!r})")
    T = int(n_best)
    mask, inc = include_mask(include, p)
    with _engine_call(_engine, device) as engine:
        engine.cv_load(X, y, ids, K, reg)
        try:
            v, masks, count, v_fold, info = engine.cv_top(mask, T)
            full, _ = engine.debug_cv_values(np.array([(1 << p) - 1], dtype=np.uint64), folds=False)
        finally:
            engine.cv_free()
    _cv_verdict(info, stacklevel=2)
    G, g = _cv_full_problem(X, y, reg)
    sizes = np.arange(len(inc), p + 1)
    n = len(sizes)
    n_models = np.asarray(count)[sizes].astype(np.int64)
    subsets = np.zeros((n, T, p), dtype=bool)
    r_squared = np.full((n, T), np.nan)
    fold_r_squared = np.full((n, T, K), np.nan)
    theta = np.full((n, T, p), np.nan)
    for i, k in enumerate(sizes):
        for r in range(n_models[i]):
            subsets[i, r] = (int(masks[k, r]) >> np.arange(p)) & 1
            r_squared[i, r] = v[k, r]
            fold_r_squared[i, r] = v_fold[k, r]
            theta[i, r] = _subset_fit(G, g, np.nonzero(subsets[i, r])[0])
    # the best over all sizes lie inside the per-size lists: a merge under the same order, larger value then smaller mask
    ii, rr = np.nonzero(np.arange(T)[None, :] < n_models[:, None])
    order = np.lexsort((np.asarray(masks)[sizes[ii], rr], -r_squared[ii, rr]))[:T]
    best_row, best_size, best_subset = -1, -1, np.zeros(p, dtype=bool)
    if n_models.any():
        best_row = int(np.nanargmax(r_squared[:, 0]))      # the first of equal maxima: the smallest size
        best_size, best_subset = int(sizes[best_row]), subsets[best_row, 0].copy()
    best_gap, std_error, within = _one_se_fields(r_squared, fold_r_squared, n_models, best_row)
    one_se_size, one_se_subset = -1, np.zeros(p, dtype=bool)
    if best_row >= 0:
        i = int(np.argmax(within[:, 0]))                   # the first size that qualifies; best_size's own row does
        one_se_size, one_se_subset = int(sizes[i]), subsets[i, 0].copy()
    return TopSubsetsCVResults(sizes=sizes, n_models=n_models, subsets=subsets, r_squared=r_squared,
                               fold_r_squared=fold_r_squared, theta=theta, gap=r_squared[:, :1] - r_squared,
                               top_sizes=sizes[ii[order]], top_subsets=subsets[ii[order], rr[order]],
                               top_r_squared=r_squared[ii[order], rr[order]], best_size=best_size,
                               best_subset=best_subset, full_r_squared=float(full[0]), best_gap=best_gap,
                               best_gap_std_error=std_error, within_one_se=within, one_se_size=one_se_size,
                               one_se_subset=one_se_subset, fold_ids=ids)


GROUPS_TOP_MAX = 16       # include/lsspa.h, lsspa_groups_top: ranks per size


def ls_spa_top_group_subsets(X_train, X_test, y_train, y_test, groups, reg=0., n_best=10, *, device=0, _engine=None):
    """The ``n_best`` best models of every size by out-of-sample R^2, over all 2^g subsets of groups of columns (g <= 32
    groups over p <= 64 columns): how much worse is the next set of variables?

    ``ls_spa_best_subsets(groups=)`` names one winner per number of groups; two variables that carry nearly the same
    signal make the runner-up differ from it by one swapped variable and 1e-4 of R^2.  This call runs the same
    enumeration (fp64, bitwise reproducible; include/lsspa.h, lsspa_groups_top) and keeps per size the ``n_best``
    (1 .. 16) best sets of groups, best first: the larger R^2, on equal values the set with the smaller mask (bit k =
    group k).  Rank 0 of every size is ``ls_spa_best_subsets(groups=)``'s winner, bit for bit.  The cost is set by g,
    not by p, and the p <= 32 limit of ``ls_spa_top_subsets`` does not apply.

    groups:  one label per column as ``ls_spa_best_subsets(groups=)`` takes them: k in 0 .. g-1 puts the column into
        group k, -1 into the baseline that every model contains.  There is no ``include=``: the baseline is the
        include set.

    Returns ``TopGroupSubsetsResults``: ``sizes`` 0 .. g, ``n_models`` [n] (the valid ranks of a size: min(n_best,
    C(g, size))), ``group_subsets`` [n][n_best][g] bool, ``subsets`` [n][n_best][p] bool (the baseline's and the listed
    groups' columns), ``n_columns`` [n][n_best], ``r_squared`` [n][n_best] (descending along a row), ``theta``
    [n][n_best][p] (each listed model refitted on the host in fp64, exactly 0.0 outside its columns), ``gap``
    [n][n_best] (``r_squared[:, :1] - r_squared``: the price of each alternative), ``top_sizes``,
    ``top_group_subsets``, ``top_subsets``, ``top_r_squared`` (the n_best best models over all sizes) and
    ``best_size``, ``best_group_subset``, ``best_subset``, ``full_r_squared``, ``baseline_r_squared``, which are
    ``ls_spa_best_subsets(groups=)``'s.  Ranks past ``n_models`` are NaN (False in the subsets, 0 in ``n_columns``).

    Bad labels, p > 64, g > 32, an ``n_best`` that is not an integer in 1 .. 16, shapes that do not fit and a ``y_test``
    that is identically zero are refused before any GPU work.  A group subset whose Gram matrix is not numerically
    positive definite is no candidate and raises the RuntimeWarning of ``ls_spa(method='subsets')``.  ``reg`` and
    ``device`` are that call's.  Not built: a bootstrap of the top list."""
    data = _coerce_data(X_train, X_test, y_train, y_test)
    p = data[0].shape[1]
    if p > GROUPS_MAX_P:
        raise ValueError(f"grouped attribution takes at most p = {GROUPS_MAX_P} columns, the baseline's included "
                         f"(this problem has p = {p})")
    labels, g = group_labels(groups, p)
    if isinstance(n_best, (bool, np.bool_)) or not isinstance(n_best, (int, np.integer)) \
            or not 1 <= n_best <= GROUPS_TOP_MAX:
        raise ValueError(f"n_best must be an integer in 1 .. {GROUPS_TOP_MAX} (got {n_best!r})")
    T = int(n_best)
    if data[1].shape[0] < 1:
        raise ValueError(f"ls_spa_top_group_subsets needs M >= 1 test rows (M = {data[1].shape[0]})")
    if not np.any(data[3]):
        raise ValueError("y_test is identically zero: the out-of-sample R^2 is not defined")
    with _engine_call(_engine, device) as engine:
        # precision stays set on a kept engine: theta and r_squared come from its fp64 factorisation, like the values
        if getattr(engine, "precision", "float64") != "float64":
            engine.set_precision("float64")
        _, full_r_squared, info = _load_and_fit(engine, data, reg, False, None)
        u, masks, count, bits = engine.groups_top(labels, T)
        if info & 1:
            _, full_r_squared = _singular_fit(engine, data[1], data[3])
        G, gv, _, _ = engine.gram()
    _info_verdict((bits | info) & 1, stacklevel=2)      # (an enumeration reports a broken pivot, nothing else)
    sizes = np.arange(g + 1)
    n = g + 1
    n_models = np.asarray(count).astype(np.int64)
    group_subsets = np.zeros((n, T, g), dtype=bool)
    subsets = np.zeros((n, T, p), dtype=bool)
    r_squared = np.full((n, T), np.nan)
    theta = np.full((n, T, p), np.nan)
    for k in sizes:
        for r in range(n_models[k]):
            group_subsets[k, r] = (int(masks[k, r]) >> np.arange(g)) & 1
            subsets[k, r] = (labels < 0) | group_subsets[k, r][np.maximum(labels, 0)]
            r_squared[k, r] = u[k, r]
            theta[k, r] = _subset_fit(G, gv, np.nonzero(subsets[k, r])[0])
    # the best over all sizes lie inside the per-size lists: a merge under the same order, larger value then smaller mask
    ii, rr = np.nonzero(np.arange(T)[None, :] < n_models[:, None])
    order = np.lexsort((np.asarray(masks)[ii, rr], -r_squared[ii, rr]))[:T]
    best_size, best_groups, best_subset = -1, np.zeros(g, dtype=bool), np.zeros(p, dtype=bool)
    if n_models.any():
        best_size = int(np.nanargmax(r_squared[:, 0]))      # the first of equal maxima: the smallest size
        best_groups, best_subset = group_subsets[best_size, 0].copy(), subsets[best_size, 0].copy()
    return TopGroupSubsetsResults(sizes=sizes, n_models=n_models, group_subsets=group_subsets, subsets=subsets,
                                  n_columns=subsets.sum(axis=2), r_squared=r_squared, theta=theta,
                                  gap=r_squared[:, :1] - r_squared, top_sizes=sizes[ii[order]],
                                  top_group_subsets=group_subsets[ii[order], rr[order]],
                                  top_subsets=subsets[ii[order], rr[order]],
                                  top_r_squared=r_squared[ii[order], rr[order]], best_size=best_size,
                                  best_group_subset=best_groups, best_subset=best_subset,
                                  full_r_squared=float(full_r_squared), baseline_r_squared=float(r_squared[0, 0]))


MULTI_MAX_COLS = 32767     # include/lsspa.h, lsspa_multi_load: p + m


def _multi_fit(G, g, H, h, yy):
    """(theta [m][p], r_squared [m], singular) of the full model of every response from the reduced form: one host
    Cholesky factor of the p x p G, a solve per response (what lsspa_boot_run does for a replicate's R^2).  singular: G
    has no Cholesky factor, or a pivot of it fails the engine's relative test (16 p eps); theta is then the solution of
    minimal norm, as ls_spa's for a single y."""
    p = G.shape[0]
    try:
        L = np.linalg.cholesky(G)
        singular = bool(np.any(np.diag(L) ** 2 <= 16.0 * p * np.finfo(float).eps * np.diag(G)))
    except np.linalg.LinAlgError:
        singular = True
    if singular:
        theta = np.stack([_min_norm_theta(G, gr) for gr in g])
    else:
        theta = np.linalg.solve(L.T, np.linalg.solve(L, g.T)).T
    r2 = (2.0 * np.einsum("rj,rj->r", theta, h) - np.einsum("ri,ij,rj->r", theta, H, theta)) / yy
    return np.ascontiguousarray(theta), r2, singular


def _multi_baseline_r_squared(G, g, H, h, yy, labels):
    """[m]: every response's R^2 of the baseline columns (label -1) alone, from the reduced form as _multi_fit forms the
    full models'; 0 without a baseline."""
    base = np.nonzero(np.asarray(labels) == -1)[0]
    if len(base) == 0:
        return np.zeros(len(yy))
    sub = np.ix_(base, base)
    return _multi_fit(G[sub], g[:, base], H[sub], h[:, base], yy)[1]


def ls_spa_multi(X_train, X_test, Y_train, Y_test, reg=0., *, groups=None, device=0, _engine=None):
    """Exact Shapley attribution of many responses on one design matrix (p <= 32; with ``groups=``, g <= 32 groups over
    p <= 64 columns).

    ``Y_train`` is [N][m] and ``Y_test`` [M][m] (a one-dimensional y counts as m = 1): the same features explain m
    targets -- a multi-output ridge model, one model per asset, gene or sensor, the permuted-y columns of a
    significance test.  Row r of the result is what ``ls_spa(X_train, X_test, Y_train[:, r], Y_test[:, r], reg,
    method='subsets')`` returns, but the rows of X are reduced once (one Gram pass per side over [X | Y]) and the 2^p
    subsets are enumerated once for every eight responses instead of once each: the elimination of a subset's
    features and the test-side products do not depend on y (include/lsspa.h, lsspa_multi_shapley).  fp64 throughout; a
    response's row is bitwise the same whatever the other columns are and wherever it stands among them.

    Returns ``MultiResponseResults``: ``attribution`` [m][p], ``theta`` [m][p] (the full-model coefficients of each
    response) and ``r_squared`` [m]; row r of ``attribution`` sums to ``r_squared[r]``.

    Shapes that do not fit raise ``SizeIncompatible``; p > 32 or p + m > 32767 ValueError naming the limit, before any
    GPU work.  As for a single y, a column of ``Y_test`` that is identically zero is a ValueError, and a Gram matrix
    that is not numerically positive definite a RuntimeWarning (it is shared, so it concerns every response); theta is
    then the solution of minimal norm.  M < p works.

    groups:  one integer label per column as ``ls_spa(method='subsets', groups=)`` takes them: k in 0 .. g-1 puts the
        column into group k, -1 into a baseline that every model includes.  The players are then the g groups, and the
        result is a ``MultiGroupResults``: row r of ``attribution`` [m][g] is what ``ls_spa(X_train, X_test,
        Y_train[:, r], Y_test[:, r], reg, method='subsets', groups=groups).attribution`` returns and sums to
        ``r_squared[r] - baseline_r_squared[r]``; ``theta`` [m][p] and ``r_squared`` [m] are the full models',
        ``baseline_r_squared`` [m] each response's R^2 of the baseline columns alone (0 without a baseline).  The
        elimination of a group subset's columns is shared by every eight responses (include/lsspa.h,
        lsspa_multi_groups_shapley).  The limits and messages are that call's -- g <= 32, p <= 64 (the p <= 32 limit
        does not apply), labels refused with ValueError -- before any GPU work."""
    X_train, X_test = np.asarray(X_train), np.asarray(X_test)
    Y_train, Y_test = np.asarray(Y_train), np.asarray(Y_test)
    if X_train.ndim != 2 or X_test.ndim != 2:
        raise ValueError("X_train and X_test must be two-dimensional")
    if Y_train.ndim == 1:
        Y_train = Y_train[:, None]
    if Y_test.ndim == 1:
        Y_test = Y_test[:, None]
    if Y_train.ndim != 2 or Y_test.ndim != 2:
        raise ValueError("Y_train and Y_test must be [rows][m] (or one-dimensional for one response)")
    if Y_train.shape[1] != Y_test.shape[1]:
        raise SizeIncompatible("Y_train and Y_test should have the same number of columns (responses).")
    validate_data(X_train, X_test, Y_train, Y_test)
    p, m = X_train.shape[1], Y_train.shape[1]
    labels = None
    if groups is not None:
        if p > GROUPS_MAX_P:
            raise ValueError(f"grouped attribution takes at most p = {GROUPS_MAX_P} columns, the baseline's included "
                             f"(this problem has p = {p})")
        labels, _ = group_labels(groups, p)
    elif p > SUBSETS_MAX_P:
        raise ValueError(f"ls_spa_multi enumerates all 2^p feature subsets and takes at most p = {SUBSETS_MAX_P} "
                         f"features (this problem has p = {p}); use a sampling method per response")
    if p < 1 or m < 1 or X_test.shape[0] < 1:
        raise ValueError(f"ls_spa_multi needs p >= 1 features, m >= 1 responses and M >= 1 test rows "
                         f"(p = {p}, m = {m}, M = {X_test.shape[0]})")
    if p + m > MULTI_MAX_COLS:
        raise ValueError(f"ls_spa_multi takes p + m <= {MULTI_MAX_COLS} columns of [X | Y] (p = {p}, m = {m}); "
                         "cut the responses into several calls")
    undo = []
    with _engine_call(_engine, device, undo=undo) as engine:
        undo.append((engine.multi_free, True))
        engine.multi_load(X_train, X_test, Y_train, Y_test, reg)
        phi, bits = engine.multi_shapley() if labels is None else engine.multi_groups_shapley(labels)
        gram = engine.multi_gram()
        theta, r_squared, singular = _multi_fit(*gram)
    _info_verdict((bits | int(singular)) & 1, stacklevel=2)
    if labels is None:
        return MultiResponseResults(attribution=phi, theta=theta, r_squared=r_squared)
    return MultiGroupResults(attribution=phi, theta=theta, r_squared=r_squared,
                             baseline_r_squared=_multi_baseline_r_squared(*gram, labels))


def _permutation_options(n_perm, permute):
    """(n_perm, sides): the number of replicates as an int and the sides to permute as lsspa_perm_run's bits (1 train,
    2 test); ValueError names what is wrong.  Needs no engine."""
    if isinstance(n_perm, bool) or int(n_perm) != n_perm or n_perm < 1:
        raise ValueError(f"n_perm must be an integer >= 1 (got {n_perm!r})")
    if isinstance(permute, str):
        permute = (permute,)
    sides = tuple(permute)
    if not sides or any(s not in ("train", "test") for s in sides) or len(set(sides)) != len(sides):
        raise ValueError(f"permute must name 'train', 'test' or both (got {permute!r})")
    return int(n_perm), ("train" in sides) * 1 + ("test" in sides) * 2


def ls_spa_permutation_test(X_train, X_test, y_train, y_test, reg=0., n_perm=1000, seed=42, *, groups=None,
                            permute=("train", "test"), device=0, _engine=None):
    """Permutation test of the exact attribution: p-values for the Shapley shares and for R^2 (p <= 32; with
    ``groups=``, g <= 32 groups over p <= 64 columns).

    The out-of-sample share of a feature that has nothing to do with y is not zero: it scatters around zero with a
    spread that depends on N, M, p and the collinearity of X.  This call draws that null distribution.  The null is the
    GLOBAL one -- y is exchangeable with respect to the rows of X: replicate r permutes ``y_train`` by pi_r and
    ``y_test`` by an independent pi'_r, refits and re-attributes.  X^T X, X_test^T X_test and ||y_test||^2 do not change
    under a permutation, so a replicate costs one gathered X^T y[pi] per side -- on the GPU, from rows that stay there
    -- and a share of an enumeration that carries eight replicates a sweep (include/lsspa.h, lsspa_perm_run).  It is
    NOT a per-feature conditional test (no column of X is permuted, nothing is held fixed): a small p-value says the
    feature earns more than it would if y were unrelated to every column.  With a baseline that is not constant
    (columns labelled -1 other than an intercept) the baseline is part of what y is permuted against; a constant column
    is unaffected.  The permutations are a pure function of (seed, replicate, side): two calls agree bitwise, replicate
    r is the same whatever ``n_perm`` is, and a seed gives the same permutations with and without ``groups=``.

    Returns ``PermutationTestResults``: the observed ``attribution``, ``theta``, ``r_squared`` (computed as one more
    response, the identity permutation, by the kernel that computes the null rows, so that ``>=`` compares like with
    like; it agrees with ``ls_spa(method='subsets')`` to rounding), ``null_attribution`` [n_perm][d],
    ``null_r_squared``, the one-sided ``p_values`` = (1 + #{null >= observed}) / (1 + n_valid), ``p_values_adjusted``
    (single-step max-T over the d players: family-wise error control), ``r_squared_p_value``, ``n_perm`` and
    ``n_failed``.  fp64 throughout; M < p works.

    permute:  ('train', 'test') (default) or one of them; the side not named keeps its observed X^T y in every replicate.
    groups:   one label per column as ``ls_spa(method='subsets', groups=)`` takes them (-1: a baseline that every model
        includes, 0 .. g-1: the groups).  The players are then the groups; ``baseline_r_squared`` and
        ``null_baseline_r_squared`` hold the R^2 of the baseline alone, and a null row sums to its R^2 minus that.
    Shapes that do not fit raise ``SizeIncompatible``; p > 32 without groups, p > 64 or g > 32 with them, bad labels,
    n_perm < 1, a bad ``permute`` or a ``y_test`` that is identically zero ValueError, all before any GPU work.  A Gram
    matrix that is not numerically positive definite is a RuntimeWarning as for ``ls_spa_multi`` (it is shared by every
    replicate; theta is then the solution of minimal norm); ``n_failed`` counts the replicates that are not finite."""
    data = _coerce_data(X_train, X_test, y_train, y_test)
    n, p = data[0].shape
    m = data[1].shape[0]
    labels = None
    if groups is not None:
        if p > GROUPS_MAX_P:
            raise ValueError(f"ls_spa_permutation_test(groups=) takes at most p = {GROUPS_MAX_P} columns, the baseline's "
                             f"included (this problem has p = {p})")
        labels, _ = group_labels(groups, p)
    elif p > SUBSETS_MAX_P:
        raise ValueError(f"ls_spa_permutation_test re-runs the enumeration of all 2^p feature subsets and takes at most "
                         f"p = {SUBSETS_MAX_P} features (this problem has p = {p}); group the columns (groups=) to "
                         "attribute to at most 32 players")
    n_perm, sides = _permutation_options(n_perm, permute)
    if p < 1 or n < 1 or m < 1 or n >= 2 ** 31 or m >= 2 ** 31:
        raise ValueError(f"ls_spa_permutation_test needs p >= 1 features and 1 <= N, M < 2^31 rows (p = {p}, N = {n}, "
                         f"M = {m})")
    if not np.any(data[3]):
        raise ValueError("y_test is identically zero: the out-of-sample R^2 is not defined")
    undo = []
    with _engine_call(_engine, device, undo=undo) as engine:
        undo.append((engine.perm_free, True))
        engine.perm_load(*data, reg)
        phi, bits = engine.perm_observed(labels)
        null, gperm, hperm, bits_null = engine.perm_run(n_perm, seed, labels, sides=sides)
        G, g, H, h, yy = engine.perm_gram()
    theta, r_squared, singular = _multi_fit(G, g[None, :], H, h[None, :], np.array([yy]))
    yyv = np.full(n_perm, yy)
    _, null_r2, _ = _multi_fit(G, gperm, H, hperm, yyv)
    _info_verdict((bits | bits_null | int(singular)) & 1, stacklevel=2)
    base = null_base = None
    if labels is not None:
        base = _multi_baseline_r_squared(G, g[None, :], H, h[None, :], np.array([yy]), labels)[0]
        null_base = _multi_baseline_r_squared(G, gperm, H, hperm, yyv, labels)
    return PermutationTestResults.from_null(phi, theta[0], r_squared[0], null, null_r2, base, null_base)


BOOT_ONES_BYTES = 64 << 20     # ls_spa_bootstrap: host bytes of the unit weights of a side that is not resampled


def _bootstrap_options(n_boot, confidence, weights, resample, n, m):
    """(w_train, w_test, sides): the caller's weights as (n_boot, rows) float64 arrays or None, and which sides are
    resampled; ValueError names what is wrong.  Needs no engine."""
    if int(n_boot) != n_boot or n_boot < 2:
        raise ValueError(f"n_boot must be an integer >= 2 (got {n_boot!r})")
    if not 0.0 < float(confidence) < 1.0:
        raise ValueError(f"confidence must lie strictly between 0 and 1 (got {confidence!r})")
    if isinstance(resample, str):
        resample = (resample,)
    sides = tuple(resample)
    if not sides or any(s not in ("train", "test") for s in sides) or len(set(sides)) != len(sides):
        raise ValueError(f"resample must name 'train', 'test' or both (got {resample!r})")
    out = [None, None]
    if weights is not None:
        if len(weights) != 2:
            raise ValueError("weights must be a pair (w_train, w_test); either may be None")
        for k, (w, rows, name) in enumerate(zip(weights, (n, m), ("w_train", "w_test"))):
            if w is None:
                continue
            w = np.ascontiguousarray(w, dtype=np.float64)
            if w.shape != (n_boot, rows):
                raise ValueError(f"{name} must have shape (n_boot, rows) = ({n_boot}, {rows}), got {w.shape}")
            if not np.all(np.isfinite(w)) or np.any(w < 0):
                raise ValueError(f"{name} must be finite and >= 0")
            if np.any(w.sum(axis=1) <= 0):
                raise ValueError(f"{name}: the weights of replicate {int(np.argmax(w.sum(axis=1) <= 0))} sum to zero")
            out[k] = w
    return out[0], out[1], sides


def _bootstrap_parts(run, n_boot, seed, w_train, w_test, fixed, n, m):
    """The engine's results of a bootstrap run of n_boot replicates, as a list of one tuple per engine call.  fixed: the
    sides (0 train, 1 test) that are not resampled and have no weights of the caller's -- weight 1 on every row: the run
    is then cut so that those rows of ones stay within BOOT_ONES_BYTES on the host."""
    if not fixed:
        return [run(n_boot, seed, w_train, w_test)]
    rows = max((n, m)[k] for k in fixed)
    step = max(1, min(n_boot, BOOT_ONES_BYTES // (8 * rows)))
    parts = []
    for r0 in range(0, n_boot, step):
        nb = min(step, n_boot - r0)
        w = [None if x is None else x[r0:r0 + nb] for x in (w_train, w_test)]
        for k in fixed:
            w[k] = np.ones((nb, (n, m)[k]))
        parts.append(run(nb, seed, w[0], w[1], first=r0))
    return parts


def _bootstrap_arrays(engine, undo, data, reg, grouped, run, n_boot, seed, options, n_arrays):
    """The shared middle of the bootstrap drivers, inside their engine call: the rows onto the device (boot_free goes into
    `undo`), then `run` (an engine's boot_*_run, bound to what it takes before R) over the n_boot replicates; its n_arrays
    results, each concatenated over the engine calls.  options: _bootstrap_options' (w_train, w_test, sides)."""
    w_train, w_test, sides = options
    fixed = [k for k, (name, w) in enumerate(zip(("train", "test"), (w_train, w_test))) if name not in sides and w is None]
    engine.boot_load(*data, reg, grouped=grouped)
    undo.append((engine.boot_free, True))
    parts = _bootstrap_parts(run, n_boot, seed, w_train, w_test, fixed, len(data[0]), len(data[1]))
    return [np.concatenate([q[k] for q in parts]) for k in range(n_arrays)]


def _warn_failed_replicates(n_failed, n_boot, where):
    """A bootstrap's RuntimeWarning about its failed replicates, attributed to the caller of the public function that
    asks.  where: the array that holds their NaN and what they are left out of."""
    if n_failed:
        warnings.warn(f"{n_failed} of {n_boot} bootstrap replicates had a Gram matrix that was not numerically "
                      "positive definite (a column constant or collinear on the resampled rows); they are NaN in "
                      f"{where}", RuntimeWarning, stacklevel=3)


class _PointWarnings(warnings.catch_warnings):
    """The point estimate's warnings are this call's: recorded while the context (made with record=True) is open, and
    handed to the caller of the public function that asks by emit(), once its engine call is over."""

    def __enter__(self):
        self._caught = super().__enter__()
        warnings.simplefilter("always")

    def emit(self):
        for w in self._caught:
            warnings.warn(w.message, w.category, stacklevel=3)


def ls_spa_bootstrap(X_train, X_test, y_train, y_test, reg=0., n_boot=1000, seed=42, *, confidence=0.95, weights=None,
                     resample=("train", "test"), groups=None, device=0, _engine=None):
    """Bootstrap confidence intervals for the exact attribution (p <= 32; with ``groups=``, g <= 32 groups over p <= 64
    columns).

    ``ls_spa(method='subsets')`` is exact for the rows it was handed; this call says how far it would move had the rows
    been another draw from the same population.  The point estimate is that call's (``attribution``, ``theta``,
    ``r_squared``, by the same path).  Each of the ``n_boot`` replicates resamples the rows with replacement, refits and
    re-attributes -- on the GPU, from rows that stay there: a replicate's reduced problem is a weighted Gram with the
    bootstrap counts as weights, a block of replicates is one pass over the rows, and their enumerations share one grid
    (include/lsspa.h, lsspa_boot_run).  The counts are a pure function of (seed, replicate, side): two calls agree bitwise.

    Returns ``BootstrapResults``: ``replicates`` [n_boot][p], ``r_squared_replicates``, ``std_error``, the percentile
    interval ``lower`` / ``upper`` at ``confidence`` (numpy's default interpolation), ``r_squared_interval``,
    ``prob_greater`` [p][p] (the share of replicates with phi_i > phi_j: "is feature 3 really worth more than feature
    7?") and ``n_failed``: replicates whose Gram matrix was not numerically positive definite are NaN and left out, with
    a RuntimeWarning; more than half of them is a RuntimeError.

    weights:  (w_train, w_test), each None or an (n_boot, rows) array of finite weights >= 0 with a positive sum per
        replicate, used instead of the counts on that side: a Bayesian bootstrap (Dirichlet weights), survey weights,
        a jackknife (zero weights).
    resample: ('train', 'test') (default) or one of them; the side not named keeps weight 1 on every row.
    groups:   one label per column as ``ls_spa(groups=)`` takes them (-1: a baseline that every model includes, 0 .. g-1:
        the groups).  The players are then the groups: the point estimate is that of ``ls_spa(method='subsets',
        groups=)``, every replicate is re-attributed over the 2^g group subsets (include/lsspa.h,
        lsspa_boot_groups_run), and ``attribution``, ``replicates`` [n_boot][g], ``std_error``, ``lower``, ``upper`` and
        ``prob_greater`` [g][g] speak of groups; ``theta`` keeps length p, and ``baseline_r_squared_replicates`` holds
        the R^2 of each replicate's baseline alone (a replicate sums to its R^2 minus that).  A given seed resamples
        the same rows with and without groups.  Limits: g <= 32 and p <= 64, ValueError otherwise.
    Without groups, p > 32 raises ValueError: group the columns (``ls_spa_groups``) or use a sampling method."""
    data = _coerce_data(X_train, X_test, y_train, y_test)
    n, p = data[0].shape
    m = data[1].shape[0]
    labels = None
    if groups is not None:
        if p > GROUPS_MAX_P:
            raise ValueError(f"ls_spa_bootstrap(groups=) takes at most p = {GROUPS_MAX_P} columns, the baseline's "
                             f"included (this problem has p = {p})")
        labels, _ = group_labels(groups, p)
    elif p > SUBSETS_MAX_P:
        raise ValueError(f"ls_spa_bootstrap re-runs the enumeration of all 2^p feature subsets and takes at most p = "
                         f"{SUBSETS_MAX_P} features (this problem has p = {p}); group the columns (ls_spa_groups) to "
                         "attribute to at most 32 players, or use a sampling method")
    options = _bootstrap_options(n_boot, confidence, weights, resample, n, m)
    n_boot = int(n_boot)
    undo = []
    with _engine_call(_engine, device, undo=undo) as engine:
        if getattr(engine, "precision", "float64") != "float64":
            engine.set_precision("float64")
        theta, r_squared, info = _load_and_fit(engine, data, reg, False, None)
        phi, bits = engine.subsets_shapley() if labels is None else engine.groups_shapley(labels)
        _info_verdict((bits | info) & 1, stacklevel=3)
        if info & 1:
            theta, r_squared = _singular_fit(engine, data[1], data[3])
        grouped = labels is not None
        run = functools.partial(engine.boot_groups_run, labels) if grouped else engine.boot_run
        rep, r2, *base, binfo = _bootstrap_arrays(engine, undo, data, reg, grouped, run, n_boot, seed, options, 3 + grouped)
    failed = (binfo & 1).astype(bool) | ~np.isfinite(rep).all(axis=1) | ~np.isfinite(r2)
    for b in base:
        failed |= ~np.isfinite(b)
    res = BootstrapResults.from_replicates(phi, theta, r_squared, rep, r2, failed, confidence, *base)
    _warn_failed_replicates(res.n_failed, n_boot, "`replicates` and left out of the intervals")
    return res


BOOT_LIFT_MAX_P = 127      # include/lsspa.h, LSSPA_BOOT_LIFT_MAX_P


def ls_spa_bootstrap_sampled(X_train, X_test, y_train, y_test, reg=0., n_boot=200, n_samples=2 ** 10, seed=42, perms=None,
                             *, groups=None, method="random", antithetical=True, boot_seed=42, confidence=0.95,
                             weights=None, resample=("train", "test"), device=0, _engine=None):
    """Bootstrap confidence intervals for the SAMPLED attribution (1 <= p <= 127; with ``groups=`` any 1 <= g <= p
    groups of those columns): what ``ls_spa_bootstrap`` gives for the exact enumerations, beyond their limits.

    ``ls_spa`` returns an attribution and a Monte-Carlo standard error that says how well the orderings were sampled;
    this call says how far the attribution would move had the rows been another draw from the same population.  Each of
    the ``n_boot`` replicates resamples the rows with replacement -- on the GPU, from rows that stay there, by
    ``ls_spa_bootstrap``'s counts rule: a given ``boot_seed`` resamples exactly the rows that call's ``seed`` resamples
    -- and is re-attributed over ONE set of ``n_samples`` orderings that is drawn ahead and shared by all replicates
    and the point estimate (common random numbers): the Monte-Carlo error of the orderings moves all replicates
    together instead of widening their spread.  One launch runs a cut of the orderings through many replicates'
    problems at once (include/lsspa.h, lsspa_boot_lift_run).  fp64 throughout; two calls agree bitwise.

    n_samples, seed, method, perms, antithetical:  the ordering source, as in ``ls_spa_multi_sampled`` (``seed`` seeds it;
        a caller's ``perms`` are taken as they are, all of them).  The number of samples is fixed -- there is no
        ``tolerance`` -- so that every replicate sees the same ones.
    boot_seed, weights, resample, confidence:  ``ls_spa_bootstrap``'s ``seed``, ``weights``, ``resample`` and
        ``confidence``.
    groups:  one integer label per column as ``ls_spa_groups`` takes them (-1: the baseline, 0 .. g-1).  The players are
        then the groups, the sources run in dimension g, ``perms`` are group orderings, and the result is a
        ``SampledBootstrapGroupResults``.

    Returns ``SampledBootstrapResults``: ``attribution`` and ``attribution_errors`` [d] (the original rows, weight 1 on
    every row, through the same path as one more problem), ``replicates`` and ``replicate_errors`` [n_boot][d],
    ``std_error``, ``lower``, ``upper``, ``prob_greater`` [d][d], ``r_squared``, ``r_squared_replicates``,
    ``r_squared_interval``, ``theta``, ``n_samples`` and ``n_failed``: a replicate whose G or H fails the pivot test in any
    ordering is NaN and left out, with a RuntimeWarning; more than half of them is a RuntimeError.

    Shapes that do not fit, p > 127, fewer rows than columns on either side, ``n_boot`` < 2, ``n_samples`` < 2, ``perms``
    together with ``method``, bad labels, ``weights``, ``resample`` or ``confidence`` and a ``y_test`` that is identically
    zero are refused before any GPU work.  Several ranks, checkpoints, fp32, the device error estimator and the history
    are not part of this function."""
    sa, se = np.shape(X_train), np.shape(X_test)
    if len(sa) == 2 and len(se) == 2 and sa[1] == se[1]:      # the limits by their names, ahead of the shape rules
        if sa[1] > BOOT_LIFT_MAX_P:
            raise ValueError(f"ls_spa_bootstrap_sampled takes at most p = {BOOT_LIFT_MAX_P} features (this problem has "
                             f"p = {sa[1]})")
        if 1 <= sa[1] and (sa[0] < sa[1] or se[0] < sa[1]) and np.shape(y_train) == sa[:1] and np.shape(y_test) == se[:1]:
            raise ValueError(f"ls_spa_bootstrap_sampled needs at least p = {sa[1]} rows on both sides (N = {sa[0]}, M = "
                             f"{se[0]}): a resampled Gram matrix must have a Cholesky factor")
    data = _coerce_data(X_train, X_test, y_train, y_test)
    n, p = data[0].shape
    m = data[1].shape[0]
    if p < 1:
        raise ValueError("ls_spa_bootstrap_sampled needs p >= 1 features")
    if int(n_samples) != n_samples or n_samples < 2:
        raise ValueError(f"n_samples must be an integer >= 2 (got {n_samples!r})")
    options = _bootstrap_options(n_boot, confidence, weights, resample, n, m)
    n_boot, n_samples = int(n_boot), int(n_samples)
    if not np.any(data[3]):
        raise ValueError("y_test is identically zero: R^2 is not defined")
    # (n_samples >= 2 and the batch size are this function's own: the helper's refusal of either cannot fire)
    labels, d, source, _, antithetical, max_samples, _ = _sampled_arguments(
        p, groups, perms, method, n_samples, 2 ** 8, seed, antithetical)
    w_train, w_test, sides = options
    fixed = [k for k, (name, w) in enumerate(zip(("train", "test"), (w_train, w_test))) if name not in sides and w is None]
    undo = [(lambda: _close_source(source), True)]
    with _engine_call(_engine, device, undo=undo) as engine:
        rows = []                      # the one set of orderings, drawn ahead
        while sum(len(r) for r in rows) < max_samples:
            got = source.take(min(2 ** 10, max_samples - sum(len(r) for r in rows)))
            if len(got) == 0:
                break
            rows.append(np.array(got, dtype=np.int32))
        if sum(len(r) for r in rows) < 2:
            raise ValueError("fewer than two orderings to sample: perms needs at least two rows")
        rows = np.concatenate(rows)
        undo.append((engine.boot_lift_free, True))
        engine.boot_lift_load(*data, reg)
        if labels is not None:
            engine.boot_lift_set_players(labels)      # (boot_lift_free drops the map with everything else)
        engine.boot_lift_set_orderings(rows, antithetical)
        phi, phi_m2, r_squared, base, info = engine.boot_lift_point()
        G, g = engine.boot_lift_problem(-1)[:2]
        parts = _bootstrap_parts(engine.boot_lift_run, n_boot, boot_seed, w_train, w_test, fixed, n, m)
        rep, rep_m2, r2, r2_base, binfo = (np.concatenate([q[k] for q in parts]) for k in range(5))
    ns = len(rows)
    _info_verdict(info & 1, stacklevel=2)
    failed = (binfo & 1).astype(bool) | ~np.isfinite(rep).all(axis=1) | ~np.isfinite(r2) | ~np.isfinite(r2_base)
    # every sample's lifts telescope from the baseline's value to the full model's, so a replicate's mean does (the
    # bound of LSSPA_INFO_SUM for well-conditioned data)
    gap = np.abs(rep.sum(axis=1) - (r2 - r2_base)) > 1e-9 * np.maximum(1.0, np.abs(r2))
    point_gap = abs(phi.sum() - (r_squared - base)) > 1e-9 * max(1.0, abs(r_squared))
    if (gap & ~failed).any() or (point_gap and not info & 1):
        _info_verdict(8, stacklevel=2)
    core = BootstrapResults.from_replicates(phi, _subset_fit(G, g, np.arange(p)), r_squared, rep, r2, failed, confidence,
                                            r2_base)
    errors = _multi_standard_errors(ns, rep_m2)
    errors[failed] = np.nan
    common = dict(attribution=phi, attribution_errors=_multi_standard_errors(ns, phi_m2), theta=core.theta,
                  r_squared=float(r_squared), replicates=core.replicates, replicate_errors=errors,
                  r_squared_replicates=core.r_squared_replicates, std_error=core.std_error, lower=core.lower,
                  upper=core.upper, r_squared_interval=core.r_squared_interval, prob_greater=core.prob_greater,
                  n_samples=ns, n_failed=core.n_failed, confidence=core.confidence)
    _warn_failed_replicates(core.n_failed, n_boot, "`replicates` and left out of the intervals")
    if labels is not None:
        return SampledBootstrapGroupResults(baseline_r_squared=float(base),
                                            baseline_r_squared_replicates=core.baseline_r_squared_replicates, **common)
    return SampledBootstrapResults(**common)


def ls_spa_interactions_bootstrap(X_train, X_test, y_train, y_test, reg=0., n_boot=1000, seed=42, *, confidence=0.95,
                                  weights=None, resample=("train", "test"), groups=None, device=0, _engine=None):
    """Bootstrap confidence intervals for the exact pairwise interaction values (p <= 32; with ``groups=``, g <= 32 groups
    over p <= 64 columns).

    ``ls_spa_interactions`` is exact for the rows it was handed, and its entries are second differences of v(K): far
    noisier under resampling than the attribution.  This call says whether "features 3 and 7 share -0.04 of the R^2"
    keeps its sign on another draw of the rows.  The point estimate is that call's (``interactions``, ``attribution``,
    ``theta``, ``r_squared``, by the same path).  Each of the ``n_boot`` replicates is one of ``ls_spa_bootstrap``'s -- a
    given seed resamples the same rows, and a replicate's attribution is bitwise that call's -- re-attributed by the
    interaction enumeration on the GPU, the replicates of a launch sharing one grid (include/lsspa.h,
    lsspa_boot_interactions_run).  Two calls agree bitwise.

    Returns ``InteractionBootstrapResults``: ``replicates`` [n_boot][d][d] in SHAP's convention like ``interactions``,
    ``attribution_replicates``, ``r_squared_replicates``, and per entry of the matrix ``std_error``, the percentile
    interval ``lower`` / ``upper`` at ``confidence`` and ``prob_positive``, the share of replicates with Phi_ij > 0;
    ``n_failed``: replicates whose Gram matrix was not numerically positive definite are NaN and left out, with a
    RuntimeWarning; more than half of them is a RuntimeError.

    weights, resample: as ``ls_spa_bootstrap`` takes them.
    groups:   one label per column as ``ls_spa_interactions(groups=)`` takes them; the players are then the g groups
        (include/lsspa.h, lsspa_boot_groups_interactions_run), every matrix is g x g and sums to the replicate's R^2
        minus ``baseline_r_squared_replicates``; ``theta`` keeps length p.  Limits: g <= 32 and p <= 64.
    Fewer than two players, p > 32 without groups, p > 64 or g > 32 with groups raise ValueError."""
    data = _coerce_data(X_train, X_test, y_train, y_test)
    n, p = data[0].shape
    m = data[1].shape[0]
    labels, d = None, p
    if groups is not None:
        if p > GROUPS_MAX_P:
            raise ValueError(f"ls_spa_interactions_bootstrap(groups=) takes at most p = {GROUPS_MAX_P} columns, the "
                             f"baseline's included (this problem has p = {p})")
        labels, d = group_labels(groups, p)
    elif p > SUBSETS_MAX_P:
        raise ValueError(f"ls_spa_interactions_bootstrap re-runs the enumeration of all 2^p feature subsets and takes at "
                         f"most p = {SUBSETS_MAX_P} features (this problem has p = {p}); group the columns (groups=) to "
                         "at most 32 players")
    if d < 2:
        raise ValueError(f"an interaction needs two players (this problem has {d})")
    options = _bootstrap_options(n_boot, confidence, weights, resample, n, m)
    n_boot = int(n_boot)
    undo = []
    with _engine_call(_engine, device, undo=undo) as engine:
        if getattr(engine, "precision", "float64") != "float64":
            engine.set_precision("float64")
        theta, r_squared, info = _load_and_fit(engine, data, reg, False, None)
        phi, raw, bits = engine.subsets_interactions() if labels is None else engine.groups_interactions(labels)
        _info_verdict((bits | info) & 1, stacklevel=3)
        if info & 1:
            theta, r_squared = _singular_fit(engine, data[1], data[3])
        grouped = labels is not None
        run = functools.partial(engine.boot_groups_interactions_run, labels) if grouped else engine.boot_interactions_run
        att, index, r2, *base, binfo = _bootstrap_arrays(engine, undo, data, reg, grouped, run, n_boot, seed, options,
                                                         4 + grouped)
    failed = (binfo & 1).astype(bool) | ~np.isfinite(att).all(axis=1) | ~np.isfinite(index).all(axis=(1, 2)) | ~np.isfinite(r2)
    for b in base:
        failed |= ~np.isfinite(b)
    rep = np.stack([_shap_matrix(a, i) for a, i in zip(att, index)])
    res = InteractionBootstrapResults.from_replicates(_shap_matrix(phi, raw), phi, theta, r_squared, rep, att, r2, failed,
                                                      confidence, *base)
    _warn_failed_replicates(res.n_failed, n_boot, "`replicates` and left out of the intervals")
    return res


def ls_spa_best_subsets_bootstrap(X_train, X_test, y_train, y_test, reg=0., n_boot=1000, seed=42, *, include=None,
                                  weights=None, resample=("train", "test"), groups=None, device=0, _engine=None):
    """Bootstrap of the best-subset selection (p <= 32): how stable is the chosen model?

    ``ls_spa_best_subsets`` says "keep features 2, 5, 11" for the rows it was handed, and best-subset selection is
    unstable: on another draw of the rows another set may win.  The point estimate is that call's (``sizes``,
    ``subsets``, ``r_squared``, ``best_size``, ``best_subset``, ``full_r_squared``, by the same path).  Each of the
    ``n_boot`` replicates is one of ``ls_spa_bootstrap``'s -- a given seed resamples the same rows -- and is searched over
    all 2^p subsets on the GPU from rows that stay there, the replicates of a launch sharing one grid
    (include/lsspa.h, lsspa_boot_best_run): per size the largest out-of-sample R^2 and its subset, the smaller mask on
    equal values.  Two calls agree bitwise.

    Returns ``BestSubsetsBootstrapResults``: the point estimate's fields, ``subset_replicates`` [n_boot][n][p] bool,
    ``r_squared_replicates`` [n_boot][n], ``best_size_replicates`` [n_boot] (the rule of ``best_size``),
    ``full_r_squared_replicates``, and over the valid replicates ``inclusion_frequency`` [n][p] (the share whose size-k
    winner holds feature j), ``best_inclusion_frequency`` [p] (the same for each replicate's overall best model),
    ``best_size_frequency`` [n], ``reselected`` [n] (the share whose size-k winner is the point estimate's) and
    ``n_failed``: replicates whose Gram matrix was not numerically positive definite are NaN / False and left out, with a
    RuntimeWarning; more than half of them is a RuntimeError.

    include:  as ``ls_spa_best_subsets`` takes it; the n sizes then start at len(include).
    weights, resample: as ``ls_spa_bootstrap`` takes them.
    groups=:  not taken here, a ValueError says so: the bootstrap of ``ls_spa_best_subsets(groups=)`` is a call of its
        own, ``ls_spa_best_group_subsets_bootstrap``.
    p > 32, a bad ``include``, ``n_boot``, ``weights`` or ``resample`` and a ``y_test`` that is identically zero are refused
    before any GPU work."""
    if groups is not None:
        raise ValueError("ls_spa_best_subsets_bootstrap does not take groups= yet: the bootstrap of the selection over "
                         "groups of columns is not built (ls_spa_best_subsets(groups=) gives the point estimate)")
    data = _coerce_data(X_train, X_test, y_train, y_test)
    n, p = data[0].shape
    m = data[1].shape[0]
    if p > SUBSETS_MAX_P:
        raise ValueError(f"ls_spa_best_subsets_bootstrap re-runs the enumeration of all 2^p feature subsets and takes at "
                         f"most p = {SUBSETS_MAX_P} features (this problem has p = {p})")
    if p < 1 or m < 1:
        raise ValueError(f"ls_spa_best_subsets_bootstrap needs p >= 1 features and M >= 1 test rows (p = {p}, M = {m})")
    mask, inc = include_mask(include, p)
    if not np.any(data[3]):
        raise ValueError("y_test is identically zero: the out-of-sample R^2 is not defined")
    options = _bootstrap_options(n_boot, 0.95, weights, resample, n, m)
    n_boot = int(n_boot)
    undo, point_warnings = [], _PointWarnings(record=True)
    with _engine_call(_engine, device, undo=undo) as engine:
        with point_warnings:
            point = ls_spa_best_subsets(*data, reg=reg, include=include, _engine=engine)
        run = functools.partial(engine.boot_best_run, include=mask)
        v, masks, found, r2, binfo = _bootstrap_arrays(engine, undo, data, reg, False, run, n_boot, seed, options, 5)
    point_warnings.emit()
    failed = (binfo & 1).astype(bool) | ~np.isfinite(r2)
    k0 = len(inc)
    res = BestSubsetsBootstrapResults.from_replicates(point, v[:, k0:], masks[:, k0:], found[:, k0:], r2, failed)
    _warn_failed_replicates(res.n_failed, n_boot, "`r_squared_replicates` and left out of the frequencies")
    return res


def ls_spa_best_group_subsets_bootstrap(X_train, X_test, y_train, y_test, groups, reg=0., n_boot=1000, seed=42, *,
                                        weights=None, resample=("train", "test"), device=0, _engine=None):
    """Bootstrap of the best-subset selection over groups of columns (g <= 32 groups over p <= 64 columns): how stable
    is the chosen set of groups?

    ``ls_spa_best_subsets(groups=)`` says "keep the factor, drop the spline" for the rows it was handed; on another draw
    of the rows another set of groups may win.  The point estimate is that call's (``sizes`` 0 .. g, ``group_subsets``,
    ``subsets``, ``r_squared``, ``best_size``, ``best_group_subset``, ``best_subset``, ``full_r_squared``,
    ``baseline_r_squared``, by the same path, its warnings this call's).  Each of the ``n_boot`` replicates is one of
    ``ls_spa_bootstrap(groups=)``'s -- a given seed resamples the same rows -- and is searched over all 2^g sets of
    groups on the GPU from rows that stay there, the replicates of a launch sharing one grid (include/lsspa.h,
    lsspa_boot_groups_best_run): per number of groups the largest out-of-sample R^2 and its set, the smaller mask (bit
    k = group k) on equal values.  Two calls agree bitwise.

    groups:   one label per column as ``ls_spa_best_subsets(groups=)`` takes them: k in 0 .. g-1 puts the column into
        group k, -1 into the baseline that every model contains.  There is no ``include=``: the baseline is the
        include set.  The p <= 32 limit of ``ls_spa_best_subsets_bootstrap`` does not apply.
    weights, resample: as ``ls_spa_bootstrap`` takes them.

    Returns ``BestGroupSubsetsBootstrapResults``: the point estimate's fields, ``group_subset_replicates``
    [n_boot][g + 1][g] bool, ``r_squared_replicates`` [n_boot][g + 1], ``best_size_replicates`` [n_boot] (the rule of
    ``best_size``), ``full_r_squared_replicates``, ``baseline_r_squared_replicates`` (column 0 of
    ``r_squared_replicates`` wherever the baseline alone is a candidate), and over the valid replicates
    ``inclusion_frequency`` [g + 1][g] (the share whose size-k winner holds group j), ``best_inclusion_frequency`` [g]
    (the same for each replicate's overall best model), ``best_size_frequency`` [g + 1], ``reselected`` [g + 1] (the
    share whose size-k winner is the point estimate's) and ``n_failed``: replicates whose Gram matrix was not
    numerically positive definite are NaN / False and left out, with a RuntimeWarning; more than half of them is a
    RuntimeError.

    Bad labels, p > 64, g > 32, a bad ``n_boot``, ``weights`` or ``resample``, shapes that do not fit and a ``y_test``
    that is identically zero are refused before any GPU work."""
    data = _coerce_data(X_train, X_test, y_train, y_test)
    n, p = data[0].shape
    m = data[1].shape[0]
    if p > GROUPS_MAX_P:
        raise ValueError(f"grouped attribution takes at most p = {GROUPS_MAX_P} columns, the baseline's included "
                         f"(this problem has p = {p})")
    labels, g = group_labels(groups, p)
    if m < 1:
        raise ValueError(f"ls_spa_best_group_subsets_bootstrap needs M >= 1 test rows (M = {m})")
    if not np.any(data[3]):
        raise ValueError("y_test is identically zero: the out-of-sample R^2 is not defined")
    options = _bootstrap_options(n_boot, 0.95, weights, resample, n, m)
    n_boot = int(n_boot)
    undo, point_warnings = [], _PointWarnings(record=True)
    with _engine_call(_engine, device, undo=undo) as engine:
        with point_warnings:
            point = ls_spa_best_subsets(*data, reg=reg, groups=labels, _engine=engine)
        run = functools.partial(engine.boot_groups_best_run, labels)
        u, masks, found, r2, base, binfo = _bootstrap_arrays(engine, undo, data, reg, True, run, n_boot, seed, options, 6)
    point_warnings.emit()
    failed = (binfo & 1).astype(bool) | ~np.isfinite(r2) | ~np.isfinite(base)
    res = BestGroupSubsetsBootstrapResults.from_replicates(point, u, masks, found, r2, base, failed)
    _warn_failed_replicates(res.n_failed, n_boot, "`r_squared_replicates` and left out of the frequencies")
    return res


GROUPS_AUTO_MAX_G = 20     # ls_spa_groups(method='auto'): the enumeration up to here (26 ms at g = 20, README.md)


def ls_spa_groups(X_train, X_test, y_train, y_test, groups, reg=0., max_samples=2 ** 13, batch_size=2 ** 8,
                  tolerance=1e-2, seed=42, perms=None, antithetical=True, return_attribution_history=False, *,
                  method="auto", num_batches=None, return_history=None, device=0, error_estimator=None,
                  precision="float64", lookahead=None, lanes="auto", row_sharded=False, comm=None, checkpoint=None,
                  _engine=None, _timings=None, _defer=None):
    """Shapley attribution of the out-of-sample R^2 over GROUPS of columns, for any number of groups and columns.

    The players of the game are the groups that ``groups`` names: one integer label per column, k in 0 .. g-1 puts the
    column into group k (every group needs a column), -1 into the baseline -- the columns of every model (an intercept,
    controls), which get no attribution.  u(S) is the R^2 of the baseline plus the columns of the groups in S, and the
    result's ``attribution`` (length g) are its Shapley values: they sum to ``r_squared`` minus the R^2 of the baseline
    alone and are not per-column attributions summed over a group.  ``theta`` (length p) and ``r_squared`` are those of
    the full fit.  Limits: 1 <= g <= p and the engine's p <= 32767.

    The Shapley value of a group is the mean over orderings of the GROUPS of the summed lifts of its columns, when every
    group ordering is expanded to a column ordering with the baseline first and each group's columns contiguous.  So a
    sample is an ordinary ordering through the engine's kernels, folded on the device from p lifts to g, and the sampling
    loop of ``ls_spa`` -- statistics, error estimate, stop rule, history -- runs in dimension g.

    Everything not named here is as in ``ls_spa``, with g in place of p wherever the dimension of a sample decides
    (the error estimate needs g >= 9, ``attribution_errors`` has length g, ``attribution_history`` is n x g); the sizes
    of the automatic look-ahead groups stay keyed on p, the cost of an ordering.

    method:  'auto' (default): 'subsets' when g <= 20 and p <= 64 (exact, and cheaper than any sampling run), else
        'argsort'.  'subsets': the exact enumeration, ``ls_spa(method='subsets', groups=groups)`` unchanged (g <= 32,
        p <= 64, the same errors).  'random', 'argsort', 'permutohedron': orderings of the g groups from the sources
        ``ls_spa`` uses for columns.  'exact': all g! group orderings through the sampling path (g up to 8 or 9).
        None: the reference's rule with g for p (all orderings below g = 9, else 'random').
    perms:  an iterable of group orderings, each a permutation of 0 .. g-1 (method must be left at 'auto' or None).
    antithetical:  a sample is a group ordering and its reverse -- the baseline first, then the groups in reversed
        order -- and its lift vector the mean of the two.
    error_estimator, precision, lookahead, lanes:  as in ``ls_spa``, same defaults per method.
    comm, checkpoint, row_sharded:  not supported here (several ranks and resuming are out of this function's scope):
        anything but None / False raises a ValueError that names the option."""
    if comm is not None:
        raise ValueError("ls_spa_groups does not take comm= (several ranks): grouped sampling runs on one GPU")
    if checkpoint is not None:
        raise ValueError("ls_spa_groups does not take checkpoint=: grouped sampling cannot be resumed")
    if row_sharded:
        raise ValueError("ls_spa_groups does not take row_sharded=: it needs comm=, which is not supported here")
    X_train, X_test, y_train, y_test = _coerce_data(X_train, X_test, y_train, y_test)
    p = X_train.shape[1]
    if method == "auto":
        if perms is not None:
            method = None
        else:
            _, g_seen = group_labels(groups, p, max_groups=None)
            method = "subsets" if (g_seen <= GROUPS_AUTO_MAX_G and p <= GROUPS_MAX_P) else "argsort"
    if method == "subsets":
        return ls_spa(X_train, X_test, y_train, y_test, reg, perms=perms, method="subsets", groups=groups,
                      return_attribution_history=return_attribution_history, return_history=return_history,
                      device=device, _engine=_engine)
    if method is not None and method not in S.METHODS:
        raise ValueError(f"method must be one of {('auto',) + tuple(S.METHODS) + ('subsets',)} or None")
    labels, g = group_labels(groups, p, max_groups=None)
    return ls_spa(X_train, X_test, y_train, y_test, reg, max_samples, batch_size, tolerance, seed, perms, antithetical,
                  return_attribution_history, method=method, num_batches=num_batches, return_history=return_history,
                  device=device, error_estimator=error_estimator, precision=precision, lookahead=lookahead, lanes=lanes,
                  _engine=_engine, _timings=_timings, _defer=_defer, _players=(labels, g))


PAIRS_MAX_D = 4096     # include/lsspa.h, LSSPA_PAIRS_MAX_D


def pair_standard_errors(counts, m2):
    """Standard errors of the SHAP-convention interaction entries Phi_ab = I_ab / 2 from a pair's count n and sum of
    squared deviations M2: sqrt(M2 / (n (n - 1))) / 2; ``inf`` where n < 2, 0 on the diagonal."""
    counts = np.asarray(counts, dtype=np.float64)
    err = np.full(counts.shape, np.inf)
    seen = counts >= 2
    err[seen] = 0.5 * np.sqrt(np.maximum(np.asarray(m2)[seen], 0.0) / (counts[seen] * (counts[seen] - 1.0)))
    np.fill_diagonal(err, 0.0)
    return err


def ls_spa_interactions_sampled(X_train, X_test, y_train, y_test, reg=0., max_samples=2 ** 13, batch_size=2 ** 8,
                                tolerance=None, seed=42, perms=None, *, groups=None, method="random", device=0,
                                precision="float64", _engine=None):
    """Sampled pairwise Shapley interaction values of the out-of-sample R^2, for any number of players: the p features,
    or with ``groups=`` the g groups of columns (2 <= d <= 4096 players; ``ls_spa_interactions`` is exact and stops at 32).

    For a uniformly random ordering of the d players in which a and b are neighbours, the players in front of them are
    a set S drawn with exactly the weight of the interaction index, so I_ab = E[v(S+a+b) - v(S+a) - v(S+b) + v(S)] over
    such orderings.  A sample is one ordering pi and its two neighbour-swapped forms -- three ordinary orderings through
    the engine's kernels -- and gives that second difference for all d - 1 neighbouring pairs of pi at once
    (include/lsspa.h, lsspa_pairs_batch); per pair the engine keeps count, mean and sum of squared deviations on the GPU,
    in a fixed order (two runs agree bitwise).  A pair is hit by a fraction 2 / d of the samples.

    Returns ``SampledInteractionResults``: ``interactions`` is d x d in SHAP's convention -- half the estimated index off
    the diagonal, attribution[a] minus the rest of row a on it -- so row a sums to ``attribution[a]`` and the whole matrix
    to ``r_squared`` (minus the R^2 of the baseline with one).  ``attribution`` is the mean of all 3 n lift vectors (each
    of a sample's three orderings is itself uniformly random), ``theta`` and ``r_squared`` are those of the full fit.
    ``interaction_errors`` holds the standard errors of the off-diagonal entries, sqrt(M2 / (n (n - 1))) / 2 with n the
    pair's count; ``counts`` those counts; a pair no sample hit has interaction 0, error ``inf`` and count 0.  The
    standard errors assume independent samples: they are only indicative for the QMC sources ('argsort',
    'permutohedron'), whose orderings are not independent, and for a caller's ``perms``.

    max_samples, batch_size:  samples are drawn in batches of ``batch_size`` until ``max_samples`` (every sample costs
        three orderings).
    tolerance:  None (default): run to ``max_samples``.  Otherwise sampling stops after the first batch at which every
        pair has count >= 2 and the largest standard error is <= tolerance.
    method:  'random' (default), 'argsort', 'permutohedron', or 'exact' (all d! orderings, d up to 8 or 9): the ordering
        sources of ``ls_spa``, in dimension d.
    perms:  an iterable of orderings of the d players instead (leave ``method`` at its default).
    groups:  one integer label per column as for ``ls_spa_groups`` (-1: baseline, 0 .. g-1: group); the players are the
        groups, ``theta`` keeps length p.
    precision:  as in ``ls_spa`` ('float32': the per-ordering factorisation work in fp32).
    d < 2 or d > 4096 raises ValueError before any GPU work.  Several ranks and resuming are not part of this function."""
    data = _coerce_data(X_train, X_test, y_train, y_test)
    p = data[0].shape[1]
    labels, d = (None, p) if groups is None else group_labels(groups, p, max_groups=None)
    if d < 2 or d > PAIRS_MAX_D:
        raise ValueError(f"sampled pairwise interactions take between 2 and {PAIRS_MAX_D} players (this problem has "
                         f"{d} {'features' if groups is None else 'groups'})")
    if perms is not None:
        if method != "random":
            raise ValueError("pass either perms= or method=, not both")
        method = None
    elif method not in S.METHODS:
        raise ValueError(f"method must be one of {tuple(S.METHODS)}")
    if int(batch_size) < 1 or int(max_samples) < 1:
        raise ValueError("batch_size and max_samples must be positive")
    _, source, batch_size, _, max_samples, never_stop = prepare_sampling(
        d, max_samples=int(max_samples), batch_size=int(batch_size), seed=seed, perms=perms, antithetical=False,
        method=method)
    if never_stop:
        tolerance = None
    undo = [(lambda: _close_source(source), True)]
    off = ~np.eye(d, dtype=bool)
    with _engine_call(_engine, device, undo=undo) as engine:
        if precision != "float64" or getattr(engine, "precision", "float64") != "float64":
            engine.set_precision(precision)
        if hasattr(engine, "set_lanes") and getattr(engine, "lanes", 1) != 1:
            engine.set_lanes(1)
        theta, r_squared, info = _load_and_fit(engine, data, reg, False, None)
        if labels is not None:
            engine.set_players(labels)      # after the full fit: that one is about the columns
        engine.pairs_enable(True)
        undo.append((lambda: engine.pairs_enable(False), False))      # the tables go back (134 MB each at d = 4096) ...
        if labels is not None:
            undo.append((engine.clear_players, False))      # ... and a player map never outlives the call that set it
        n, state = 0, None
        while n < max_samples:
            rows = source.take(min(batch_size, max_samples - n))
            if len(rows) == 0:
                break
            engine.pairs_batch(rows)
            n += len(rows)
            state = None
            if tolerance is not None:
                state = engine.pairs_get()      # the state is read once per batch
                _, _, counts, _, m2 = state
                if counts[off].min() >= 2 and pair_standard_errors(counts, m2).max() <= tolerance:
                    break
        if n == 0:
            raise ValueError("no ordering to sample: perms is empty")
        n, phi, counts, mean, m2 = state if state is not None else engine.pairs_get()
        _info_verdict(info | (engine.info_collected() if hasattr(engine, "info_collected") else engine.info()),
                      stacklevel=2)
        if info & 1:
            theta, r_squared = _singular_fit(engine, data[1], data[3])
    return SampledInteractionResults(interactions=_shap_matrix(phi, mean), attribution=phi, theta=theta,
                                     r_squared=r_squared, interaction_errors=pair_standard_errors(counts, m2),
                                     counts=counts, n_samples=int(n))


MULTI_LIFT_MAX_P = 104     # include/lsspa.h, LSSPA_MULTI_LIFT_MAX_P


def ls_spa_multi_sampled(X_train, X_test, Y_train, Y_test, reg=0., max_samples=2 ** 13, batch_size=2 ** 8,
                         tolerance=None, seed=42, perms=None, *, groups=None, method="random", antithetical=True,
                         device=0, _engine=None):
    """Sampled Shapley attribution of many responses on one design matrix (p <= 104): what ``ls_spa_multi`` gives
    exactly for p <= 32, estimated from sampled orderings beyond that.

    ``Y_train`` is [N][m] and ``Y_test`` [M][m] (a one-dimensional y counts as m = 1).  Every response sees the same
    orderings, and of an ordering's work the two Cholesky factorisations and the triangular solve between them do not
    depend on y: a workgroup carries eight responses through them at once, and only the O(p^2) lift scan is per response
    (include/lsspa.h, lsspa_multi_lift_batch).  The rows of X are reduced once, by one Gram pass per side over [X | Y].
    fp64 throughout; two calls agree bitwise.

    Returns ``SampledMultiResults``: ``attribution`` [m][p] is the mean of the samples' lift vectors, row r an estimate
    of what ``ls_spa(X_train, X_test, Y_train[:, r], Y_test[:, r], reg)`` estimates, and sums to ``r_squared[r]``;
    ``attribution_errors`` [m][p] its standard errors sqrt(M2 / (n (n - 1))) (``inf`` while n < 2; indicative only for
    the QMC sources and a caller's ``perms``, whose samples are not independent); ``theta`` [m][p] and ``r_squared`` [m]
    the full models'; ``n_samples``.

    max_samples, batch_size:  samples are drawn in batches of ``batch_size`` until ``max_samples``.
    tolerance:  None (default): run to ``max_samples``.  Otherwise sampling stops after the first batch at which
        n >= 2 and the largest standard error is <= tolerance.
    method:  'random' (default), 'argsort', 'permutohedron', or 'exact' (all p! orderings, p up to 8 or 9): the ordering
        sources of ``ls_spa``.
    perms:  an iterable of orderings instead (leave ``method`` at its default).
    antithetical:  a sample is the mean of an ordering and its reverse (default), as in ``ls_spa``.
    groups:  one integer label per column as ``ls_spa_groups`` takes them: k in 0 .. g-1 puts the column into group k,
        -1 into a baseline that every model includes (any 1 <= g <= p; p <= 104 and M >= p as without groups).  The
        players are then the g groups and the result is a ``SampledMultiGroupResults``: row r of ``attribution`` [m][g]
        estimates what ``ls_spa_groups(X_train, X_test, Y_train[:, r], Y_test[:, r], groups, reg)`` estimates and sums
        to ``r_squared[r] - baseline_r_squared[r]``, ``attribution_errors`` is [m][g], ``baseline_r_squared`` [m] each
        response's R^2 of the baseline columns alone (0 without a baseline).  The ordering sources run in dimension g:
        'exact' is all g! group orderings, ``perms`` an iterable of permutations of 0 .. g-1; with ``antithetical`` a
        sample is a group ordering and its reverse, the baseline first in both.  The kernel folds a response's column
        lifts to group lifts itself (include/lsspa.h, lsspa_multi_lift_set_players).  Labels are refused with
        ValueError before any GPU work.

    Shapes that do not fit raise ``SizeIncompatible``; p > 104, M < p (the test Gram matrix must have a Cholesky factor)
    or p + m > 32767 ValueError naming the limit, before any GPU work.  A column of ``Y_test`` that is identically zero
    is a ValueError, a Gram matrix that is not numerically positive definite a RuntimeWarning (it is shared, so it
    concerns every response); theta is then the solution of minimal norm.  Several ranks, checkpoints and fp32 are not
    part of this function."""
    X_train, X_test = np.asarray(X_train), np.asarray(X_test)
    Y_train, Y_test = np.asarray(Y_train), np.asarray(Y_test)
    if X_train.ndim != 2 or X_test.ndim != 2:
        raise ValueError("X_train and X_test must be two-dimensional")
    if Y_train.ndim == 1:
        Y_train = Y_train[:, None]
    if Y_test.ndim == 1:
        Y_test = Y_test[:, None]
    if Y_train.ndim != 2 or Y_test.ndim != 2:
        raise ValueError("Y_train and Y_test must be [rows][m] (or one-dimensional for one response)")
    if Y_train.shape[1] != Y_test.shape[1]:
        raise SizeIncompatible("Y_train and Y_test should have the same number of columns (responses).")
    validate_data(X_train, X_test, Y_train, Y_test)
    p, m, M = X_train.shape[1], Y_train.shape[1], X_test.shape[0]
    if p < 1 or m < 1:
        raise ValueError(f"ls_spa_multi_sampled needs p >= 1 features and m >= 1 responses (p = {p}, m = {m})")
    if p > MULTI_LIFT_MAX_P:
        raise ValueError(f"ls_spa_multi_sampled takes at most p = {MULTI_LIFT_MAX_P} features (this problem has "
                         f"p = {p}); use ls_spa per response")
    if M < p:
        raise ValueError(f"ls_spa_multi_sampled takes M >= p test rows (M = {M}, p = {p}): the test Gram matrix must "
                         "have a Cholesky factor; use ls_spa per response")
    if p + m > MULTI_MAX_COLS:
        raise ValueError(f"ls_spa_multi_sampled takes p + m <= {MULTI_MAX_COLS} columns of [X | Y] (p = {p}, m = {m}); "
                         "cut the responses into several calls")
    labels, d, source, batch_size, antithetical, max_samples, never_stop = _sampled_arguments(
        p, groups, perms, method, max_samples, batch_size, seed, antithetical)
    if never_stop:
        tolerance = None
    undo = [(lambda: _close_source(source), True)]
    with _engine_call(_engine, device, undo=undo) as engine:
        undo.append((engine.multi_lift_free, True))
        engine.multi_lift_load(X_train, X_test, Y_train, Y_test, reg)
        if labels is not None:
            engine.multi_lift_set_players(labels)      # (multi_lift_free drops the map with everything else)
        n, mean, m2 = _sample_until(source, lambda rows: engine.multi_lift_batch(rows, antithetical),
                                    engine.multi_lift_get, lambda state: _multi_standard_errors(state[0], state[2]).max(),
                                    batch_size, max_samples, tolerance)
        bits = engine.multi_lift_info()
        gram = engine.multi_lift_gram()
        theta, r_squared, singular = _multi_fit(*gram)
    bits |= int(singular)
    # every sample's lifts of response r telescope to r_squared[r] -- over groups from the baseline's R^2 to it --, so
    # every row of the mean sums to that (the bound of LSSPA_INFO_SUM for well-conditioned data)
    base = np.zeros(m) if labels is None else _multi_baseline_r_squared(*gram, labels)
    if not bits & 1 and not np.all(np.abs(mean.sum(axis=1) - (r_squared - base))
                                   <= 1e-9 * np.maximum(1.0, np.abs(r_squared))):
        bits |= 8
    _info_verdict(bits, stacklevel=2)
    if labels is not None:
        return SampledMultiGroupResults(attribution=mean, attribution_errors=_multi_standard_errors(n, m2), theta=theta,
                                        r_squared=r_squared, baseline_r_squared=base, n_samples=int(n))
    return SampledMultiResults(attribution=mean, attribution_errors=_multi_standard_errors(n, m2), theta=theta,
                               r_squared=r_squared, n_samples=int(n))


def _multi_standard_errors(n, m2):
    """Standard errors of the running means: sqrt(M2 / (n (n - 1))), inf while n < 2."""
    if n < 2:
        return np.full(np.shape(m2), np.inf)
    return np.sqrt(np.maximum(m2, 0.0) / (float(n) * (n - 1.0)))


# ------------------------------------------------------------------------------------------
# helper-level surface of the reference (called by its notebooks and tests)
# ------------------------------------------------------------------------------------------
_helper_engine = None


def _helper():
    global _helper_engine
    if _helper_engine is None:
        from ._engine import HipEngine
        _helper_engine = HipEngine(0)
    return _helper_engine


def reduce_data(X_train, X_test, y_train, y_test, reg):
    """(R_tr, F_te, q_tr, q_te) with R_tr^T R_tr = X_tr^T X_tr / N + reg I, R_tr^T q_tr = X_tr^T y_tr / N,
    F_te^T F_te = X_te^T X_te, F_te^T q_te = X_te^T y_te -- the contract of the reference's
    ``reduce_data`` (ls_spa/ls_spa.py:290-318).  Here R_tr is the Cholesky factor of the MFMA Gram
    matrix (positive diagonal), so it equals LAPACK's QR factor up to row signs."""
    eng = _helper()
    eng.load_data(np.array(X_train), np.array(X_test), np.array(y_train), np.array(y_test), reg)
    return eng.factors()


def square_shapley(X_train, X_test, y_train, y_test, y_norm_sq, perm):
    """Lift vector of one ordering from reduced factors (ls_spa/ls_spa.py:256-287): arguments are
    the four outputs of ``reduce_data``, ||y_test||^2 of the raw labels and the ordering."""
    R, F = np.asarray(X_train, dtype=np.float64), np.asarray(X_test, dtype=np.float64)
    q, qt = np.asarray(y_train, dtype=np.float64), np.asarray(y_test, dtype=np.float64)
    eng = _helper()
    eng.load_reduced(R.T @ R, R.T @ q, float(q @ q), float(y_norm_sq), Ft=F.T.copy(), ytil=qt)
    return eng.run_batch(np.asarray(perm)[None, :], False, want_lifts=True, accumulate=False)[0]
