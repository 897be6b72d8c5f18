"""Device engine: a thin object wrapper over the C ABI (one context = one GPU).

The driver (``_driver.py``) only talks to this interface:

    load_data / load_reduced      one-time reduction (a1)
    full_fit                      theta, r_squared (a7)
    run_batch                     lift vectors of a batch of orderings (a2, a3) and the
                                  batch's moments about the running mean (a4)
    pending_buffer / merge        the all-reduce target and the Chan merge (a4, multi-GPU)
    stats                         n, mean, biased covariance
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native as N


class DeviceArrayView:
    """Zero-copy view of a device buffer for consumers of ``__cuda_array_interface__``
    (torch.as_tensor on ROCm included): used to hand the pending-statistics buffer to
    torch.distributed without going through the host."""

    def __init__(self, ptr: int, count: int, owner):
        self._owner = owner  # keeps the context alive
        self.__cuda_array_interface__ = {
            "shape": (int(count),),
            "typestr": "<f8",
            "data": (int(ptr), False),
            "version": 2,
            "strides": None,
        }


def debug_expand_groups(labels, group_perms, antithetical: bool):
    """Test hook, host only (no engine, no GPU): the column orderings the kernels are given for (B, g) orderings of the
    groups under a player map of these labels (include/lsspa.h, lsspa_debug_expand_groups)."""
    lib = N.load()
    labels = np.ascontiguousarray(labels, dtype=np.int32).ravel()
    g = int(labels.max()) + 1 if len(labels) else 0
    group_perms = np.ascontiguousarray(group_perms, dtype=np.int32)
    if group_perms.ndim != 2 or group_perms.shape[1] != g:
        raise ValueError(f"group_perms must have shape (B, {g})")
    B = group_perms.shape[0]
    out = np.empty((B * (2 if antithetical else 1), len(labels)), dtype=np.int32)
    rc = lib.lsspa_debug_expand_groups(N.iptr(labels), len(labels), g, N.iptr(group_perms), B, int(bool(antithetical)),
                                       N.iptr(out))
    if rc != N.OK:
        raise ValueError(f"lsspa_debug_expand_groups: status {rc} (labels or a row of group_perms refused)")
    return out


def debug_expand_pairs(perms):
    """Test hook, host only (no engine, no GPU): the (3 B, d) orderings a batch of sampled pairwise interactions runs for
    the (B, d) orderings ``perms`` (include/lsspa.h, lsspa_debug_expand_pairs): row 3 s is perms[s], row 3 s + 1 has its
    positions (0,1), (2,3), .. swapped, row 3 s + 2 its positions (1,2), (3,4), ..."""
    perms = np.ascontiguousarray(perms, dtype=np.int32)
    if perms.ndim != 2 or perms.shape[0] < 1 or perms.shape[1] < 1:
        raise ValueError("perms must have shape (B, d)")
    out = np.empty((3 * perms.shape[0], perms.shape[1]), dtype=np.int32)
    rc = N.load().lsspa_debug_expand_pairs(perms.shape[1], N.iptr(perms), perms.shape[0], N.iptr(out))
    if rc != N.OK:
        raise ValueError(f"lsspa_debug_expand_pairs: status {rc} (a row of perms is not a permutation)")
    return out


def debug_stats_slices(n_samples: int, p: int):
    """Test hook, host only: (samples given to every slice of a chunk's moments, small) as the library cuts a chunk of
    n_samples at dimension p (include/lsspa.h, lsspa_debug_stats_slices)."""
    nz, per, small = C.c_int32(), C.c_int32(), C.c_int32()
    rc = N.load().lsspa_debug_stats_slices(int(n_samples), int(p), C.byref(nz), C.byref(per), C.byref(small))
    if rc != N.OK:
        raise ValueError(f"lsspa_debug_stats_slices: status {rc}")
    return [max(0, min(n_samples, (k + 1) * per.value) - k * per.value) for k in range(nz.value)], bool(small.value)


BOOT_PLAN_FIELDS = ("cb", "ldz", "pairs", "rpw", "rps_train", "rps_test", "slices_train", "slices_test", "rep_bytes",
                    "block", "n_blocks", "enum_reps", "units", "per", "steps")


def debug_boot_plan(R: int, n: int, m: int, p: int, block: int = 0, inter: bool = False):
    """Test hook, host only: how a bootstrap run of R replicates on n / m rows at p features is cut (include/lsspa.h,
    lsspa_debug_boot_plan), as a dict of BOOT_PLAN_FIELDS.  inter: the run of the interaction values
    (lsspa_debug_boot_inter_plan), whose rep_bytes leave the enumeration's partial table out."""
    out = np.zeros(15, dtype=np.int64)
    name = "lsspa_debug_boot_inter_plan" if inter else "lsspa_debug_boot_plan"
    rc = getattr(N.load(), name)(int(R), int(n), int(m), int(p), int(block), out.ctypes.data_as(N._pi64))
    if rc != N.OK:
        raise ValueError(f"{name}: status {rc}")
    return dict(zip(BOOT_PLAN_FIELDS, (int(v) for v in out)))


def debug_boot_best_plan(R: int, n: int, m: int, p: int, block: int = 0):
    """Test hook, host only: debug_boot_plan for a bootstrap of the best-subset selection (include/lsspa.h,
    lsspa_debug_boot_best_plan): rep_bytes counts 16 bytes an entry of the enumeration's table."""
    out = np.zeros(15, dtype=np.int64)
    rc = N.load().lsspa_debug_boot_best_plan(int(R), int(n), int(m), int(p), int(block), out.ctypes.data_as(N._pi64))
    if rc != N.OK:
        raise ValueError(f"lsspa_debug_boot_best_plan: status {rc}")
    return dict(zip(BOOT_PLAN_FIELDS, (int(v) for v in out)))


PERM_PLAN_FIELDS = ("block", "n_blocks", "rps_train", "rps_test", "slices_train", "slices_test", "cb", "ldi_train",
                    "ldi_test", "rep_bytes")


def debug_perm_plan(R: int, n: int, m: int, p: int, block: int = 0):
    """Test hook, host only: how a permutation-test run of R replicates on n / m rows at p columns is cut
    (include/lsspa.h, lsspa_debug_perm_plan), as a dict of PERM_PLAN_FIELDS."""
    out = np.zeros(10, dtype=np.int64)
    rc = N.load().lsspa_debug_perm_plan(int(R), int(n), int(m), int(p), int(block), out.ctypes.data_as(N._pi64))
    if rc != N.OK:
        raise ValueError(f"lsspa_debug_perm_plan: status {rc}")
    return dict(zip(PERM_PLAN_FIELDS, (int(v) for v in out)))


def debug_perm_indices(seed: int, r: int, side: int, n: int):
    """Test hook, host only: the permutation a [n] (uint32) of (seed, replicate r, side, n): y_pi[i] = y[a[i]]
    (include/lsspa.h, lsspa_debug_perm_indices)."""
    out = np.empty(max(int(n), 0), dtype=np.uint32)
    rc = N.load().lsspa_debug_perm_indices(int(seed) & (2 ** 64 - 1), int(r) & (2 ** 64 - 1), int(side), int(n),
                                           out.ctypes.data_as(C.POINTER(C.c_uint32)))
    if rc != N.OK:
        raise ValueError(f"lsspa_debug_perm_indices: status {rc}")
    return out


def debug_boot_groups_plan(R: int, n: int, m: int, labels, block: int = 0, inter: bool = False):
    """Test hook, host only: debug_boot_plan for a bootstrap over the groups of columns that labels names (one label per
    column; include/lsspa.h, lsspa_debug_boot_groups_plan).  ValueError for labels or sizes the library refuses.
    inter: the run of the interaction values (lsspa_debug_boot_groups_inter_plan)."""
    labels = np.ascontiguousarray(labels, dtype=np.int32).ravel()
    g = int(labels.max()) + 1 if len(labels) else 0
    out = np.zeros(15, dtype=np.int64)
    name = "lsspa_debug_boot_groups_inter_plan" if inter else "lsspa_debug_boot_groups_plan"
    rc = getattr(N.load(), name)(int(R), int(n), int(m), N.iptr(labels), len(labels), g, int(block),
                                 out.ctypes.data_as(N._pi64))
    if rc != N.OK:
        raise ValueError(f"{name}: status {rc}")
    return dict(zip(BOOT_PLAN_FIELDS, (int(v) for v in out)))


def debug_boot_groups_best_plan(R: int, n: int, m: int, labels, block: int = 0):
    """Test hook, host only: debug_boot_groups_plan for a bootstrap of the best-subset selection over the groups of labels
    (include/lsspa.h, lsspa_debug_boot_groups_best_plan): rep_bytes counts 16 bytes an entry of the enumeration's table,
    and steps / enum_reps are chosen for speed within the launch bounds."""
    labels = np.ascontiguousarray(labels, dtype=np.int32).ravel()
    g = int(labels.max()) + 1 if len(labels) else 0
    out = np.zeros(15, dtype=np.int64)
    rc = N.load().lsspa_debug_boot_groups_best_plan(int(R), int(n), int(m), N.iptr(labels), len(labels), g, int(block),
                                                    out.ctypes.data_as(N._pi64))
    if rc != N.OK:
        raise ValueError(f"lsspa_debug_boot_groups_best_plan: status {rc}")
    return dict(zip(BOOT_PLAN_FIELDS, (int(v) for v in out)))


OWEN_PLAN_FIELDS = ("players", "gl", "gh", "ql", "inner_low", "inner_high", "high_subsets", "launches")


def debug_owen_plan(labels):
    """Test hook, host only: per target group, how groups_owen enumerates its refined game (include/lsspa.h,
    lsspa_debug_owen_plan) -- a list of g dicts with OWEN_PLAN_FIELDS.  ValueError for labels the library refuses."""
    labels = np.ascontiguousarray(labels, dtype=np.int32).ravel()
    g = int(labels.max()) + 1 if len(labels) else 0
    out = np.zeros((max(g, 1), 8), dtype=np.int64)
    rc = N.load().lsspa_debug_owen_plan(N.iptr(labels), len(labels), g, out.ctypes.data_as(N._pi64))
    if rc != N.OK:
        raise ValueError(f"lsspa_debug_owen_plan: status {rc}")
    return [dict(zip(OWEN_PLAN_FIELDS, (int(v) for v in row))) for row in out[:g]]


GROUPS_BEST_PLAN_FIELDS = ("gl", "gh", "ql", "nb", "units", "per", "launches", "classes")


def debug_groups_best_plan(labels):
    """Test hook, host only: how groups_best enumerates the group game of these labels (include/lsspa.h,
    lsspa_debug_groups_best_plan) -- a dict with GROUPS_BEST_PLAN_FIELDS.  ValueError for labels the library refuses."""
    labels = np.ascontiguousarray(labels, dtype=np.int32).ravel()
    g = int(labels.max()) + 1 if len(labels) else 0
    out = np.zeros(8, dtype=np.int64)
    rc = N.load().lsspa_debug_groups_best_plan(N.iptr(labels), len(labels), g, out.ctypes.data_as(N._pi64))
    if rc != N.OK:
        raise ValueError(f"lsspa_debug_groups_best_plan: status {rc}")
    return dict(zip(GROUPS_BEST_PLAN_FIELDS, (int(v) for v in out)))


GROUPS_TOP_PLAN_FIELDS = ("gl", "gh", "ql", "nb", "units", "per", "steps", "launches", "sizes", "table_bytes")


def debug_groups_top_plan(labels, n_best: int):
    """Test hook, host only: how groups_top enumerates the group game of these labels for n_best models a size
    (include/lsspa.h, lsspa_debug_groups_top_plan) -- a dict with GROUPS_TOP_PLAN_FIELDS.  ValueError for labels or an
    n_best the library refuses."""
    labels = np.ascontiguousarray(labels, dtype=np.int32).ravel()
    g = int(labels.max()) + 1 if len(labels) else 0
    out = np.zeros(10, dtype=np.int64)
    rc = N.load().lsspa_debug_groups_top_plan(N.iptr(labels), len(labels), g, int(n_best), out.ctypes.data_as(N._pi64))
    if rc != N.OK:
        raise ValueError(f"lsspa_debug_groups_top_plan: status {rc}")
    return dict(zip(GROUPS_TOP_PLAN_FIELDS, (int(v) for v in out)))


SUBSETS_TOP_PLAN_FIELDS = ("units", "per", "steps", "launches", "sizes", "table_bytes", "reduce_rounds")


def debug_subsets_top_plan(p: int, n_best: int):
    """Test hook, host only: how subsets_top enumerates p features for n_best models a size (include/lsspa.h,
    lsspa_debug_subsets_top_plan) -- a dict with SUBSETS_TOP_PLAN_FIELDS.  ValueError for a p or n_best the library
    refuses."""
    out = np.zeros(8, dtype=np.int64)
    rc = N.load().lsspa_debug_subsets_top_plan(int(p), int(n_best), out.ctypes.data_as(N._pi64))
    if rc != N.OK:
        raise ValueError(f"lsspa_debug_subsets_top_plan: status {rc}")
    return dict(zip(SUBSETS_TOP_PLAN_FIELDS, (int(v) for v in out)))


CV_PLAN_FIELDS = ("units", "per", "steps", "launches", "lds_bytes", "workgroup")


def debug_cv_plan(p: int, folds: int):
    """Test hook, host only: how cv_best enumerates p features over `folds` fold problems (include/lsspa.h,
    lsspa_debug_cv_plan) -- a dict with CV_PLAN_FIELDS.  ValueError for a p or a number of folds the library refuses."""
    out = np.zeros(8, dtype=np.int64)
    rc = N.load().lsspa_debug_cv_plan(int(p), int(folds), out.ctypes.data_as(N._pi64))
    if rc != N.OK:
        raise ValueError(f"lsspa_debug_cv_plan: status {rc}")
    return dict(zip(CV_PLAN_FIELDS, (int(v) for v in out)))


BOOT_LIFT_PLAN_FIELDS = ("cb", "gram_form", "rps_train", "rps_test", "slices_train", "slices_test", "block", "n_blocks",
                         "reps_per_launch", "orderings_per_launch", "samples_per_launch", "sample_cuts", "launches",
                         "raw_bytes", "lift_form", "rep_bytes")


def debug_boot_lift_plan(R: int, n: int, m: int, p: int, d: int, n_samples: int, antithetical: bool, block: int = 0):
    """Test hook, host only: how boot_lift_run cuts R replicates of n / m rows, p columns, samples of dimension d and
    n_samples samples (include/lsspa.h, lsspa_debug_boot_lift_plan) -- a dict with BOOT_LIFT_PLAN_FIELDS; gram_form 1 is
    the wide Gram kernel (cb = 6 .. 8), lift_form 1 the LDS-resident ordering kernel.  ValueError for arguments the
    library refuses."""
    out = np.zeros(16, dtype=np.int64)
    rc = N.load().lsspa_debug_boot_lift_plan(int(R), int(n), int(m), int(p), int(d), int(n_samples),
                                             int(bool(antithetical)), int(block), out.ctypes.data_as(N._pi64))
    if rc != N.OK:
        raise ValueError(f"lsspa_debug_boot_lift_plan: status {rc}")
    return dict(zip(BOOT_LIFT_PLAN_FIELDS, (int(v) for v in out)))


CV_LIFT_PLAN_FIELDS = ("nb", "form", "workgroups_per_sample", "samples_per_launch", "launches", "lds_bytes", "workgroup")


def debug_cv_lift_plan(p: int, d: int, folds: int, B: int, antithetical: bool):
    """Test hook, host only: how cv_lift_batch cuts a batch of B samples of dimension d over p columns and `folds` fold
    problems into launches (include/lsspa.h, lsspa_debug_cv_lift_plan) -- a dict with CV_LIFT_PLAN_FIELDS; form 0 is the
    register-resident kernel, 1 the LDS-resident one.  ValueError for arguments the library refuses."""
    out = np.zeros(8, dtype=np.int64)
    rc = N.load().lsspa_debug_cv_lift_plan(int(p), int(d), int(folds), int(B), int(bool(antithetical)),
                                           out.ctypes.data_as(N._pi64))
    if rc != N.OK:
        raise ValueError(f"lsspa_debug_cv_lift_plan: status {rc}")
    return dict(zip(CV_LIFT_PLAN_FIELDS, (int(v) for v in out)))


CV_TOP_PLAN_FIELDS = ("units", "per", "steps", "launches", "lds_bytes", "workgroup", "sizes", "table_bytes")


def debug_cv_top_plan(p: int, folds: int, n_best: int):
    """Test hook, host only: how cv_top enumerates p features over `folds` fold problems for n_best models a size
    (include/lsspa.h, lsspa_debug_cv_top_plan) -- a dict with CV_TOP_PLAN_FIELDS.  ValueError for a p, a number of folds
    or an n_best the library refuses."""
    out = np.zeros(8, dtype=np.int64)
    rc = N.load().lsspa_debug_cv_top_plan(int(p), int(folds), int(n_best), out.ctypes.data_as(N._pi64))
    if rc != N.OK:
        raise ValueError(f"lsspa_debug_cv_top_plan: status {rc}")
    return dict(zip(CV_TOP_PLAN_FIELDS, (int(v) for v in out)))


CV_GROUPS_PLAN_FIELDS = ("gl", "gh", "ql", "nb", "units", "per", "steps", "launches", "lds_bytes", "workgroup",
                         "lds_bytes_one_problem", "launch_bound")


def debug_cv_groups_plan(labels, folds: int):
    """Test hook, host only: how cv_groups_best enumerates the group game of these labels over `folds` fold problems
    (include/lsspa.h, lsspa_debug_cv_groups_plan) -- a dict with CV_GROUPS_PLAN_FIELDS.  ValueError for labels or a
    number of folds the library refuses."""
    labels = np.ascontiguousarray(labels, dtype=np.int32).ravel()
    g = int(labels.max()) + 1 if len(labels) else 0
    out = np.zeros(12, dtype=np.int64)
    rc = N.load().lsspa_debug_cv_groups_plan(N.iptr(labels), len(labels), g, int(folds), out.ctypes.data_as(N._pi64))
    if rc != N.OK:
        raise ValueError(f"lsspa_debug_cv_groups_plan: status {rc}")
    return dict(zip(CV_GROUPS_PLAN_FIELDS, (int(v) for v in out)))


CV_GROUPS_TOP_PLAN_FIELDS = ("gl", "gh", "ql", "nb", "units", "per", "steps", "launches", "lds_bytes", "workgroup",
                             "sizes", "table_bytes")


def debug_cv_groups_top_plan(labels, folds: int, n_best: int):
    """Test hook, host only: how cv_groups_top enumerates the group game of these labels over `folds` fold problems for
    n_best models a size (include/lsspa.h, lsspa_debug_cv_groups_top_plan) -- a dict with CV_GROUPS_TOP_PLAN_FIELDS.
    ValueError for labels, a number of folds or an n_best the library refuses."""
    labels = np.ascontiguousarray(labels, dtype=np.int32).ravel()
    g = int(labels.max()) + 1 if len(labels) else 0
    out = np.zeros(12, dtype=np.int64)
    rc = N.load().lsspa_debug_cv_groups_top_plan(N.iptr(labels), len(labels), g, int(folds), int(n_best),
                                                 out.ctypes.data_as(N._pi64))
    if rc != N.OK:
        raise ValueError(f"lsspa_debug_cv_groups_top_plan: status {rc}")
    return dict(zip(CV_GROUPS_TOP_PLAN_FIELDS, (int(v) for v in out)))


CV_PATH_PLAN_FIELDS = ("units", "per", "steps", "block", "blocks", "reps", "launches", "bound")


def debug_cv_path_plan(p: int, folds: int, n_regs: int, block: int = 0):
    """Test hook, host only: how cv_path_shapley runs n_regs ridge values of p features over `folds` fold problems
    (include/lsspa.h, lsspa_debug_cv_path_plan) -- a dict with CV_PATH_PLAN_FIELDS.  ValueError for arguments the
    library refuses."""
    out = np.zeros(8, dtype=np.int64)
    rc = N.load().lsspa_debug_cv_path_plan(int(p), int(folds), int(n_regs), int(block), out.ctypes.data_as(N._pi64))
    if rc != N.OK:
        raise ValueError(f"lsspa_debug_cv_path_plan: status {rc}")
    return dict(zip(CV_PATH_PLAN_FIELDS, (int(v) for v in out)))


CV_PATH_GROUPS_PLAN_FIELDS = ("gl", "gh", "ql", "nb") + CV_PATH_PLAN_FIELDS


def debug_cv_path_groups_plan(labels, folds: int, n_regs: int, block: int = 0):
    """Test hook, host only: how cv_path_groups_shapley runs n_regs ridge values of the group game of these labels over
    `folds` fold problems (include/lsspa.h, lsspa_debug_cv_path_groups_plan) -- a dict with
    CV_PATH_GROUPS_PLAN_FIELDS.  ValueError for arguments the library refuses."""
    labels = np.ascontiguousarray(labels, dtype=np.int32).ravel()
    g = int(labels.max()) + 1 if len(labels) else 0
    out = np.zeros(12, dtype=np.int64)
    rc = N.load().lsspa_debug_cv_path_groups_plan(N.iptr(labels), len(labels), g, int(folds), int(n_regs), int(block),
                                                  out.ctypes.data_as(N._pi64))
    if rc != N.OK:
        raise ValueError(f"lsspa_debug_cv_path_groups_plan: status {rc}")
    return dict(zip(CV_PATH_GROUPS_PLAN_FIELDS, (int(v) for v in out)))


def debug_gram_plan(n: int, p: int):
    """Test hook, host only: how a Gram launch of n rows at p features is cut (include/lsspa.h, lsspa_debug_gram_plan) --
    a dict of n_split, nt, xlive and, per unit class A / B / C, cnt, slices and rps (rows per slice)."""
    ns, nt, xl = C.c_int32(), C.c_int32(), C.c_int32()
    cnt, sl, rps = (np.zeros(3, dtype=np.int32) for _ in range(3))
    rc = N.load().lsspa_debug_gram_plan(int(n), int(p), C.byref(ns), N.iptr(cnt), N.iptr(sl), N.iptr(rps), C.byref(nt),
                                        C.byref(xl))
    if rc != N.OK:
        raise ValueError(f"lsspa_debug_gram_plan: status {rc}")
    return {"n_split": ns.value, "nt": nt.value, "xlive": xl.value, "cnt": [int(v) for v in cnt],
            "slices": [int(v) for v in sl], "rps": [int(v) for v in rps]}


PANEL_PLAN_FIELDS = ("Jo", "n_lt", "n_x", "grouped", "xlast", "grid", "p_live", "n_ord")


def debug_panel_plan(p: int, n_ord: int, tri: bool, flags: int = 0):
    """Test hook, host only: the panel launches of the general path for n_ord orderings at p features (include/lsspa.h,
    lsspa_debug_panel_plan) -- a dict of p_pad, n_mats and launches, a list with one dict of PANEL_PLAN_FIELDS per
    launch (grouped and xlast as bool)."""
    pp, nm, nl = C.c_int32(), C.c_int32(), C.c_int32()
    fn = N.load().lsspa_debug_panel_plan
    rc = fn(int(p), int(n_ord), int(bool(tri)), int(flags), C.byref(pp), C.byref(nm), C.byref(nl), None, 0)
    if rc != N.OK:
        raise ValueError(f"lsspa_debug_panel_plan: status {rc}")
    out = np.zeros((nl.value, 8), dtype=np.int32)
    rc = fn(int(p), int(n_ord), int(bool(tri)), int(flags), C.byref(pp), C.byref(nm), C.byref(nl), N.iptr(out),
            nl.value)
    if rc != N.OK:
        raise ValueError(f"lsspa_debug_panel_plan: status {rc}")
    return {"p_pad": pp.value, "n_mats": nm.value, "launches": [_panel_plan_dict(row) for row in out]}


def debug_panel_plan_launch(p_pad: int, Jo: int, n_mats: int, n_ord: int, has_X: bool, p_live: int):
    """Test hook, host only: one panel launch from launch_chol2_panel's own arguments, a dict of PANEL_PLAN_FIELDS;
    ValueError for what the launch refuses (include/lsspa.h, lsspa_debug_panel_plan_launch)."""
    out = np.zeros(8, dtype=np.int32)
    rc = N.load().lsspa_debug_panel_plan_launch(int(p_pad), int(Jo), int(n_mats), int(n_ord), int(bool(has_X)),
                                                int(p_live), N.iptr(out))
    if rc != N.OK:
        raise ValueError(f"lsspa_debug_panel_plan_launch: status {rc}")
    return _panel_plan_dict(out)


def _panel_plan_dict(row):
    d = dict(zip(PANEL_PLAN_FIELDS, (int(v) for v in row)))
    d["grouped"], d["xlast"] = bool(d["grouped"]), bool(d["xlast"])
    return d


class HipEngine:
    """One MI355X.  Raises LSSPANativeError when the HIP library or the GPU is missing."""

    def __init__(self, device: int = 0, stream: int | None = None):
        self._lib = N.load()
        h = C.c_void_p()
        rc = self._lib.lsspa_create(int(device), C.byref(h))
        if rc != N.OK:
            msg = self._lib.lsspa_last_error(None)
            raise N.LSSPANativeError(f"lsspa_create(device={device}) failed: {msg.decode() if msg else rc}")
        self._h = h
        self.device = int(device)
        self.p = 0
        self.players = 0      # groups of a player map (set_players); 0: the columns are the players
        self.m = 0
        self.tri = False
        self.y_norm_sq = float("nan")
        self.precision = "float64"
        self.lanes = 1
        if stream is not None:
            self._check(self._lib.lsspa_set_stream(self._h, C.c_void_p(int(stream))))

    # ---- plumbing -------------------------------------------------------------------
    def _check(self, rc: int):
        if rc != N.OK:
            msg = self._lib.lsspa_last_error(self._h)
            text = msg.decode() if msg else ""
            if rc == 1:
                raise ValueError(f"lsspa: {text}")
            if rc == 4:
                raise MemoryError(f"lsspa: {text}")
            raise N.LSSPANativeError(f"lsspa call failed (status {rc}): {text}")

    def close(self):
        if getattr(self, "_h", None):
            self._lib.lsspa_destroy(self._h)
            self._h = None

    def __del__(self):  # pragma: no cover - best effort
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self):
        self._check(self._lib.lsspa_synchronize(self._h))

    def _refresh_dims(self):
        p, m, tri, yy = C.c_int32(), C.c_int32(), C.c_int32(), C.c_double()
        self._check(self._lib.lsspa_get_problem(self._h, C.byref(p), C.byref(m), C.byref(tri), C.byref(yy)))
        self.p, self.m, self.tri, self.y_norm_sq = p.value, m.value, bool(tri.value), yy.value
        self.players = 0      # a reduction drops the player map (include/lsspa.h)

    @property
    def dim(self) -> int:
        """Dimension of a sample: lift vectors, statistics, history, estimator results.  p, or g under a player map."""
        return self.players or self.p

    # ---- groups of columns as the players of the sampling path ---------------------------------
    def set_players(self, labels):
        """One label per column (-1 the baseline, 0 .. g-1 the groups): from now on run_batch / launch_batch take
        (B, g) orderings of the groups and everything a sample is has length g (include/lsspa.h, lsspa_set_players).
        Resets the statistics; history and estimator have to be enabled again."""
        labels, g = self._labels(labels)
        if len(labels) != self.p:
            raise ValueError(f"labels must have length p = {self.p}")
        self._check(self._lib.lsspa_set_players(self._h, N.iptr(labels), g))
        self.players = g

    def clear_players(self):
        if self.players:
            self._check(self._lib.lsspa_set_players(self._h, None, 0))
            self.players = 0

    # ---- a1: reduction ---------------------------------------------------------------
    def load_data(self, X_train, X_test, y_train, y_test, reg: float):
        """Host ndarrays (float64 or float32, both sides alike) -> device Gram reduction."""
        dt = np.float32 if (X_train.dtype == np.float32 and X_test.dtype == np.float32) else np.float64
        Xa = np.ascontiguousarray(X_train, dtype=dt)
        Xe = np.ascontiguousarray(X_test, dtype=dt)
        ya = np.ascontiguousarray(y_train, dtype=dt)
        ye = np.ascontiguousarray(y_test, dtype=dt)
        n, p = Xa.shape
        mrows = Xe.shape[0]
        self._check(self._lib.lsspa_reduce(
            self._h, Xa.ctypes.data, p, ya.ctypes.data, n, Xe.ctypes.data, p, ye.ctypes.data, mrows, p,
            float(reg), N.F32 if dt == np.float32 else N.F64, N.HOST))
        self._refresh_dims()

    def reduce_timing(self):
        """Host seconds of the last reduction from host arrays: page-locking, streamed copies + Gram kernels,
        un-locking, finalize (include/lsspa.h, lsspa_reduce_timing)."""
        out = np.zeros(4)
        self._check(self._lib.lsspa_reduce_timing(self._h, N.dptr(out)))
        return dict(zip(("pin", "h2d_gram", "unpin", "finalize"), (float(v) for v in out)))

    def load_data_sharded(self, X_train, X_test, y_train, y_test, reg: float, comm, shard_test: bool = True):
        """Row-sharded reduction: the arrays are THIS rank's rows; one all-reduce of the Gram sums
        (2 (p+1)^2 fp64, padded) replaces moving the rows.  shard_test=False: every rank passes all the
        test rows (required when there are fewer than p of them) and rank 0 alone contributes them."""
        dt = np.float32 if (X_train.dtype == np.float32 and X_test.dtype == np.float32) else np.float64
        Xa = np.ascontiguousarray(X_train, dtype=dt)
        Xe = np.ascontiguousarray(X_test, dtype=dt)
        ya = np.ascontiguousarray(y_train, dtype=dt)
        ye = np.ascontiguousarray(y_test, dtype=dt)
        n_loc, p = Xa.shape
        m_loc = Xe.shape[0]
        n_tot, m_sum = comm.sum_ints([n_loc, m_loc])
        m_tot = m_sum if shard_test else m_loc
        if not shard_test and m_tot >= p and comm.rank != 0:
            m_loc = 0   # replicated test rows enter the Gram sum once
        self._check(self._lib.lsspa_reduce_partial(
            self._h, Xa.ctypes.data, p, ya.ctypes.data, n_loc, Xe.ctypes.data, p, ye.ctypes.data, m_loc, m_tot, p,
            N.F32 if dt == np.float32 else N.F64, N.HOST))
        comm.allreduce_reduction(self)
        self._check(self._lib.lsspa_reduce_finish(self._h, int(n_tot), float(reg)))
        self._refresh_dims()
        return n_tot, m_tot

    def reduce_partial_device(self, X_train_ptr, ld_train, y_train_ptr, n_local, X_test_ptr, ld_test, y_test_ptr,
                              m_local, m_total, p, f32=False):
        """Device-pointer form of the first step (rows already in HBM)."""
        self._check(self._lib.lsspa_reduce_partial(
            self._h, C.c_void_p(X_train_ptr), ld_train, C.c_void_p(y_train_ptr), n_local, C.c_void_p(X_test_ptr),
            ld_test, C.c_void_p(y_test_ptr), m_local, m_total, p, N.F32 if f32 else N.F64, N.DEVICE))

    def reduce_buffer(self) -> DeviceArrayView:
        ptr, cnt = C.c_void_p(), C.c_int64()
        self._check(self._lib.lsspa_reduce_buffer(self._h, C.byref(ptr), C.byref(cnt)))
        return DeviceArrayView(ptr.value, cnt.value, self)

    def reduce_finish(self, n_total: int, reg: float):
        self._check(self._lib.lsspa_reduce_finish(self._h, int(n_total), float(reg)))
        self._refresh_dims()

    def load_device_data(self, X_train_ptr, ld_train, y_train_ptr, n, X_test_ptr, ld_test, y_test_ptr, m_rows,
                         p, reg, f32=False):
        """Same, from device pointers (e.g. torch tensors' data_ptr())."""
        self._check(self._lib.lsspa_reduce(
            self._h, C.c_void_p(X_train_ptr), ld_train, C.c_void_p(y_train_ptr), n, C.c_void_p(X_test_ptr),
            ld_test, C.c_void_p(y_test_ptr), m_rows, p, float(reg), N.F32 if f32 else N.F64, N.DEVICE))
        self._refresh_dims()

    def load_reduced(self, G, g, aug_train, y_norm_sq, H=None, h=None, Ft=None, ytil=None):
        G = np.ascontiguousarray(G, dtype=np.float64)
        g = np.ascontiguousarray(g, dtype=np.float64)
        p = G.shape[0]
        if H is not None:
            H = np.ascontiguousarray(H, dtype=np.float64)
            h = np.ascontiguousarray(h, dtype=np.float64)
            self._check(self._lib.lsspa_set_reduced(self._h, p, N.dptr(G), N.dptr(g), float(aug_train), 1,
                                                    N.dptr(H), N.dptr(h), p, None, None, float(y_norm_sq)))
        else:
            Ft = np.ascontiguousarray(Ft, dtype=np.float64)
            ytil = np.ascontiguousarray(ytil, dtype=np.float64)
            self._check(self._lib.lsspa_set_reduced(self._h, p, N.dptr(G), N.dptr(g), float(aug_train), 0,
                                                    None, None, Ft.shape[1], N.dptr(Ft), N.dptr(ytil),
                                                    float(y_norm_sq)))
        self._refresh_dims()

    def gram(self):
        p = self.p
        G, g = np.empty((p, p)), np.empty(p)
        if self.tri:
            H, h = np.empty((p, p)), np.empty(p)
            self._check(self._lib.lsspa_get_gram(self._h, N.dptr(G), N.dptr(g), N.dptr(H), N.dptr(h)))
            return G, g, H, h
        self._check(self._lib.lsspa_get_gram(self._h, N.dptr(G), N.dptr(g), None, None))
        return G, g, None, None

    # ---- a7 ----------------------------------------------------------------------------
    def full_fit(self):
        theta = np.empty(self.p)
        r2, info = C.c_double(), C.c_int32()
        self._check(self._lib.lsspa_full_fit(self._h, N.dptr(theta), C.byref(r2), C.byref(info)))
        return theta, r2.value, info.value

    # ---- exact attribution by subset enumeration (p <= 32) --------------------------------
    SUBSETS_MAX_P = 32

    def subsets_shapley(self):
        """(phi, info): the exact Shapley attribution of the loaded problem over all 2^p subsets (include/lsspa.h,
        lsspa_subsets_shapley); info & 1: a subset's Gram matrix was not numerically positive definite."""
        phi = np.empty(self.p)
        info = C.c_int32()
        self._check(self._lib.lsspa_subsets_shapley(self._h, N.dptr(phi), C.byref(info)))
        return phi, info.value

    def subsets_interactions(self):
        """(phi, I, info): phi as subsets_shapley gives it (bitwise) and the raw pairwise Shapley interaction index
        I [p][p] from the same enumeration (include/lsspa.h, lsspa_subsets_interactions): symmetric, 0 on the diagonal.
        subsets_timing() then speaks of this call."""
        phi, inter = np.empty(self.p), np.empty((self.p, self.p))
        info = C.c_int32()
        self._check(self._lib.lsspa_subsets_interactions(self._h, N.dptr(phi), N.dptr(inter), C.byref(info)))
        return phi, inter, info.value

    def subsets_best(self, include=0):
        """(v, masks, found, info): the best subset of every size k = 0 .. p by the out-of-sample R^2 v, over all 2^p
        subsets that contain the columns of the mask `include` (include/lsspa.h, lsspa_subsets_best): v [p + 1] float64,
        masks [p + 1] uint32 (bit j = feature j), found [p + 1] bool (False: no candidate of that size, v is NaN).
        subsets_timing() then speaks of this call."""
        n = self.p + 1
        v, masks, found = np.empty(n), np.empty(n, dtype=np.uint32), np.empty(n, dtype=np.uint8)
        info = C.c_int32()
        self._check(self._lib.lsspa_subsets_best(
            self._h, int(include), N.dptr(v), masks.ctypes.data_as(C.POINTER(C.c_uint32)),
            found.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(info)))
        return v, masks, found.astype(bool), info.value

    SUBSETS_TOP_MAX = 16

    def subsets_top(self, include=0, n_best=10):
        """(v, masks, count, info): the n_best <= 16 best subsets of every size k = 0 .. p among those that contain the
        columns of the mask `include`, best first -- the larger v, on equal values the smaller mask (include/lsspa.h,
        lsspa_subsets_top): v [p + 1][n_best] float64, masks [p + 1][n_best] uint32 (bit j = feature j), count [p + 1]
        int32, the valid ranks of a size (NaN / 0 past them).  Rank 0 is subsets_best's.  subsets_timing() then speaks
        of this call."""
        n, T = self.p + 1, int(n_best)
        v, masks = np.empty((n, max(T, 0))), np.empty((n, max(T, 0)), dtype=np.uint32)
        count = np.empty(n, dtype=np.int32)
        info = C.c_int32()
        self._check(self._lib.lsspa_subsets_top(
            self._h, int(include), T, N.dptr(v), masks.ctypes.data_as(C.POINTER(C.c_uint32)),
            count.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(info)))
        return v, masks, count, info.value

    # ---- bootstrap of the exact attribution (p <= 32; over groups of columns p <= 64) ------
    def boot_load(self, X_train, X_test, y_train, y_test, reg: float, grouped: bool = False):
        """Keep [X | y] of both sides on the device for boot_run (include/lsspa.h, lsspa_boot_load); the loaded problem is
        not touched.  grouped: lsspa_boot_groups_load, which takes p <= 64 for boot_groups_run."""
        dt = np.float32 if (X_train.dtype == np.float32 and X_test.dtype == np.float32) else np.float64
        Xa, Xe = np.ascontiguousarray(X_train, dtype=dt), np.ascontiguousarray(X_test, dtype=dt)
        ya, ye = np.ascontiguousarray(y_train, dtype=dt), np.ascontiguousarray(y_test, dtype=dt)
        n, p = Xa.shape
        self.boot_load_ptr(Xa.ctypes.data, p, ya.ctypes.data, n, Xe.ctypes.data, p, ye.ctypes.data, Xe.shape[0], p, reg,
                           f32=dt == np.float32, location=N.HOST, grouped=grouped)

    def boot_load_ptr(self, X_train_ptr, ld_train, y_train_ptr, n, X_test_ptr, ld_test, y_test_ptr, m_rows, p, reg,
                      f32=False, location=N.DEVICE, grouped: bool = False):
        """Same, from pointers: rows [n][ld_train] and [m_rows][ld_test] of f32 or f64 on the host or the device (e.g.
        torch tensors' data_ptr()), ld >= p."""
        load = self._lib.lsspa_boot_groups_load if grouped else self._lib.lsspa_boot_load
        self._check(load(
            self._h, C.c_void_p(X_train_ptr), int(ld_train), C.c_void_p(y_train_ptr), int(n), C.c_void_p(X_test_ptr),
            int(ld_test), C.c_void_p(y_test_ptr), int(m_rows), int(p), float(reg), N.F32 if f32 else N.F64,
            int(location)))
        self._boot_dims = (int(p), int(n), int(m_rows))

    def boot_free(self):
        self.boot_timing_last = self.boot_timing()      # the data go, the last run's timing stays readable
        self._check(self._lib.lsspa_boot_free(self._h))
        self._boot_dims = None

    def _boot_weights(self, w, R, side):
        if w is None:
            return None
        dims = getattr(self, "_boot_dims", None)
        w = np.ascontiguousarray(w, dtype=np.float64)
        if dims is not None and w.shape != (R, dims[1 + side]):
            raise ValueError(f"weights of the {('training', 'test')[side]} side must have shape ({R}, {dims[1 + side]}), "
                             f"got {w.shape}")
        return w

    def boot_run(self, R: int, seed: int, w_train=None, w_test=None, block: int = 0, first: int = 0):
        """(phi [R][p], r2 [R], info [R]) of replicates first .. first + R - 1 (include/lsspa.h, lsspa_boot_run)."""
        dims = getattr(self, "_boot_dims", None)
        p = dims[0] if dims else 1
        wa, we = self._boot_weights(w_train, R, 0), self._boot_weights(w_test, R, 1)
        phi, r2, info = np.empty((R, p)), np.empty(R), np.zeros(R, dtype=np.int32)
        self._check(self._lib.lsspa_boot_run(self._h, int(R), int(seed) & (2 ** 64 - 1), int(first), N.dptr(wa),
                                             N.dptr(we), int(block), N.dptr(phi), N.dptr(r2), N.iptr(info)))
        return phi, r2, info

    def boot_groups_run(self, labels, R: int, seed: int, w_train=None, w_test=None, block: int = 0, first: int = 0):
        """(phi [R][g], r2 [R], r2_base [R], info [R]) of replicates first .. first + R - 1 over the groups of columns that
        labels names (include/lsspa.h, lsspa_boot_groups_run); the phi of a replicate sum to r2 - r2_base."""
        labels, g = self._labels(labels)
        dims = getattr(self, "_boot_dims", None)
        if dims is not None and len(labels) != dims[0]:
            raise ValueError(f"labels must have length p = {dims[0]}")
        wa, we = self._boot_weights(w_train, R, 0), self._boot_weights(w_test, R, 1)
        phi, r2, base = np.empty((R, max(g, 1))), np.empty(R), np.empty(R)
        info = np.zeros(R, dtype=np.int32)
        self._check(self._lib.lsspa_boot_groups_run(self._h, N.iptr(labels), g, int(R), int(seed) & (2 ** 64 - 1),
                                                    int(first), N.dptr(wa), N.dptr(we), int(block), N.dptr(phi),
                                                    N.dptr(r2), N.dptr(base), N.iptr(info)))
        return phi, r2, base, info

    def boot_interactions_run(self, R: int, seed: int, w_train=None, w_test=None, block: int = 0, first: int = 0):
        """(phi [R][p], I [R][p][p], r2 [R], info [R]) of replicates first .. first + R - 1: boot_run's replicates with the
        raw pairwise interaction index of each (include/lsspa.h, lsspa_boot_interactions_run); phi is boot_run's."""
        dims = getattr(self, "_boot_dims", None)
        p = dims[0] if dims else 1
        wa, we = self._boot_weights(w_train, R, 0), self._boot_weights(w_test, R, 1)
        phi, inter, r2 = np.empty((R, p)), np.empty((R, p, p)), np.empty(R)
        info = np.zeros(R, dtype=np.int32)
        self._check(self._lib.lsspa_boot_interactions_run(self._h, int(R), int(seed) & (2 ** 64 - 1), int(first),
                                                          N.dptr(wa), N.dptr(we), int(block), N.dptr(phi), N.dptr(inter),
                                                          N.dptr(r2), N.iptr(info)))
        return phi, inter, r2, info

    def boot_groups_interactions_run(self, labels, R: int, seed: int, w_train=None, w_test=None, block: int = 0,
                                     first: int = 0):
        """(phi [R][g], I [R][g][g], r2 [R], r2_base [R], info [R]): boot_groups_run's replicates with the raw interaction
        index between the groups of each (include/lsspa.h, lsspa_boot_groups_interactions_run)."""
        labels, g = self._labels(labels)
        dims = getattr(self, "_boot_dims", None)
        if dims is not None and len(labels) != dims[0]:
            raise ValueError(f"labels must have length p = {dims[0]}")
        wa, we = self._boot_weights(w_train, R, 0), self._boot_weights(w_test, R, 1)
        n = max(g, 1)
        phi, inter, r2, base = np.empty((R, n)), np.empty((R, n, n)), np.empty(R), np.empty(R)
        info = np.zeros(R, dtype=np.int32)
        self._check(self._lib.lsspa_boot_groups_interactions_run(
            self._h, N.iptr(labels), g, int(R), int(seed) & (2 ** 64 - 1), int(first), N.dptr(wa), N.dptr(we), int(block),
            N.dptr(phi), N.dptr(inter), N.dptr(r2), N.dptr(base), N.iptr(info)))
        return phi, inter, r2, base, info

    def boot_best_run(self, R: int, seed: int, w_train=None, w_test=None, *, include=0, first: int = 0, block: int = 0):
        """(v [R][p + 1], masks [R][p + 1] uint32, found [R][p + 1] bool, r2 [R], info [R]) of replicates first .. first +
        R - 1: boot_run's replicates, each searched for its best subset of every size as subsets_best does it
        (include/lsspa.h, lsspa_boot_best_run); r2 and info are boot_run's."""
        dims = getattr(self, "_boot_dims", None)
        n = (dims[0] if dims else 1) + 1
        wa, we = self._boot_weights(w_train, R, 0), self._boot_weights(w_test, R, 1)
        v, masks, found = np.empty((R, n)), np.empty((R, n), dtype=np.uint32), np.empty((R, n), dtype=np.uint8)
        r2, info = np.empty(R), np.zeros(R, dtype=np.int32)
        self._check(self._lib.lsspa_boot_best_run(
            self._h, int(R), int(seed) & (2 ** 64 - 1), int(first), N.dptr(wa), N.dptr(we), int(block), int(include),
            N.dptr(v), masks.ctypes.data_as(C.POINTER(C.c_uint32)), found.ctypes.data_as(C.POINTER(C.c_uint8)),
            N.dptr(r2), N.iptr(info)))
        return v, masks, found.astype(bool), r2, info

    debug_boot_best_plan = staticmethod(debug_boot_best_plan)

    def boot_groups_best_run(self, labels, R: int, seed: int, w_train=None, w_test=None, *, first: int = 0,
                             block: int = 0):
        """(u [R][g + 1], masks [R][g + 1] uint32, found [R][g + 1] bool, r2 [R], r2_base [R], info [R]) of replicates
        first .. first + R - 1: boot_groups_run's replicates, each searched for its best set of every number of groups
        as groups_best does it (include/lsspa.h, lsspa_boot_groups_best_run; bit k of a mask = label k); r2, r2_base and
        info are boot_groups_run's."""
        labels, g = self._labels(labels)
        dims = getattr(self, "_boot_dims", None)
        if dims is not None and len(labels) != dims[0]:
            raise ValueError(f"labels must have length p = {dims[0]}")
        wa, we = self._boot_weights(w_train, R, 0), self._boot_weights(w_test, R, 1)
        n = max(g, 0) + 1
        u, masks, found = np.empty((R, n)), np.empty((R, n), dtype=np.uint32), np.empty((R, n), dtype=np.uint8)
        r2, base, info = np.empty(R), np.empty(R), np.zeros(R, dtype=np.int32)
        self._check(self._lib.lsspa_boot_groups_best_run(
            self._h, N.iptr(labels), g, int(R), int(seed) & (2 ** 64 - 1), int(first), N.dptr(wa), N.dptr(we), int(block),
            N.dptr(u), masks.ctypes.data_as(C.POINTER(C.c_uint32)), found.ctypes.data_as(C.POINTER(C.c_uint8)),
            N.dptr(r2), N.dptr(base), N.iptr(info)))
        return u, masks, found.astype(bool), r2, base, info

    debug_boot_groups_best_plan = staticmethod(debug_boot_groups_best_plan)

    def boot_timing(self):
        """Kernel seconds of the last boot_run: counts (or the upload of weights), Gram, enumeration."""
        a, b, c = C.c_double(), C.c_double(), C.c_double()
        self._check(self._lib.lsspa_boot_timing(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return {"counts": a.value / 1e3, "gram": b.value / 1e3, "enumeration": c.value / 1e3}

    def boot_debug_counts(self, seed: int, r: int, side: int):
        out = np.empty(self._boot_dims[1 + side], dtype=np.uint32)
        self._check(self._lib.lsspa_boot_debug_counts(self._h, int(seed) & (2 ** 64 - 1), int(r), int(side),
                                                      out.ctypes.data_as(C.POINTER(C.c_uint32))))
        return out

    def boot_debug_grams(self, R: int, w_train=None, w_test=None):
        """(S_train, S_test [R][p+1][p+1], wsum [R]): the weighted sums before finalise (None: weight 1 on that side)."""
        c = self._boot_dims[0] + 1
        wa, we = self._boot_weights(w_train, R, 0), self._boot_weights(w_test, R, 1)
        Sa, Se, ws = np.empty((R, c, c)), np.empty((R, c, c)), np.empty(R)
        self._check(self._lib.lsspa_boot_debug_grams(self._h, int(R), N.dptr(wa), N.dptr(we), N.dptr(Sa), N.dptr(Se),
                                                     N.dptr(ws)))
        return Sa, Se, ws

    # ---- K-fold cross-validation (p <= 32, 2 <= K <= 32) ---------------------------------------
    CV_MAX_FOLDS = 32

    def cv_load(self, X, y, fold_ids, K: int, reg: float):
        """Keep the rows [X | y] and the K fold problems of the labels fold_ids [N] (0 .. K-1) on the device
        (include/lsspa.h, lsspa_cv_load); the loaded problem and the bootstrap's rows are not touched."""
        dt = np.float32 if X.dtype == np.float32 else np.float64
        Xa, ya = np.ascontiguousarray(X, dtype=dt), np.ascontiguousarray(y, dtype=dt)
        n, p = Xa.shape
        self.cv_load_ptr(Xa.ctypes.data, p, ya.ctypes.data, n, p, fold_ids, K, reg, f32=dt == np.float32,
                         location=N.HOST)

    def cv_load_ptr(self, X_ptr, ld, y_ptr, n, p, fold_ids, K, reg, f32=False, location=N.DEVICE):
        """Same, from pointers: rows [n][ld] of f32 or f64 on the host or the device, ld >= p; fold_ids a host array."""
        fid = np.ascontiguousarray(fold_ids, dtype=np.int32)
        if fid.shape != (int(n),):
            raise ValueError(f"fold_ids must have shape ({int(n)},), got {fid.shape}")
        self._check(self._lib.lsspa_cv_load(
            self._h, C.c_void_p(X_ptr), int(ld), C.c_void_p(y_ptr), int(n), int(p), N.iptr(fid), int(K), float(reg),
            N.F32 if f32 else N.F64, int(location)))
        self._cv_dims = (int(p), int(K), int(n))

    def cv_free(self):
        self._check(self._lib.lsspa_cv_free(self._h))
        self._cv_dims = None

    def _cv_pk(self):
        dims = getattr(self, "_cv_dims", None)
        return (dims[0], dims[1]) if dims else (1, 2)

    def cv_shapley(self):
        """(phi [p], phi_fold [K][p], r2_fold [K], info [K]): the attribution of the cross-validated R^2, the folds'
        attributions it is the sum of, each fold's share of the R^2 of the full model and the folds' info words
        (include/lsspa.h, lsspa_cv_shapley)."""
        p, K = self._cv_pk()
        phi, fold, r2, info = np.empty(p), np.empty((K, p)), np.empty(K), np.zeros(K, dtype=np.int32)
        self._check(self._lib.lsspa_cv_shapley(self._h, N.dptr(phi), N.dptr(fold), N.dptr(r2), N.iptr(info)))
        return phi, fold, r2, info

    def cv_best(self, include=0, steps: int = 0):
        """(v [p + 1], masks [p + 1] uint32, found [p + 1] bool, v_fold [p + 1][K], info [K]): the best subset of every
        size by the cross-validated value (include/lsspa.h, lsspa_cv_best).  steps > 0: that many steps of a unit per
        launch (test hook; the result does not depend on it)."""
        p, K = self._cv_pk()
        n = p + 1
        v, masks, found = np.empty(n), np.empty(n, dtype=np.uint32), np.empty(n, dtype=np.uint8)
        v_fold, info = np.empty((n, K)), np.zeros(K, dtype=np.int32)
        self._check(self._lib.lsspa_cv_best(
            self._h, int(include), int(steps), N.dptr(v), masks.ctypes.data_as(C.POINTER(C.c_uint32)),
            found.ctypes.data_as(C.POINTER(C.c_uint8)), N.dptr(v_fold), N.iptr(info)))
        return v, masks, found.astype(bool), v_fold, info

    def cv_top(self, include=0, n_best=10, steps: int = 0):
        """(v [p + 1][n_best], masks [p + 1][n_best] uint32, count [p + 1] int32, v_fold [p + 1][n_best][K], info [K]):
        the n_best <= 16 best subsets of every size by the cross-validated value, best first -- the larger value, on
        equal values the smaller mask (include/lsspa.h, lsspa_cv_top); NaN / 0 past count.  Rank 0 is cv_best's.
        steps as in cv_best.  cv_timing() then speaks of this call."""
        p, K = self._cv_pk()
        n, T = p + 1, int(n_best)
        v, masks = np.empty((n, max(T, 0))), np.empty((n, max(T, 0)), dtype=np.uint32)
        count = np.empty(n, dtype=np.int32)
        v_fold, info = np.empty((n, max(T, 0), K)), np.zeros(K, dtype=np.int32)
        self._check(self._lib.lsspa_cv_top(
            self._h, int(include), T, int(steps), N.dptr(v), masks.ctypes.data_as(C.POINTER(C.c_uint32)),
            count.ctypes.data_as(C.POINTER(C.c_int32)), N.dptr(v_fold), N.iptr(info)))
        return v, masks, count, v_fold, info

    def cv_timing(self):
        """Kernel seconds of the load's Gram side and of the last enumeration, its longest launch and the launches."""
        a, b, c, n = C.c_double(), C.c_double(), C.c_double(), C.c_int64()
        self._check(self._lib.lsspa_cv_timing(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(n)))
        return {"gram": a.value / 1e3, "enumeration": b.value / 1e3, "max_launch": c.value / 1e3, "launches": n.value}

    def cv_get_problem(self, f: int):
        """Test hook: (G, g, H, h, inv_yy) of fold problem f as the device computed it."""
        p, _ = self._cv_pk()
        G, g, H, h, yy = np.empty((p, p)), np.empty(p), np.empty((p, p)), np.empty(p), C.c_double()
        self._check(self._lib.lsspa_cv_get_problem(self._h, int(f), N.dptr(G), N.dptr(g), N.dptr(H), N.dptr(h),
                                                   C.byref(yy)))
        return G, g, H, h, yy.value

    def debug_cv_values(self, masks, folds: bool = True):
        """Test hook: (v [n], v_fold [n][K] or None) of the subsets `masks` (bit j = feature j) by cv_best's own device
        code (include/lsspa.h, lsspa_debug_cv_values)."""
        _, K = self._cv_pk()
        masks = np.ascontiguousarray(masks, dtype=np.uint64)
        v = np.empty(len(masks))
        v_fold = np.empty((len(masks), K)) if folds else None
        self._check(self._lib.lsspa_debug_cv_values(self._h, masks.ctypes.data_as(C.POINTER(C.c_uint64)), len(masks),
                                                    N.dptr(v), N.dptr(v_fold)))
        return v, v_fold

    debug_cv_plan = staticmethod(debug_cv_plan)
    debug_cv_top_plan = staticmethod(debug_cv_top_plan)

    # ---- ... over groups of columns (g <= 32 groups of p <= 64 columns) ----
    def cv_groups_load(self, X, y, fold_ids, K: int, reg: float):
        """cv_load with the limit p <= 64 (include/lsspa.h, lsspa_cv_groups_load): the same store, either load replaces
        the other; after p <= 32 both families of calls work."""
        dt = np.float32 if X.dtype == np.float32 else np.float64
        Xa, ya = np.ascontiguousarray(X, dtype=dt), np.ascontiguousarray(y, dtype=dt)
        n, p = Xa.shape
        fid = np.ascontiguousarray(fold_ids, dtype=np.int32)
        if fid.shape != (int(n),):
            raise ValueError(f"fold_ids must have shape ({int(n)},), got {fid.shape}")
        self._check(self._lib.lsspa_cv_groups_load(
            self._h, C.c_void_p(Xa.ctypes.data), int(p), C.c_void_p(ya.ctypes.data), int(n), int(p), N.iptr(fid), int(K),
            float(reg), N.F32 if dt == np.float32 else N.F64, N.HOST))
        self._cv_dims = (int(p), int(K), int(n))

    def _cv_labels(self, labels):
        labels, g = self._labels(labels)
        p, K = self._cv_pk()
        if len(labels) != p:
            raise ValueError(f"labels must have length p = {p}")
        return labels, g, K

    def cv_groups_shapley(self, labels):
        """(phi [g], phi_fold [K][g], r2_fold [K], base_fold [K], info [K]): the attribution of the cross-validated R^2
        to the groups of `labels`, the folds' attributions it is the sum of, each fold's value of all groups and of the
        baseline alone, and the folds' info words (include/lsspa.h, lsspa_cv_groups_shapley)."""
        labels, g, K = self._cv_labels(labels)
        n = max(g, 1)
        phi, fold, r2, base = np.empty(n), np.empty((K, n)), np.empty(K), np.empty(K)
        info = np.zeros(K, dtype=np.int32)
        self._check(self._lib.lsspa_cv_groups_shapley(self._h, N.iptr(labels), g, N.dptr(phi), N.dptr(fold), N.dptr(r2),
                                                      N.dptr(base), N.iptr(info)))
        return phi, fold, r2, base, info

    def cv_groups_best(self, labels, steps: int = 0):
        """(u [g + 1], masks [g + 1] uint32 (bit k = group k), found [g + 1] bool, u_fold [g + 1][K], info [K]): the best
        set of groups of every size 0 .. g by the cross-validated value (include/lsspa.h, lsspa_cv_groups_best).
        steps > 0: that many steps of a unit per launch (test hook; the result does not depend on it)."""
        labels, g, K = self._cv_labels(labels)
        n = max(g, 0) + 1
        u, masks, found = np.empty(n), np.empty(n, dtype=np.uint32), np.empty(n, dtype=np.uint8)
        u_fold, info = np.empty((n, K)), np.zeros(K, dtype=np.int32)
        self._check(self._lib.lsspa_cv_groups_best(
            self._h, N.iptr(labels), g, int(steps), N.dptr(u), masks.ctypes.data_as(C.POINTER(C.c_uint32)),
            found.ctypes.data_as(C.POINTER(C.c_uint8)), N.dptr(u_fold), N.iptr(info)))
        return u, masks, found.astype(bool), u_fold, info

    def debug_cv_group_values(self, labels, masks, folds: bool = True):
        """Test hook: (u [n], u_fold [n][K] or None) of the sets of groups `masks` (bit k = group k) by cv_groups_best's
        own device code (include/lsspa.h, lsspa_debug_cv_group_values)."""
        labels, g, K = self._cv_labels(labels)
        masks = np.ascontiguousarray(masks, dtype=np.uint64)
        u = np.empty(len(masks))
        u_fold = np.empty((len(masks), K)) if folds else None
        self._check(self._lib.lsspa_debug_cv_group_values(
            self._h, N.iptr(labels), g, masks.ctypes.data_as(C.POINTER(C.c_uint64)), len(masks), N.dptr(u),
            N.dptr(u_fold)))
        return u, u_fold

    def cv_groups_top(self, labels, n_best=10, steps: int = 0):
        """(u [g + 1][n_best], masks [g + 1][n_best] uint32 (bit k = group k), count [g + 1] int32,
        u_fold [g + 1][n_best][K], info [K]): the n_best <= 16 best sets of groups of every size 0 .. g by the
        cross-validated value, best first -- the larger value, on equal values the smaller mask (include/lsspa.h,
        lsspa_cv_groups_top); NaN / 0 past count.  Rank 0 is cv_groups_best's.  steps as in cv_groups_best.
        cv_timing() then speaks of this call."""
        labels, g, K = self._cv_labels(labels)
        n, T = max(g, 0) + 1, int(n_best)
        u, masks = np.empty((n, max(T, 0))), np.empty((n, max(T, 0)), dtype=np.uint32)
        count = np.empty(n, dtype=np.int32)
        u_fold, info = np.empty((n, max(T, 0), K)), np.zeros(K, dtype=np.int32)
        self._check(self._lib.lsspa_cv_groups_top(
            self._h, N.iptr(labels), g, T, int(steps), N.dptr(u), masks.ctypes.data_as(C.POINTER(C.c_uint32)),
            count.ctypes.data_as(C.POINTER(C.c_int32)), N.dptr(u_fold), N.iptr(info)))
        return u, masks, count, u_fold, info

    debug_cv_groups_plan = staticmethod(debug_cv_groups_plan)
    debug_cv_groups_top_plan = staticmethod(debug_cv_groups_top_plan)

    # ---- ... the ridge path: L ridge values on one load ----
    def cv_path_shapley(self, regs, block: int = 0):
        """(phi [L][p], phi_fold [L][K][p], r2_fold [L][K], info [L][K]): row l is cv_shapley() after a load with
        reg = regs[l], bit for bit (include/lsspa.h, lsspa_cv_path_shapley).  block > 0: that many ridge values a block
        (test hook; the result does not depend on it).  cv_timing() then speaks of this call."""
        p, K = self._cv_pk()
        regs = np.ascontiguousarray(regs, dtype=np.float64)
        L = len(regs)
        phi, fold, r2 = np.empty((L, p)), np.empty((L, K, p)), np.empty((L, K))
        info = np.zeros((L, K), dtype=np.int32)
        self._check(self._lib.lsspa_cv_path_shapley(self._h, N.dptr(regs), L, int(block), N.dptr(phi), N.dptr(fold),
                                                    N.dptr(r2), N.iptr(info)))
        return phi, fold, r2, info

    def cv_path_groups_shapley(self, labels, regs, block: int = 0):
        """(phi [L][g], phi_fold [L][K][g], r2_fold [L][K], base_fold [L][K], info [L][K]): row l is
        cv_groups_shapley(labels) after a load with reg = regs[l], bit for bit (include/lsspa.h,
        lsspa_cv_path_groups_shapley).  block as in cv_path_shapley."""
        labels, g, K = self._cv_labels(labels)
        n = max(g, 1)
        regs = np.ascontiguousarray(regs, dtype=np.float64)
        L = len(regs)
        phi, fold, r2, base = np.empty((L, n)), np.empty((L, K, n)), np.empty((L, K)), np.empty((L, K))
        info = np.zeros((L, K), dtype=np.int32)
        self._check(self._lib.lsspa_cv_path_groups_shapley(
            self._h, N.iptr(labels), g, N.dptr(regs), L, int(block), N.dptr(phi), N.dptr(fold), N.dptr(r2),
            N.dptr(base), N.iptr(info)))
        return phi, fold, r2, base, info

    debug_cv_path_plan = staticmethod(debug_cv_path_plan)
    debug_cv_path_groups_plan = staticmethod(debug_cv_path_groups_plan)

    # ---- exact attribution of many responses at once (p <= 32; over groups g <= 32, p <= 64) ----
    MULTI_RB = 8      # responses a wave carries per pass (csrc/kernels.h)

    def multi_load(self, X_train, X_test, Y_train, Y_test, reg: float):
        """One Gram pass per side over [X | Y] (Y_train [N][m], Y_test [M][m]) for multi_shapley (include/lsspa.h,
        lsspa_multi_load); the loaded problem is not touched."""
        dt = np.float32 if (X_train.dtype == np.float32 and X_test.dtype == np.float32) else np.float64
        Xa, Xe = np.ascontiguousarray(X_train, dtype=dt), np.ascontiguousarray(X_test, dtype=dt)
        Ya, Ye = np.ascontiguousarray(Y_train, dtype=dt), np.ascontiguousarray(Y_test, dtype=dt)
        n, p = Xa.shape
        m = Ya.shape[1]
        self.multi_load_ptr(Xa.ctypes.data, p, Ya.ctypes.data, m, n, Xe.ctypes.data, p, Ye.ctypes.data, m,
                            Xe.shape[0], p, m, reg, f32=dt == np.float32, location=N.HOST)

    def multi_load_ptr(self, X_train_ptr, ld_train, Y_train_ptr, ldy_train, n, X_test_ptr, ld_test, Y_test_ptr,
                       ldy_test, m_rows, p, m, reg, f32=False, location=N.DEVICE):
        """Same, from pointers: X [n][ld_train] and Y [n][ldy_train] (the test side alike) of f32 or f64 on the host or
        the device, ld >= p and ldy >= m."""
        self._check(self._lib.lsspa_multi_load(
            self._h, C.c_void_p(X_train_ptr), int(ld_train), C.c_void_p(Y_train_ptr), int(ldy_train), int(n),
            C.c_void_p(X_test_ptr), int(ld_test), C.c_void_p(Y_test_ptr), int(ldy_test), int(m_rows), int(p), int(m),
            float(reg), N.F32 if f32 else N.F64, int(location)))
        self._multi_dims = (int(p), int(m))

    def multi_load_reduced(self, G, g, H, h, yy):
        """The same from the Gram form: G, H [p][p], g, h [m][p], yy [m] (lsspa_multi_set_reduced)."""
        G, H = (np.ascontiguousarray(a, dtype=np.float64) for a in (G, H))
        g, h = (np.ascontiguousarray(np.atleast_2d(a), dtype=np.float64) for a in (g, h))
        yy = np.ascontiguousarray(np.atleast_1d(yy), dtype=np.float64)
        p, m = G.shape[0], g.shape[0]
        if G.shape != (p, p) or H.shape != (p, p) or g.shape != (m, p) or h.shape != (m, p) or yy.shape != (m,):
            raise ValueError("multi_load_reduced takes G, H [p][p], g, h [m][p] and yy [m]")
        self._check(self._lib.lsspa_multi_set_reduced(self._h, p, m, N.dptr(G), N.dptr(g), N.dptr(H), N.dptr(h),
                                                      N.dptr(yy)))
        self._multi_dims = (p, m)

    def multi_shapley(self, first: int = 0, count=None, block: int = 0):
        """(phi [count][p], info) of responses first .. first + count - 1 (all from `first` on by default); block:
        responses enumerated together, 0 = as many as the budget holds (include/lsspa.h, lsspa_multi_shapley)."""
        p, m = getattr(self, "_multi_dims", None) or (1, 0)
        count = m - int(first) if count is None else int(count)
        phi = np.empty((max(count, 0), p))
        info = C.c_int32()
        self._check(self._lib.lsspa_multi_shapley(self._h, int(first), count, int(block), N.dptr(phi), C.byref(info)))
        return phi, info.value

    def multi_gram(self):
        """(G, g [m][p], H, h [m][p], yy [m]) of the loaded responses."""
        p, m = self._multi_dims
        G, g, H, h, yy = np.empty((p, p)), np.empty((m, p)), np.empty((p, p)), np.empty((m, p)), np.empty(m)
        self._check(self._lib.lsspa_multi_get_gram(self._h, N.dptr(G), N.dptr(g), N.dptr(H), N.dptr(h), N.dptr(yy)))
        return G, g, H, h, yy

    def multi_values(self, masks):
        """Test hook: v [n][m], v_r(S) of every mask (bit j = feature j) by the enumeration's own device code."""
        masks = np.ascontiguousarray(masks, dtype=np.uint64).ravel()
        out = np.empty((len(masks), self._multi_dims[1]))
        self._check(self._lib.lsspa_debug_multi_values(self._h, masks.ctypes.data_as(C.POINTER(C.c_uint64)), len(masks),
                                                       N.dptr(out)))
        return out

    def _multi_labels(self, labels):
        labels, g = self._labels(labels)
        dims = getattr(self, "_multi_dims", None)
        if dims is not None and len(labels) != dims[0]:
            raise ValueError(f"labels must have length p = {dims[0]}")
        return labels, g

    def multi_groups_shapley(self, labels, first: int = 0, count=None, block: int = 0):
        """(phi [count][g], info): multi_shapley over the groups of columns that labels names (one label per column: -1
        the baseline, 0 .. g-1 the groups; include/lsspa.h, lsspa_multi_groups_shapley).  The library checks the
        labels."""
        labels, g = self._multi_labels(labels)
        m = (getattr(self, "_multi_dims", None) or (1, 0))[1]
        count = m - int(first) if count is None else int(count)
        phi = np.empty((max(count, 0), max(g, 1)))
        info = C.c_int32()
        self._check(self._lib.lsspa_multi_groups_shapley(self._h, N.iptr(labels), g, int(first), count, int(block),
                                                         N.dptr(phi), C.byref(info)))
        return phi, info.value

    def multi_group_values(self, labels, masks):
        """Test hook: u [n][m], u_r(S) of every mask (bit k = group k) by the grouped enumeration's own device code."""
        labels, g = self._multi_labels(labels)
        masks = np.ascontiguousarray(masks, dtype=np.uint64).ravel()
        out = np.empty((len(masks), (getattr(self, "_multi_dims", None) or (1, 0))[1]))
        self._check(self._lib.lsspa_debug_multi_group_values(self._h, N.iptr(labels), g,
                                                             masks.ctypes.data_as(C.POINTER(C.c_uint64)), len(masks),
                                                             N.dptr(out)))
        return out

    def multi_timing(self):
        """Device seconds of the last multi_load's Gram passes and of the last multi_shapley's (or
        multi_groups_shapley's) enumeration, its longest launch, and the number of launches."""
        a, b, c, n = C.c_double(), C.c_double(), C.c_double(), C.c_int64()
        self._check(self._lib.lsspa_multi_timing(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(n)))
        return {"gram": a.value / 1e3, "enumeration": b.value / 1e3, "max_launch": c.value / 1e3, "launches": n.value}

    def multi_free(self):
        self._check(self._lib.lsspa_multi_free(self._h))
        self._multi_dims = None

    # ---- permutation test of the exact attribution (p <= 32; over groups g <= 32, p <= 64) ----
    def perm_load(self, X_train, X_test, y_train, y_test, reg: float):
        """Keep X and y of both sides on the device and reduce [X | y] once per side for perm_run / perm_observed
        (include/lsspa.h, lsspa_perm_load); the loaded problem and every other call's state are not touched."""
        dt = np.float32 if (X_train.dtype == np.float32 and X_test.dtype == np.float32) else np.float64
        Xa, Xe = np.ascontiguousarray(X_train, dtype=dt), np.ascontiguousarray(X_test, dtype=dt)
        ya, ye = np.ascontiguousarray(y_train, dtype=dt), np.ascontiguousarray(y_test, dtype=dt)
        n, p = Xa.shape
        self.perm_load_ptr(Xa.ctypes.data, p, ya.ctypes.data, n, Xe.ctypes.data, p, ye.ctypes.data, Xe.shape[0], p, reg,
                           f32=dt == np.float32, location=N.HOST)

    def perm_load_ptr(self, X_train_ptr, ld_train, y_train_ptr, n, X_test_ptr, ld_test, y_test_ptr, m_rows, p, reg,
                      f32=False, location=N.DEVICE):
        """Same, from pointers: rows [n][ld_train] and [m_rows][ld_test] of f32 or f64 on the host or the device,
        ld >= p."""
        self._check(self._lib.lsspa_perm_load(
            self._h, C.c_void_p(X_train_ptr), int(ld_train), C.c_void_p(y_train_ptr), int(n), C.c_void_p(X_test_ptr),
            int(ld_test), C.c_void_p(y_test_ptr), int(m_rows), int(p), float(reg), N.F32 if f32 else N.F64,
            int(location)))
        self._perm_dims = (int(p), int(n), int(m_rows))

    def _perm_labels(self, labels):
        p = (getattr(self, "_perm_dims", None) or (1,))[0]
        if labels is None:
            return None, 0, p
        labels, g = self._labels(labels)
        if len(labels) != p:
            raise ValueError(f"labels must have length p = {p}")
        return labels, g, max(g, 1)

    def perm_run(self, R: int, seed: int, labels=None, first: int = 0, sides: int = 3, block: int = 0):
        """(phi [R][d], gperm [R][p], hperm [R][p], info) of replicates first .. first + R - 1 (include/lsspa.h,
        lsspa_perm_run): d = p, or the g groups of labels; sides: bit 0 permutes the training side, bit 1 the test side."""
        labels, g, d = self._perm_labels(labels)
        p = (getattr(self, "_perm_dims", None) or (1,))[0]
        R = int(R)
        phi, gp, hp = np.empty((max(R, 0), d)), np.empty((max(R, 0), p)), np.empty((max(R, 0), p))
        info = C.c_int32()
        self._check(self._lib.lsspa_perm_run(self._h, N.iptr(labels), g, R, int(seed) & (2 ** 64 - 1), int(first),
                                             int(sides), int(block), N.dptr(phi), N.dptr(gp), N.dptr(hp), C.byref(info)))
        return phi, gp, hp, info.value

    def perm_observed(self, labels=None):
        """(phi [d], info): the identity permutation through perm_run's enumeration (lsspa_perm_observed)."""
        labels, g, d = self._perm_labels(labels)
        phi = np.empty(d)
        info = C.c_int32()
        self._check(self._lib.lsspa_perm_observed(self._h, N.iptr(labels), g, N.dptr(phi), C.byref(info)))
        return phi, info.value

    def perm_gram(self):
        """(G, g [p], H, h [p], yy) of the load."""
        p = self._perm_dims[0]
        G, g, H, h, yy = np.empty((p, p)), np.empty(p), np.empty((p, p)), np.empty(p), np.empty(1)
        self._check(self._lib.lsspa_perm_get_gram(self._h, N.dptr(G), N.dptr(g), N.dptr(H), N.dptr(h), N.dptr(yy)))
        return G, g, H, h, float(yy[0])

    def perm_timing(self):
        """Seconds of the last perm_run: drawing and uploading the index rows (host threads of the library), the X^T y
        kernels and the enumeration (device)."""
        a, b, c, d = C.c_double(), C.c_double(), C.c_double(), C.c_double()
        self._check(self._lib.lsspa_perm_timing(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return {"draw": a.value / 1e3, "upload": b.value / 1e3, "xty": c.value / 1e3, "enumeration": d.value / 1e3}

    def perm_free(self):
        self.perm_timing_last = self.perm_timing()      # the data go, the last run's timing stays readable
        self._check(self._lib.lsspa_perm_free(self._h))
        self._perm_dims = None

    # ---- what the sampled families (fam: multi_lift, cv_lift, boot_lift) share: player map, sample dimension, perms ----
    def _lift_players(self, fam, labels, g):
        """lsspa_<fam>_set_players: labels (g: the largest + 1 unless given), or None and 0 to clear; remembers g."""
        if labels is not None:
            labels = np.ascontiguousarray(labels, dtype=np.int32)
            g = int(labels.max()) + 1 if g is None else int(g)
        self._check(getattr(self._lib, f"lsspa_{fam}_set_players")(self._h, N.iptr(labels), g))
        setattr(self, f"_{fam}_g", g)

    def _lift_sd(self, fam, unloaded):
        """(dimension of a sample: g with a player map, else p; the second of the family's dimensions)"""
        dims = getattr(self, f"_{fam}_dims", None) or unloaded
        return (getattr(self, f"_{fam}_g", 0) or dims[0]), dims[1]

    def _lift_perms(self, fam, perms, rows="B"):
        """(perms as int32, loaded): loaded, perms must be [rows][d]; before, the library says what comes first."""
        perms = np.ascontiguousarray(perms, dtype=np.int32)
        loaded = getattr(self, f"_{fam}_dims", None) is not None
        d = self._lift_sd(fam, (1, 0))[0]
        if loaded and (perms.ndim != 2 or perms.shape[1] != d):
            raise ValueError(f"perms must be [{rows}][{'g' if getattr(self, f'_{fam}_g', 0) else 'p'} = {d}]")
        return perms, loaded

    # ---- sampled attribution of many responses on one design matrix (p <= 104) ----
    MULTI_LIFT_MAX_P = 104     # include/lsspa.h, LSSPA_MULTI_LIFT_MAX_P

    def multi_lift_load(self, X_train, X_test, Y_train, Y_test, reg: float):
        """One Gram pass per side over [X | Y] (Y_train [N][m], Y_test [M][m]) for multi_lift_batch (include/lsspa.h,
        lsspa_multi_lift_load); the loaded problem and the state of multi_load are not touched."""
        dt = np.float32 if (X_train.dtype == np.float32 and X_test.dtype == np.float32) else np.float64
        Xa, Xe = np.ascontiguousarray(X_train, dtype=dt), np.ascontiguousarray(X_test, dtype=dt)
        Ya, Ye = np.ascontiguousarray(Y_train, dtype=dt), np.ascontiguousarray(Y_test, dtype=dt)
        n, p = Xa.shape
        m = Ya.shape[1]
        self.multi_lift_load_ptr(Xa.ctypes.data, p, Ya.ctypes.data, m, n, Xe.ctypes.data, p, Ye.ctypes.data, m,
                                 Xe.shape[0], p, m, reg, f32=dt == np.float32, location=N.HOST)

    def multi_lift_load_ptr(self, X_train_ptr, ld_train, Y_train_ptr, ldy_train, n, X_test_ptr, ld_test, Y_test_ptr,
                            ldy_test, m_rows, p, m, reg, f32=False, location=N.DEVICE):
        """Same, from pointers: X [n][ld_train] and Y [n][ldy_train] (the test side alike) of f32 or f64 on the host or
        the device, ld >= p and ldy >= m."""
        self._check(self._lib.lsspa_multi_lift_load(
            self._h, C.c_void_p(X_train_ptr), int(ld_train), C.c_void_p(Y_train_ptr), int(ldy_train), int(n),
            C.c_void_p(X_test_ptr), int(ld_test), C.c_void_p(Y_test_ptr), int(ldy_test), int(m_rows), int(p), int(m),
            float(reg), N.F32 if f32 else N.F64, int(location)))
        self._multi_lift_dims, self._multi_lift_g = (int(p), int(m)), 0

    def multi_lift_load_reduced(self, G, g, H, h, yy):
        """The same from the Gram form: G, H [p][p], g, h [m][p], yy [m] (lsspa_multi_lift_set_reduced)."""
        G, H = (np.ascontiguousarray(a, dtype=np.float64) for a in (G, H))
        g, h = (np.ascontiguousarray(np.atleast_2d(a), dtype=np.float64) for a in (g, h))
        yy = np.ascontiguousarray(np.atleast_1d(yy), dtype=np.float64)
        p, m = G.shape[0], g.shape[0]
        if G.shape != (p, p) or H.shape != (p, p) or g.shape != (m, p) or h.shape != (m, p) or yy.shape != (m,):
            raise ValueError("multi_lift_load_reduced takes G, H [p][p], g, h [m][p] and yy [m]")
        self._check(self._lib.lsspa_multi_lift_set_reduced(self._h, p, m, N.dptr(G), N.dptr(g), N.dptr(H), N.dptr(h),
                                                           N.dptr(yy)))
        self._multi_lift_dims, self._multi_lift_g = (p, m), 0

    def multi_lift_set_players(self, labels, g=None):
        """Groups of columns as the players of multi_lift_batch: one label per column, -1 the baseline, 0 .. g-1 the
        groups (g: the largest label + 1 unless given).  From now on multi_lift_batch takes [B][g] orderings of the
        groups and multi_lift_get returns [m][g]; the statistics start over (include/lsspa.h,
        lsspa_multi_lift_set_players).  The library checks the labels."""
        labels, g_seen = self._labels(labels)
        g = g_seen if g is None else int(g)
        dims = getattr(self, "_multi_lift_dims", None)
        if dims is not None and len(labels) != dims[0]:
            raise ValueError(f"labels must have length p = {dims[0]}")
        self._lift_players("multi_lift", labels, g)

    def multi_lift_clear_players(self):
        self._lift_players("multi_lift", None, 0)

    def _multi_lift_sd(self):
        """(dimension of a sample: g with a player map, else p; m)"""
        return self._lift_sd("multi_lift", (1, 1))

    def multi_lift_batch(self, perms, antithetical: bool, want_lifts: bool = False, accumulate: bool = True):
        """The lift vectors of every response for the orderings perms [B][p] (with antithetical a sample is the mean of
        an ordering and its reverse), folded into the running statistics if accumulate; lifts [B][m][p] if want_lifts
        (include/lsspa.h, lsspa_multi_lift_batch).  With a player map (multi_lift_set_players) perms is [B][g] and the
        lifts [B][m][g].  The library checks the orderings."""
        (p, m), (perms, loaded) = self._multi_lift_sd(), self._lift_perms("multi_lift", perms)
        want_lifts = want_lifts and loaded
        out = np.empty((perms.shape[0], m, p)) if want_lifts else None
        self._check(self._lib.lsspa_multi_lift_batch(self._h, N.iptr(perms) if perms.size else None, perms.shape[0],
                                                     int(bool(antithetical)), N.dptr(out) if want_lifts else None,
                                                     int(bool(accumulate))))
        return out

    def multi_lift_get(self):
        """(n, mean [m][p], M2 [m][p]) of the samples folded in so far ([m][g] with a player map)."""
        p, m = self._multi_lift_sd()
        n, mean, m2 = C.c_int64(), np.empty((m, p)), np.empty((m, p))
        self._check(self._lib.lsspa_multi_lift_get(self._h, C.byref(n), N.dptr(mean), N.dptr(m2)))
        return n.value, mean, m2

    def multi_lift_reset(self):
        self._check(self._lib.lsspa_multi_lift_reset(self._h))

    def multi_lift_gram(self):
        """(G, g [m][p], H, h [m][p], yy [m]) of the loaded responses."""
        p, m = getattr(self, "_multi_lift_dims", None) or (1, 1)
        G, g, H, h, yy = np.empty((p, p)), np.empty((m, p)), np.empty((p, p)), np.empty((m, p)), np.empty(m)
        self._check(self._lib.lsspa_multi_lift_get_gram(self._h, N.dptr(G), N.dptr(g), N.dptr(H), N.dptr(h),
                                                        N.dptr(yy)))
        return G, g, H, h, yy

    def multi_lift_info(self) -> int:
        info = C.c_int32()
        self._check(self._lib.lsspa_multi_lift_info(self._h, C.byref(info)))
        return info.value

    def multi_lift_timing(self):
        """Device seconds of the last multi_lift_load's Gram passes, of the last batch's lift launches and of its
        statistics launches."""
        a, b, c = C.c_double(), C.c_double(), C.c_double()
        self._check(self._lib.lsspa_multi_lift_timing(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return {"gram": a.value / 1e3, "batch": b.value / 1e3, "stats": c.value / 1e3}

    def multi_lift_free(self):
        self._check(self._lib.lsspa_multi_lift_free(self._h))
        self._multi_lift_dims, self._multi_lift_g = None, 0

    # ---- sampled attribution of the K-fold cross-validated R^2 (p <= 127, 2 <= K <= 32) ----------
    CV_LIFT_MAX_P = 127

    def cv_lift_load(self, X, y, fold_ids, K: int, reg: float):
        """The K fold problems of the labels fold_ids [N] (0 .. K-1) for cv_lift_batch (include/lsspa.h,
        lsspa_cv_lift_load); the loaded problem and the state of cv_load and multi_lift_load are not touched."""
        dt = np.float32 if X.dtype == np.float32 else np.float64
        Xa, ya = np.ascontiguousarray(X, dtype=dt), np.ascontiguousarray(y, dtype=dt)
        n, p = Xa.shape
        fid = np.ascontiguousarray(fold_ids, dtype=np.int32)
        if fid.shape != (int(n),):
            raise ValueError(f"fold_ids must have shape ({int(n)},), got {fid.shape}")
        self._check(self._lib.lsspa_cv_lift_load(
            self._h, C.c_void_p(Xa.ctypes.data), int(p), C.c_void_p(ya.ctypes.data), int(n), int(p), N.iptr(fid), int(K),
            float(reg), N.F32 if dt == np.float32 else N.F64, N.HOST))
        self._cv_lift_dims, self._cv_lift_g = (int(p), int(K)), 0

    def cv_lift_set_players(self, labels, g=None):
        """Groups of columns as the players of cv_lift_batch, as multi_lift_set_players names them (include/lsspa.h,
        lsspa_cv_lift_set_players): perms are then [B][g], the lifts and the statistics in dimension g.  The library
        checks the labels."""
        self._lift_players("cv_lift", np.asarray(labels), g)

    def cv_lift_clear_players(self):
        self._lift_players("cv_lift", None, 0)

    def _cv_lift_sd(self):
        """(dimension of a sample: g with a player map, else p; K)"""
        return self._lift_sd("cv_lift", (1, 2))

    def cv_lift_batch(self, perms, antithetical: bool, want_lifts: bool = False, accumulate: bool = True):
        """One ordering through the K fold problems, for every row of perms [B][d] (with antithetical a sample is an
        ordering and its reverse), folded into the running statistics if accumulate; with want_lifts
        (fold_lifts [B][K][d], lifts [B][d]), the folds' lift vectors and their ascending sum (include/lsspa.h,
        lsspa_cv_lift_batch).  The library checks the orderings."""
        (d, K), (perms, loaded) = self._cv_lift_sd(), self._lift_perms("cv_lift", perms)
        want_lifts = want_lifts and loaded
        B = perms.shape[0] if perms.ndim == 2 else 0
        fold = np.empty((B, K, d)) if want_lifts else None
        tot = np.empty((B, d)) if want_lifts else None
        self._check(self._lib.lsspa_cv_lift_batch(self._h, N.iptr(perms) if perms.size else None, B,
                                                  int(bool(antithetical)), N.dptr(fold) if want_lifts else None,
                                                  N.dptr(tot) if want_lifts else None, int(bool(accumulate))))
        return (fold, tot) if want_lifts else None

    def cv_lift_get(self):
        """(n, mean [K + 1][d], M2 [K + 1][d]) of the samples folded in so far: rows 0 .. K-1 the folds, row K the sum."""
        d, K = self._cv_lift_sd()
        n, mean, m2 = C.c_int64(), np.empty((K + 1, d)), np.empty((K + 1, d))
        self._check(self._lib.lsspa_cv_lift_get(self._h, C.byref(n), N.dptr(mean), N.dptr(m2)))
        return n.value, mean, m2

    def cv_lift_reset(self):
        self._check(self._lib.lsspa_cv_lift_reset(self._h))

    def cv_lift_problem(self, f: int):
        """(G, g, H, h, inv_yy) of fold problem f as the device computed it."""
        p, _ = getattr(self, "_cv_lift_dims", None) or (1, 2)
        G, g, H, h, yy = np.empty((p, p)), np.empty(p), np.empty((p, p)), np.empty(p), C.c_double()
        self._check(self._lib.lsspa_cv_lift_get_problem(self._h, int(f), N.dptr(G), N.dptr(g), N.dptr(H), N.dptr(h),
                                                        C.byref(yy)))
        return G, g, H, h, yy.value

    def cv_lift_info(self):
        """info [K]: bit 1 of word f: a pivot of fold problem f failed in some ordering since the last reset."""
        _, K = self._cv_lift_sd()
        info = np.zeros(K, dtype=np.int32)
        self._check(self._lib.lsspa_cv_lift_info(self._h, N.iptr(info)))
        return info

    def cv_lift_timing(self):
        """Device seconds of the last cv_lift_load's Gram side, of the last batch's lift launches and of its fold and
        statistics launches."""
        a, b, c = C.c_double(), C.c_double(), C.c_double()
        self._check(self._lib.lsspa_cv_lift_timing(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return {"gram": a.value / 1e3, "batch": b.value / 1e3, "stats": c.value / 1e3}

    def cv_lift_free(self):
        self._check(self._lib.lsspa_cv_lift_free(self._h))
        self._cv_lift_dims, self._cv_lift_g = None, 0

    debug_cv_lift_plan = staticmethod(debug_cv_lift_plan)

    # ---- bootstrap of the sampled attribution (p <= 127) -------------------------------------------
    BOOT_LIFT_MAX_P = 127

    def boot_lift_load(self, X_train, X_test, y_train, y_test, reg: float):
        """Keep [X | y] of both sides on the device for boot_lift_run (include/lsspa.h, lsspa_boot_lift_load); the loaded
        problem and the state of boot_load, cv_lift_load and multi_lift_load are not touched."""
        dt = np.float32 if (X_train.dtype == np.float32 and X_test.dtype == np.float32) else np.float64
        Xa, Xe = np.ascontiguousarray(X_train, dtype=dt), np.ascontiguousarray(X_test, dtype=dt)
        ya, ye = np.ascontiguousarray(y_train, dtype=dt), np.ascontiguousarray(y_test, dtype=dt)
        n, p = Xa.shape
        self._check(self._lib.lsspa_boot_lift_load(
            self._h, C.c_void_p(Xa.ctypes.data), int(p), C.c_void_p(ya.ctypes.data), int(n), C.c_void_p(Xe.ctypes.data),
            int(p), C.c_void_p(ye.ctypes.data), int(Xe.shape[0]), int(p), float(reg),
            N.F32 if dt == np.float32 else N.F64, N.HOST))
        self._boot_lift_dims, self._boot_lift_g, self._boot_lift_n = (int(p), int(n), int(Xe.shape[0])), 0, 0

    def boot_lift_set_players(self, labels, g=None):
        """Groups of columns as the players, as cv_lift_set_players names them (include/lsspa.h,
        lsspa_boot_lift_set_players); drops the orderings.  The library checks the labels."""
        self._lift_players("boot_lift", np.asarray(labels), g)
        self._boot_lift_n = 0

    def boot_lift_clear_players(self):
        self._lift_players("boot_lift", None, 0)
        self._boot_lift_n = 0

    def _boot_lift_sd(self):
        """(dimension of a sample: g with a player map, else p; samples of the orderings set)"""
        return self._lift_sd("boot_lift", (1, 0))[0], getattr(self, "_boot_lift_n", 0)

    def boot_lift_set_orderings(self, perms, antithetical: bool):
        """The one set of orderings every replicate and the point problem run through: perms [n_samples][d] (with
        antithetical a sample is an ordering and its reverse).  The library checks the orderings."""
        perms, _ = self._lift_perms("boot_lift", perms, "n_samples")
        B = perms.shape[0] if perms.ndim == 2 else 0
        self._check(self._lib.lsspa_boot_lift_set_orderings(self._h, N.iptr(perms) if perms.size else None, B,
                                                            int(bool(antithetical))))
        self._boot_lift_n = B

    def _boot_lift_weights(self, w, shape, side):
        if w is None:
            return None
        dims = getattr(self, "_boot_lift_dims", None)
        w = np.ascontiguousarray(w, dtype=np.float64)
        want = tuple(shape) + (dims[1 + side],) if dims is not None else w.shape
        if w.shape != want:
            raise ValueError(f"weights of the {('training', 'test')[side]} side must have shape {want}, got {w.shape}")
        return w

    def boot_lift_run(self, R: int, seed: int, w_train=None, w_test=None, block: int = 0, first: int = 0,
                      want_samples: bool = False):
        """(mean [R][d], m2 [R][d], r2 [R], r2_base [R], info [R]) of replicates first .. first + R - 1 over the orderings
        set (include/lsspa.h, lsspa_boot_lift_run); with want_samples a sixth array [R][n_samples][d] of every sample's
        entry.  A replicate's mean sums to r2 - r2_base."""
        d, ns = self._boot_lift_sd()
        wa, we = self._boot_lift_weights(w_train, (R,), 0), self._boot_lift_weights(w_test, (R,), 1)
        mean, m2, r2, base = np.empty((R, d)), np.empty((R, d)), np.empty(R), np.empty(R)
        info = np.zeros(R, dtype=np.int32)
        samples = np.empty((R, ns, d)) if want_samples else None
        self._check(self._lib.lsspa_boot_lift_run(self._h, int(R), int(seed) & (2 ** 64 - 1), int(first), N.dptr(wa),
                                                  N.dptr(we), int(block), N.dptr(mean), N.dptr(m2), N.dptr(r2),
                                                  N.dptr(base), N.iptr(info), N.dptr(samples)))
        return (mean, m2, r2, base, info, samples) if want_samples else (mean, m2, r2, base, info)

    def boot_lift_point(self, want_samples: bool = False):
        """(mean [d], m2 [d], r2, r2_base, info) of the original rows, weight 1 on every row, through the same path as one
        more problem (include/lsspa.h, lsspa_boot_lift_point); with want_samples a sixth array [n_samples][d]."""
        d, ns = self._boot_lift_sd()
        mean, m2, r2, base = np.empty(d), np.empty(d), C.c_double(), C.c_double()
        info = np.zeros(1, dtype=np.int32)
        samples = np.empty((ns, d)) if want_samples else None
        self._check(self._lib.lsspa_boot_lift_point(self._h, N.dptr(mean), N.dptr(m2), C.byref(r2), C.byref(base),
                                                    N.iptr(info), N.dptr(samples)))
        out = (mean, m2, r2.value, base.value, int(info[0]))
        return out + (samples,) if want_samples else out

    def boot_lift_problem(self, r: int, seed: int = 0, w_train=None, w_test=None):
        """(G, g, H, h, inv_yy) of replicate r as the device writes it in a run: the counts of (seed, r, side), or the
        weights w_train [n] / w_test [m] of that replicate; r < 0: the point problem."""
        p = (getattr(self, "_boot_lift_dims", None) or (1, 0, 0))[0]
        wa, we = self._boot_lift_weights(w_train, (), 0), self._boot_lift_weights(w_test, (), 1)
        G, g, H, h, yy = np.empty((p, p)), np.empty(p), np.empty((p, p)), np.empty(p), C.c_double()
        self._check(self._lib.lsspa_boot_lift_get_problem(self._h, int(r), int(seed) & (2 ** 64 - 1), N.dptr(wa),
                                                          N.dptr(we), N.dptr(G), N.dptr(g), N.dptr(H), N.dptr(h),
                                                          C.byref(yy)))
        return G, g, H, h, yy.value

    def boot_lift_debug_grams(self, R: int, w_train=None, w_test=None):
        """(S_train, S_test [R][p+1][p+1], wsum [R]): the weighted sums before finalise (None: weight 1 on that side)."""
        c = self._boot_lift_dims[0] + 1
        wa, we = self._boot_lift_weights(w_train, (R,), 0), self._boot_lift_weights(w_test, (R,), 1)
        Sa, Se, ws = np.empty((R, c, c)), np.empty((R, c, c)), np.empty(R)
        self._check(self._lib.lsspa_boot_lift_debug_grams(self._h, int(R), N.dptr(wa), N.dptr(we), N.dptr(Sa), N.dptr(Se),
                                                          N.dptr(ws)))
        return Sa, Se, ws

    def boot_lift_timing(self):
        """Device seconds of the last pass: counts, Gram side, lift launches, statistics launches; and `launches`, the
        number of lift launches."""
        a, b, c, d, n = C.c_double(), C.c_double(), C.c_double(), C.c_double(), C.c_int64()
        self._check(self._lib.lsspa_boot_lift_timing(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(d), C.byref(n)))
        return {"counts": a.value / 1e3, "gram": b.value / 1e3, "lift": c.value / 1e3, "stats": d.value / 1e3,
                "launches": n.value}

    def boot_lift_free(self):
        self._check(self._lib.lsspa_boot_lift_free(self._h))
        self._boot_lift_dims, self._boot_lift_g, self._boot_lift_n = None, 0, 0

    debug_boot_lift_plan = staticmethod(debug_boot_lift_plan)

    def _exact_timing(self, getter):
        ms, mx, n = C.c_double(), C.c_double(), C.c_int64()
        self._check(getter(self._h, C.byref(ms), C.byref(mx), C.byref(n)))
        return ms.value / 1e3, mx.value / 1e3, n.value

    def _exact_values(self, fn, masks, *labels_g):
        masks = np.ascontiguousarray(masks, dtype=np.uint64).ravel()
        out = np.empty(len(masks))
        self._check(fn(self._h, *labels_g, masks.ctypes.data_as(C.POINTER(C.c_uint64)), len(masks), N.dptr(out)))
        return out

    def subsets_timing(self):
        """(kernel seconds, longest launch in seconds, launches) of the last subsets_shapley, subsets_interactions,
        subsets_best or subsets_top call."""
        return self._exact_timing(self._lib.lsspa_subsets_timing)

    def debug_subset_values(self, masks):
        """Test hook: v(S) of every mask (bit j = feature j) by the enumeration's own device code."""
        return self._exact_values(self._lib.lsspa_debug_subset_values, masks)

    # ---- exact attribution over groups of columns (g <= 32, p <= 64) ---------------------
    @staticmethod
    def _labels(labels):
        labels = np.ascontiguousarray(labels, dtype=np.int32).ravel()
        return labels, (int(labels.max()) + 1 if len(labels) else 0)

    def groups_shapley(self, labels):
        """(phi, info): the exact Shapley attribution over the groups of columns that labels names (one label per
        column: -1 the baseline, 0 .. g-1 the groups; include/lsspa.h, lsspa_groups_shapley), phi of length g.  The
        library checks the labels (their length is the caller's to get right: p of the loaded problem)."""
        labels, g = self._labels(labels)
        if len(labels) != self.p:
            raise ValueError(f"labels must have length p = {self.p}")
        phi = np.empty(max(g, 1))
        info = C.c_int32()
        self._check(self._lib.lsspa_groups_shapley(self._h, N.iptr(labels), g, N.dptr(phi), C.byref(info)))
        return phi, info.value

    def groups_interactions(self, labels):
        """(phi, I, info): phi as groups_shapley gives it (bitwise) and the raw pairwise Shapley interaction index
        I [g][g] between the groups from the same enumeration (include/lsspa.h, lsspa_groups_interactions): symmetric,
        0 on the diagonal, indexed by the labels like phi.  groups_timing() then speaks of this call."""
        labels, g = self._labels(labels)
        if len(labels) != self.p:
            raise ValueError(f"labels must have length p = {self.p}")
        n = max(g, 1)
        phi, inter = np.empty(n), np.empty((n, n))
        info = C.c_int32()
        self._check(self._lib.lsspa_groups_interactions(self._h, N.iptr(labels), g, N.dptr(phi), N.dptr(inter),
                                                        C.byref(info)))
        return phi, inter, info.value

    def groups_owen(self, labels):
        """(owen, phi, info): the exact Owen value of every column with the groups that labels names as coalition
        structure (include/lsspa.h, lsspa_groups_owen) -- owen of length p, 0.0 on baseline columns, a group's entries
        summing to its phi -- and phi of length g, bitwise groups_shapley's.  groups_timing() then speaks of all of this
        call's enumerations."""
        labels, g = self._labels(labels)
        if len(labels) != self.p:
            raise ValueError(f"labels must have length p = {self.p}")
        owen, phi = np.empty(self.p), np.empty(max(g, 1))
        info = C.c_int32()
        self._check(self._lib.lsspa_groups_owen(self._h, N.iptr(labels), g, N.dptr(owen), N.dptr(phi), C.byref(info)))
        return owen, phi, info.value

    def groups_best(self, labels):
        """(u, masks, found, info): the best group subset of every size k = 0 .. g (the number of groups beside the
        baseline) by the out-of-sample R^2 u, over all 2^g subsets of the groups that labels names (include/lsspa.h,
        lsspa_groups_best): u [g + 1] float64, masks [g + 1] uint32 (bit k = group k), found [g + 1] bool (False: no
        candidate of that size, u is NaN).  groups_timing() then speaks of this call."""
        labels, g = self._labels(labels)
        if len(labels) != self.p:
            raise ValueError(f"labels must have length p = {self.p}")
        n = max(g, 0) + 1
        u, masks, found = np.empty(n), np.empty(n, dtype=np.uint32), np.empty(n, dtype=np.uint8)
        info = C.c_int32()
        self._check(self._lib.lsspa_groups_best(
            self._h, N.iptr(labels), g, N.dptr(u), masks.ctypes.data_as(C.POINTER(C.c_uint32)),
            found.ctypes.data_as(C.POINTER(C.c_uint8)), C.byref(info)))
        return u, masks, found.astype(bool), info.value

    GROUPS_TOP_MAX = 16

    def groups_top(self, labels, n_best=10):
        """(u, masks, count, info): the n_best <= 16 best group subsets of every size k = 0 .. g, best first -- the
        larger u, on equal values the smaller mask (include/lsspa.h, lsspa_groups_top): u [g + 1][n_best] float64, masks
        [g + 1][n_best] uint32 (bit k = group k), count [g + 1] int32, the valid ranks of a size (NaN / 0 past them).
        Rank 0 is groups_best's.  groups_timing() then speaks of this call."""
        labels, g = self._labels(labels)
        if len(labels) != self.p:
            raise ValueError(f"labels must have length p = {self.p}")
        n, T = max(g, 0) + 1, int(n_best)
        u, masks = np.empty((n, max(T, 0))), np.empty((n, max(T, 0)), dtype=np.uint32)
        count = np.empty(n, dtype=np.int32)
        info = C.c_int32()
        self._check(self._lib.lsspa_groups_top(
            self._h, N.iptr(labels), g, T, N.dptr(u), masks.ctypes.data_as(C.POINTER(C.c_uint32)),
            count.ctypes.data_as(C.POINTER(C.c_int32)), C.byref(info)))
        return u, masks, count, info.value

    debug_groups_top_plan = staticmethod(debug_groups_top_plan)

    def groups_timing(self):
        """(kernel seconds, longest launch in seconds, launches) of the last groups_shapley, groups_interactions,
        groups_owen, groups_best or groups_top call."""
        return self._exact_timing(self._lib.lsspa_groups_timing)

    def debug_group_values(self, labels, masks):
        """Test hook: u(S) of every mask (bit k = group k) by the grouped enumeration's own device code."""
        labels, g = self._labels(labels)
        if len(labels) != self.p:
            raise ValueError(f"labels must have length p = {self.p}")
        return self._exact_values(self._lib.lsspa_debug_group_values, masks, N.iptr(labels), g)

    def factors(self):
        p, m = self.p, self.m
        R, q = np.empty((p, p)), np.empty(p)
        F, qt = np.empty((m, p)), np.empty(m)
        self._check(self._lib.lsspa_get_factors(self._h, N.dptr(R), N.dptr(q), N.dptr(F), N.dptr(qt)))
        return R, F, q, qt

    # ---- a2 / a3 / a4 ------------------------------------------------------------------
    def run_batch(self, perms, antithetical: bool, want_lifts: bool = False, accumulate: bool = True):
        perms = np.ascontiguousarray(perms, dtype=np.int32)
        if perms.ndim != 2 or perms.shape[1] != self.dim:
            raise ValueError(f"perms must have shape (B, {self.dim})")
        B = perms.shape[0]
        out = np.empty((B, self.dim)) if want_lifts else None
        self._check(self._lib.lsspa_lift_batch(self._h, N.iptr(perms), B, int(bool(antithetical)),
                                               N.dptr(out), self._acc_mode(accumulate)))
        return out

    @staticmethod
    def _acc_mode(accumulate):
        """False / True / 2: nothing, into the pending buffer (all-reduce + merge() follow), or -- one GPU -- folded
        into the running statistics at once (no merge() call; include/lsspa.h)."""
        if isinstance(accumulate, (bool, np.bool_)):
            return int(accumulate)
        return int(accumulate)      # integers go through as they are: the library refuses anything but 0, 1, 2

    # ---- sampled pairwise interactions (any number of players) -----------------------------
    PAIRS_MAX_D = 4096     # include/lsspa.h, LSSPA_PAIRS_MAX_D

    def pairs_enable(self, on: bool = True):
        """Allocate and zero (or free) the state of the sampled pairwise interaction index in the sample dimension
        (include/lsspa.h, lsspa_pairs_enable); a reduction and set_players / clear_players switch it off."""
        self._check(self._lib.lsspa_pairs_enable(self._h, int(bool(on))))

    def pairs_reset(self):
        self._check(self._lib.lsspa_pairs_reset(self._h))

    def pairs_batch(self, perms):
        """One batch of (B, dim) orderings: three orderings a sample through the kernels, every adjacent pair's second
        difference folded into its (count, mean, M2) on the device (include/lsspa.h, lsspa_pairs_batch)."""
        perms = np.ascontiguousarray(perms, dtype=np.int32)
        if perms.ndim != 2 or perms.shape[1] != self.dim:
            raise ValueError(f"perms must have shape (B, {self.dim})")
        self._check(self._lib.lsspa_pairs_batch(self._h, N.iptr(perms), perms.shape[0]))

    def pairs_get(self, tables: bool = True):
        """(n_samples, phi, count, mean, M2): phi the mean of all 3 n lift vectors; the three (dim, dim) tables symmetric
        with a zero diagonal, mean the raw index estimate of a pair (None, None, None with tables=False)."""
        d = self.dim
        n = C.c_int64()
        phi = np.empty(d)
        count = np.empty((d, d), dtype=np.int64) if tables else None
        mean, m2 = (np.empty((d, d)), np.empty((d, d))) if tables else (None, None)
        self._check(self._lib.lsspa_pairs_get(self._h, C.byref(n), N.dptr(phi),
                                              count.ctypes.data_as(N._pi64) if tables else None, N.dptr(mean), N.dptr(m2)))
        return n.value, phi, count, mean, m2

    def debug_pairs_inject(self, lifts, perms):
        """Test hook: the pair kernels alone on chosen lift vectors (3 B, dim) and orderings (B, dim) (include/lsspa.h,
        lsspa_debug_pairs_inject); no ordering is factored."""
        perms = np.ascontiguousarray(perms, dtype=np.int32)
        lifts = np.ascontiguousarray(lifts, dtype=np.float64)
        if perms.ndim != 2 or perms.shape[1] != self.dim or lifts.shape != (3 * perms.shape[0], self.dim):
            raise ValueError(f"perms must have shape (B, {self.dim}) and lifts (3 B, {self.dim})")
        self._check(self._lib.lsspa_debug_pairs_inject(self._h, N.dptr(lifts), N.iptr(perms), perms.shape[0]))

    def set_lanes(self, n: int):
        """1: batches run one after the other (default).  2: successive batches alternate between two workspaces on
        two streams (include/lsspa.h, lsspa_set_lanes)."""
        self._check(self._lib.lsspa_set_lanes(self._h, int(n)))
        self.lanes = int(n)

    def launch_batch(self, perms, antithetical: bool):
        """Enqueue a batch up to its lift vectors; returns a ticket for collect_batch / discard_batch."""
        perms = np.ascontiguousarray(perms, dtype=np.int32)
        if perms.ndim != 2 or perms.shape[1] != self.dim:
            raise ValueError(f"perms must have shape (B, {self.dim})")
        t = C.c_int32()
        self._check(self._lib.lsspa_lift_launch(self._h, N.iptr(perms), perms.shape[0], int(bool(antithetical)),
                                                C.byref(t)))
        return (t.value, perms.shape[0])

    def collect_batch(self, ticket, want_lifts: bool = False, accumulate: bool = True, first: int = 0,
                      count: int | None = None):
        """Accumulate (and / or fetch) ``count`` samples of a launched batch starting at sample ``first`` (default:
        all of it).  Parts are taken front to back."""
        t, B = ticket
        count = B - first if count is None else int(count)
        out = np.empty((count, self.dim)) if want_lifts else None
        self._check(self._lib.lsspa_lift_collect(self._h, t, int(first), count, N.dptr(out),
                                                 self._acc_mode(accumulate)))
        return out

    def collect_chunks(self, ticket, first: int, chunk: int, n_chunks: int, accumulate=2):
        """n_chunks consecutive parts of `chunk` samples of a launched batch, folded one after the other (include/lsspa.h,
        lsspa_lift_collect_chunks: one statistics launch for a small problem's parts, each still merged by itself)."""
        self._check(self._lib.lsspa_lift_collect_chunks(self._h, ticket[0], int(first), int(chunk), int(n_chunks),
                                                        self._acc_mode(accumulate)))

    def discard_batch(self, ticket):
        self._check(self._lib.lsspa_lift_discard(self._h, ticket[0]))

    def info(self) -> int:
        v = C.c_int32()
        self._check(self._lib.lsspa_get_info(self._h, C.byref(v)))
        return v.value

    def info_collected(self) -> int:
        """The info bits of every batch collected so far, without waiting for batches launched and dropped."""
        v = C.c_int32()
        self._check(self._lib.lsspa_get_info_collected(self._h, C.byref(v)))
        return v.value

    def sum_deviation(self) -> float:
        """Largest |sum of a sample's lifts - R^2| of all batches since the last reset (0 before full_fit)."""
        v = C.c_double()
        self._check(self._lib.lsspa_get_sum_deviation(self._h, C.byref(v)))
        return v.value

    def reset_stats(self):
        self._check(self._lib.lsspa_stats_reset(self._h))

    def pending_buffer(self) -> DeviceArrayView:
        ptr, cnt = C.c_void_p(), C.c_int64()
        self._check(self._lib.lsspa_stats_pending(self._h, C.byref(ptr), C.byref(cnt)))
        return DeviceArrayView(ptr.value, cnt.value, self)

    def merge(self):
        self._check(self._lib.lsspa_stats_merge(self._h))

    def stats(self, want_cov: bool = True):
        n = C.c_int64()
        mean = np.empty(self.dim)
        cov = np.empty((self.dim, self.dim)) if want_cov else None
        self._check(self._lib.lsspa_stats_get(self._h, C.byref(n), N.dptr(mean), N.dptr(cov)))
        return n.value, mean, cov

    def set_stats(self, n: int, mean, cov_biased):
        """Restore running statistics saved from ``stats()`` (checkpoint / resume)."""
        mean = np.ascontiguousarray(mean, dtype=np.float64)
        cov = np.ascontiguousarray(cov_biased, dtype=np.float64)
        if mean.shape != (self.dim,) or cov.shape != (self.dim, self.dim):
            raise ValueError("mean / covariance shapes do not match the loaded problem")
        self._check(self._lib.lsspa_stats_set(self._h, int(n), N.dptr(mean), N.dptr(cov)))

    # ---- lift history + device-side error estimator ---------------------------------------
    def history_enable(self, capacity: int):
        self._check(self._lib.lsspa_history_enable(self._h, int(capacity)))

    def history_count(self) -> int:
        n = C.c_int64()
        self._check(self._lib.lsspa_history_get(self._h, C.byref(n), None))
        return n.value

    def history(self):
        """All accumulated samples' lift vectors, (count, p)."""
        out = np.empty((self.history_count(), self.dim))
        n = C.c_int64()
        self._check(self._lib.lsspa_history_get(self._h, C.byref(n), N.dptr(out)))
        return out

    def history_append(self, lifts):
        lifts = np.ascontiguousarray(lifts, dtype=np.float64)
        if lifts.ndim != 2 or lifts.shape[1] != self.dim:
            raise ValueError("lifts must be (rows, p)")
        self._check(self._lib.lsspa_history_append(self._h, N.dptr(lifts), lifts.shape[0]))

    def error_draws(self, xi_local, n_total: int):
        """xi_local: (1024, n_local) standard normals for this engine's history rows."""
        xi_local = np.ascontiguousarray(xi_local, dtype=np.float64)
        if xi_local.ndim != 2 or xi_local.shape[0] != 1024:
            raise ValueError("xi must be (1024, n_local)")
        nl = xi_local.shape[1]
        self._check(self._lib.lsspa_error_draws(self._h, N.dptr(xi_local) if nl else None, max(nl, 1), nl,
                                                int(n_total)))

    def draws_buffer(self) -> DeviceArrayView:
        ptr, cnt = C.c_void_p(), C.c_int64()
        self._check(self._lib.lsspa_error_buffer(self._h, C.byref(ptr), C.byref(cnt)))
        return DeviceArrayView(ptr.value, cnt.value, self)

    def error_quantiles(self):
        feat, tot = np.empty(self.dim), C.c_double()
        self._check(self._lib.lsspa_error_quantiles(self._h, N.dptr(feat), C.byref(tot)))
        return feat, tot.value

    # ---- running form of the device-side estimator (include/lsspa.h) ---------------------
    RESULT_SLOTS = 64
    SMALL_P_MAX = 127      # csrc/k_small.hip small_p_eligible: p + 1 <= 128 takes the one-workgroup-per-ordering kernels

    def error_running_enable(self, seed: int):
        """D = Xi L and s = Xi 1 stay in HBM; Xi is a function of (seed, sample id, draw)."""
        self._check(self._lib.lsspa_error_running_enable(self._h, int(seed) & (2 ** 64 - 1)))

    def error_advance(self, first_id: int, stride: int = 1):
        """Fold the samples accumulated since the last call in: they are samples first_id, first_id + stride, ..."""
        self._check(self._lib.lsspa_error_advance(self._h, int(first_id), int(stride)))

    def error_running_draws(self, n_total: int):
        self._check(self._lib.lsspa_error_running_draws(self._h, int(n_total)))

    def error_quantiles_enqueue(self, slot: int):
        self._check(self._lib.lsspa_error_quantiles_enqueue(self._h, int(slot)))

    def error_check_enqueue(self, n_total: int, slot: int):
        """One rank: draws and quantiles of a check in one call (the draws are evaluated as they are read)."""
        self._check(self._lib.lsspa_error_check_enqueue(self._h, int(n_total), int(slot)))

    def error_result(self, slot: int, wait: bool = True):
        """(feature_errors, overall_error, mean, n) of a slot, or None if wait is False and it is not there yet."""
        feat, mean = np.empty(self.dim), np.empty(self.dim)
        tot, n, ready = C.c_double(), C.c_int64(), C.c_int32()
        self._check(self._lib.lsspa_error_result(self._h, int(slot), int(bool(wait)), C.byref(ready), N.dptr(feat),
                                                 C.byref(tot), N.dptr(mean), C.byref(n)))
        if not ready.value:
            return None
        return feat, tot.value, mean, n.value

    def group_collect(self, ticket, first, count, first_id, stride, n_after, slot):
        """The chunks of a launched batch in one call (include/lsspa.h, lsspa_group_collect): per chunk collect,
        (all-reduce + merge), fold into the running estimator and -- where n_after > 0 -- enqueue its check."""
        first = np.ascontiguousarray(first, dtype=np.int32)
        count = np.ascontiguousarray(count, dtype=np.int32)
        first_id = np.ascontiguousarray(first_id, dtype=np.int64)
        n_after = np.ascontiguousarray(n_after, dtype=np.int64)
        slot = np.ascontiguousarray(slot, dtype=np.int32)
        k = len(first)
        assert len(count) == len(first_id) == len(n_after) == len(slot) == k
        self._check(self._lib.lsspa_group_collect(
            self._h, ticket[0], k, N.iptr(first), N.iptr(count), first_id.ctypes.data_as(N._pi64), int(stride),
            n_after.ctypes.data_as(N._pi64), N.iptr(slot)))

    def error_state(self):
        D, s = np.empty((1024, self.dim)), np.empty(1024)
        self._check(self._lib.lsspa_error_state_get(self._h, N.dptr(D), N.dptr(s)))
        return D, s

    def set_error_state(self, D, s):
        D = np.ascontiguousarray(D, dtype=np.float64)
        s = np.ascontiguousarray(s, dtype=np.float64)
        if D.shape != (1024, self.dim) or s.shape != (1024,):
            raise ValueError("D must be (1024, p) and s (1024,)")
        self._check(self._lib.lsspa_error_state_set(self._h, N.dptr(D), N.dptr(s)))

    def error_xi(self, seed: int, first_id: int, stride: int, count: int):
        """Test hook: the estimator's normals of `count` sample ids, (1024, count)."""
        out = np.empty((1024, int(count)))
        self._check(self._lib.lsspa_error_xi(self._h, int(seed) & (2 ** 64 - 1), int(first_id), int(stride), int(count),
                                             N.dptr(out)))
        return out

    # ---- profiling / test hooks ---------------------------------------------------------
    def profile(self, on: bool):
        self._check(self._lib.lsspa_profile_enable(self._h, int(on)))

    def profile_reset(self):
        self._check(self._lib.lsspa_profile_reset(self._h))

    def profile_read(self):
        out = {}
        for k, name in enumerate(N.KERNEL_CLASSES):
            ms, cnt = C.c_double(), C.c_int64()
            self._check(self._lib.lsspa_profile_get(self._h, k, C.byref(ms), C.byref(cnt)))
            out[name] = (ms.value, cnt.value)
        return out

    def set_flags(self, flags: int):
        self._check(self._lib.lsspa_set_flags(self._h, int(flags)))

    def set_precision(self, dtype):
        """'float64' (default) or 'float32' for the per-ordering factorisation work."""
        name = np.dtype(dtype).name
        if name not in ("float64", "float32"):
            raise ValueError("precision must be float64 or float32")
        self._check(self._lib.lsspa_set_precision(self._h, N.F32 if name == "float32" else N.F64))
        self.precision = name

    def debug_fail_alloc(self, nth: int):
        """Test hook: the nth device allocation from now fails with MemoryError (0 disarms)."""
        self._check(self._lib.lsspa_debug_fail_alloc(self._h, int(nth)))

    def debug_reduce_chunk_rows(self, rows: int):
        """Test hook: rows per chunk of the streamed reduction of host arrays (a multiple of 16; 0: default sizing)."""
        self._check(self._lib.lsspa_debug_reduce_chunk_rows(self._h, int(rows)))

    def debug_inject_lifts(self, lifts):
        """Test hook: a (B, p) matrix of chosen lift vectors as a launched batch (include/lsspa.h,
        lsspa_debug_lift_inject); returns the ticket collect_batch / collect_chunks / group_collect take."""
        lifts = np.ascontiguousarray(lifts, dtype=np.float64)
        if lifts.ndim != 2 or lifts.shape[1] != self.p:
            raise ValueError(f"lifts must have shape (B, {self.p})")
        t = C.c_int32()
        self._check(self._lib.lsspa_debug_lift_inject(self._h, N.dptr(lifts), lifts.shape[0], C.byref(t)))
        return (t.value, lifts.shape[0])

    def mfma_probe(self, A, B, f32=False):
        A = np.ascontiguousarray(A, dtype=np.float64)
        B = np.ascontiguousarray(B, dtype=np.float64)
        D = np.empty((16, 16))
        self._check(self._lib.lsspa_mfma_probe(self._h, N.dptr(A), N.dptr(B), N.dptr(D), int(bool(f32))))
        return D

    def debug_factor(self, perm):
        pp, mp, vr = C.c_int32(), C.c_int32(), C.c_int32()
        self._check(self._lib.lsspa_debug_factor(self._h, None, None, None, None, C.byref(pp), C.byref(mp),
                                                 C.byref(vr)))
        perm = np.ascontiguousarray(perm, dtype=np.int32)
        L = np.empty((pp.value, pp.value))
        Lt = np.empty((pp.value, pp.value)) if self.tri else None
        V = np.empty((vr.value, mp.value))
        self._check(self._lib.lsspa_debug_factor(self._h, N.iptr(perm), N.dptr(L), N.dptr(Lt), N.dptr(V),
                                                 C.byref(pp), C.byref(mp), C.byref(vr)))
        return L, Lt, V
