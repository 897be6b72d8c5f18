"""The five row loaders of the C API on the MI355X -- lsspa_boot_load, lsspa_boot_groups_load, lsspa_perm_load,
lsspa_multi_load, lsspa_multi_lift_load -- over the whole matrix the header promises: float64 or float32 rows, on the
host or on the device, any ld >= p and ldy >= m, other strides on the two sides, host rows in several staging chunks.

tests/loader_cases.py has the cases and tests/test_loader_cases_host.py proves on the CPU what they reach.  The data are
integers on which every Gram sum is exact, laid out as tests/test_gpu_gram_exact.py lays its rows out: the unused columns
are NaN and the allocation ends with the last column of the last row, so a wrong stride, a swapped stride, a read of the
gap or a row packed to the wrong place puts a NaN or a wrong integer into what is read back.  What is read back:

  boot, boot_groups   boot_debug_grams with unit weights: [X | y]^T [X | y] of the packed rows of either side, and N
  perm                perm_gram (the Gram pass) and perm_run: X^T y[pi_r] of 17 replicates, the only view of the packed rows
  multi, multi_lift   multi_gram / multi_lift_gram: G, H, and g, h, yy of every response

all compared with np.testing.assert_array_equal against the int64 truth and against the baseline variant of the shape
(float64, host, ld = p, ldy = m: what the array methods of the engine pass).  One family of data is real-valued
(float32 values, widened exactly for the float64 load): the packed rows must have the same bits from either dtype, the
Gram pass -- whose float32 and float64 kernels differ -- stays inside the rounding bound of
tests/test_gpu_gram_exact.py (it prints LOADACC worst err / bound)."""
import functools

import numpy as np
import pytest

import gram_cases as GC
import loader_cases as LC
import perm_ref
from ls_spa import _native as N
from ls_spa._engine import HipEngine

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
LD = np.longdouble
SEED = 20240607
MANY = ("multi", "multi_lift")


@pytest.fixture(scope="module")
def eng():
    e = HipEngine(0)
    yield e
    e.close()


# ---- placement, load, read-back -------------------------------------------------------------------------------------
def place(A, location, ld):
    """(pointer, keep-alive) of the matrix A [n][c] laid out with stride ld >= c on the host or the device (_place of
    tests/test_gpu_gram_exact.py for any matrix): the allocation ends with column c - 1 of the last row and the unused
    columns are NaN."""
    n, c = A.shape
    assert ld >= c and n >= 1
    count = (n - 1) * ld + c
    if location == LC.HOST:
        flat = np.full(count, np.nan, dtype=A.dtype)
        np.lib.stride_tricks.as_strided(flat, (n, c), (ld * flat.itemsize, flat.itemsize))[...] = A
        return flat.ctypes.data, flat
    import torch
    flat = torch.full((count,), float("nan"), dtype=getattr(torch, A.dtype.name), device="cuda")
    flat.as_strided((n, c), (ld, 1)).copy_(torch.from_numpy(np.ascontiguousarray(A)))
    return flat.data_ptr(), flat


def load_args(c, data):
    """(arguments of the C entry point between the context and reg, keep-alive) of a case's rows."""
    (Xa, Ya), (Xe, Ye) = data
    (lda, ldya), (lde, ldye) = LC.strides(c)
    placed = [place(np.ascontiguousarray(A, dtype=c.dtype), c.location, ld)
              for A, ld in ((Xa, lda), (Ya, ldya), (Xe, lde), (Ye, ldye))]
    if c.location == LC.DEVICE:
        import torch
        torch.cuda.synchronize()
    pXa, pYa, pXe, pYe = (q[0] for q in placed)
    if c.family in MANY:
        return [pXa, lda, pYa, ldya, c.N, pXe, lde, pYe, ldye, c.M, c.p, c.m], placed
    return [pXa, lda, pYa, c.N, pXe, lde, pYe, c.M, c.p], placed


def load(eng, c, data=None, reg=None):
    """The case's rows through the pointer form of its family's load (which returns after the last read of the rows)."""
    args, keep = load_args(c, LC.case_data(c) if data is None else data)
    reg = LC.reg_of(c) if reg is None else reg
    kw = dict(f32=c.dtype == LC.F32, location=c.location)
    if c.family in ("boot", "boot_groups"):
        eng.boot_load_ptr(*args, reg, grouped=c.family == "boot_groups", **kw)
    else:
        getattr(eng, c.family + "_load_ptr")(*args, reg, **kw)
    del keep


def read(eng, c):
    """name -> array of everything the tests read back after a load of c."""
    if c.family in ("boot", "boot_groups"):
        Sa, Se, ws = eng.boot_debug_grams(2, np.ones((2, c.N)), np.ones((2, c.M)))
        return {"S_train": Sa, "S_test": Se, "wsum": ws}
    if c.family == "perm":
        G, g, H, h, yy = eng.perm_gram()
        phi, gp, hp, info = eng.perm_run(LC.PERM_R, SEED, LC.perm_labels(c.p))
        return {"G": G, "g": g[None, :], "H": H, "h": h[None, :], "yy": np.array([yy]), "gperm": gp, "hperm": hp,
                "phi": phi, "info": np.array([info])}
    G, g, H, h, yy = eng.multi_gram() if c.family == "multi" else eng.multi_lift_gram()
    return {"G": G, "g": g, "H": H, "h": h, "yy": yy}


def same_bits(got, want, what):
    assert got.keys() == want.keys()
    for k in got:
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what}: {k}")


@functools.lru_cache(maxsize=None)
def _indices(side, n):
    return [perm_ref.indices(SEED, r, side, n) for r in range(LC.PERM_R)]


def truth(c):
    """name -> array: what read() must return, from the int64 Gram of either side (the enumeration's phi aside)."""
    (Xa, Ya), (Xe, Ye) = LC.case_data(c)
    Ta, Te = LC.truth_int64(Xa, Ya), LC.truth_int64(Xe, Ye)
    if c.family in ("boot", "boot_groups"):
        return {"S_train": np.stack([Ta.astype(np.float64)] * 2), "S_test": np.stack([Te.astype(np.float64)] * 2),
                "wsum": np.full(2, float(c.N))}
    G, g, H, h, yy = LC.reduced_truth(c, Ta, Te)
    out = {"G": G, "g": g, "H": H, "h": h, "yy": yy}
    if c.family == "perm":
        for key, X, y, side, scale in (("gperm", Xa, Ya[:, 0], 0, 1.0 / c.N), ("hperm", Xe, Ye[:, 0], 1, 1.0)):
            Xi, yi = X.astype(np.int64), y.astype(np.int64)
            out[key] = np.stack([(Xi.T @ yi[a]).astype(np.float64) * scale for a in _indices(side, len(yi))])
    return out


_BASELINES = {}


def baseline_bits(eng, c):
    """read() after the baseline load of c's shape, once a shape."""
    key = LC.shape_of(c)
    if key not in _BASELINES:
        load(eng, LC.baseline(c))
        _BASELINES[key] = read(eng, LC.baseline(c))
    return _BASELINES[key]


# ---- 1. every case against the truth and against its baseline ------------------------------------------------------
@pytest.mark.parametrize("c", LC.CASES, ids=[LC.name(c) for c in LC.CASES])
def test_a_load_gives_the_truth_and_the_bits_of_its_baseline(eng, c):
    want = truth(c)
    load(eng, c)
    got = read(eng, c)
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{LC.name(c)}: {k} against the integer truth")
    if c.family in LC.GRAM_LOADED:
        np.testing.assert_array_equal(got["G"], got["G"].T)
        np.testing.assert_array_equal(got["H"], got["H"].T)
    # the baseline after the variant, so that it also overwrites what the variant left
    base = baseline_bits(eng, c)
    for k in want:
        np.testing.assert_array_equal(base[k], want[k], err_msg=f"{LC.name(c)}: {k} of the baseline against the truth")
    same_bits(got, base, LC.name(c) + " against its baseline")


def test_the_array_methods_take_the_same_path(eng):
    """boot_load, perm_load, multi_load, multi_lift_load of contiguous arrays are the baseline variant."""
    for family in LC.FAMILIES:
        c = LC.baseline(next(c for c in LC.CASES if c.family == family and c.p > 1))
        (Xa, Ya), (Xe, Ye) = LC.case_data(c)
        if family in MANY:
            getattr(eng, family + "_load")(Xa, Xe, Ya, Ye, LC.reg_of(c))
        elif family == "perm":
            eng.perm_load(Xa, Xe, Ya[:, 0], Ye[:, 0], LC.reg_of(c))
        else:
            eng.boot_load(Xa, Xe, Ya[:, 0], Ye[:, 0], LC.reg_of(c), grouped=family == "boot_groups")
        got = read(eng, c)
        same_bits(got, baseline_bits(eng, c), f"{family}: the array method against the pointer form")


# ---- 2. a run on every cell's packed rows ------------------------------------------------------------------------------
# (family, p, N, M, groups): the grouped run at the smallest p lsspa_boot_groups_load alone takes, over few groups
RUN_SHAPES = {"boot": (9, 40, 30, 0), "boot_groups": (33, 70, 50, 4)}
RUN_R = 3


def _boot_run(eng, family, p, N, M, groups, seed):
    rng = np.random.default_rng(seed)
    wa, we = (rng.integers(1, 8, size=(RUN_R, n)).astype(np.float64) for n in (N, M))
    if family == "boot":
        phi, r2, info = eng.boot_run(RUN_R, 0, wa, we)
        return {"phi": phi, "r2": r2, "info": info}
    phi, r2, base, info = eng.boot_groups_run(np.arange(p) % groups, RUN_R, 0, wa, we)
    return {"phi": phi, "r2": r2, "base": base, "info": info}


@functools.lru_cache(maxsize=None)
def _run_baseline(eng, family):
    p, N, M, groups = RUN_SHAPES[family]
    load(eng, LC.Case(family, LC.F64, LC.HOST, p, 1, N, M, 0, 0, 0), reg=LC.REG)
    return _boot_run(eng, family, p, N, M, groups, 7)


@pytest.mark.parametrize("dt,loc", LC.CELLS, ids=[f"{dt}_{'host' if loc == LC.HOST else 'device'}" for dt, loc in LC.CELLS])
@pytest.mark.parametrize("family", ["boot", "boot_groups"])
def test_a_bootstrap_run_has_the_bits_of_the_baseline_load(eng, family, dt, loc):
    """boot_run / boot_groups_run with fixed integer weights on rows loaded from every (dtype, location) cell, with
    padded rows of different strides: the attribution has the bits of the run on the baseline load."""
    p, N, M, groups = RUN_SHAPES[family]
    assert groups <= 8
    base = _run_baseline(eng, family)
    assert np.isfinite(base["phi"]).all() and not base["info"].any()
    load(eng, LC.Case(family, dt, loc, p, 1, N, M, 3, 24, 0), reg=LC.REG)
    same_bits(_boot_run(eng, family, p, N, M, groups, 7), base, f"{family} {dt} {loc}")


# ---- 3. real-valued rows: float32 against the same values in float64 ---------------------------------------------------
# (family, p, m, N, M)
REAL_SHAPES = [("boot", 9, 1, 300, 200), ("boot_groups", 33, 1, 300, 200), ("perm", 9, 1, 300, 200),
               ("multi", 7, 3, 300, 200), ("multi_lift", 16, 3, 300, 200)]


def real_case_data(shape):
    """((X_train, Y_train), (X_test, Y_test)): gram_cases.real_data in float32, widened exactly to float64."""
    family, p, m, N, M = shape
    out = []
    for side, n in enumerate((N, M)):
        X, y = GC.real_data(GC.seed_of("loader_real_%s" % family) + side, n, p + m - 1, LC.F32)
        Z = np.concatenate([X, y[:, None]], axis=1).astype(np.float64)
        out.append((np.ascontiguousarray(Z[:, :p]), np.ascontiguousarray(Z[:, p:])))
    return tuple(out)


def check_reduced_against_long_double(got, c, data, what):
    """G, g, H, h, yy against the long-double Gram of [X | Y]:  |C_ab - truth| <= gamma_n sum_k |z_ka| |z_kb|,
    gamma_n = n u / (1 - n u) (tests/test_gpu_gram_exact.py); the training side is then multiplied by a rounded 1 / N, two
    more roundings relative to the value (tests/test_gpu_permutation_test.py).  reg = 0."""
    p = c.p
    worst = 0.0
    for side, ((X, Y), n) in enumerate(zip(data, (c.N, c.M))):
        Z = np.concatenate([X, Y], axis=1).astype(LD)
        want, mag = Z.T @ Z, np.abs(Z).T @ np.abs(Z)
        bound = LD(n * U) / (1 - LD(n * U)) * mag
        if side == 0:
            want, bound = want / n, (bound + 2 * U * np.abs(want)) / n
        parts = ((got["G" if side == 0 else "H"], want[:p, :p], bound[:p, :p]),
                 (got["g" if side == 0 else "h"], want[p:, :p], bound[p:, :p]))
        if side == 1:
            parts += ((got["yy"], np.diagonal(want)[p:], np.diagonal(bound)[p:]),)
        for a, w, b in parts:
            assert a.shape == w.shape
            worst = max(worst, float((np.abs(a.astype(LD) - w) / np.maximum(b, LD(1e-300))).max()))
    print(f"LOADACC {what}: worst err/bound {worst:.4f}")
    assert worst <= 1.0


@pytest.mark.parametrize("shape", REAL_SHAPES, ids=[s[0] for s in REAL_SHAPES])
def test_real_valued_float32_rows_against_the_same_values_in_float64(eng, shape):
    family, p, m, N, M = shape
    data = real_case_data(shape)
    base = LC.Case(family, LC.F64, LC.HOST, p, m, N, M, 0, 0, 0)
    variants = [base._replace(dtype=LC.F32, location=LC.DEVICE, ld_extra_train=3, ld_extra_test=24, ldy_extra=1),
                base._replace(dtype=LC.F32, location=LC.HOST, ld_extra_train=1, ld_extra_test=0, ldy_extra=3),
                base._replace(location=LC.DEVICE, ld_extra_train=24, ld_extra_test=1, ldy_extra=1)]
    out = []
    for c in [base] + variants:
        load(eng, c, data, reg=0.0)
        got = read(eng, c)
        if family in ("boot", "boot_groups"):
            got.update(_boot_run(eng, family, p, N, M, 4, 11))
        out.append(got)
        if family in LC.GRAM_LOADED:
            check_reduced_against_long_double(got, c, data, LC.name(c))
    for c, got in zip(variants, out[1:]):
        # the packed rows are float64 whatever they were loaded from, and the same kernels run on them
        packed = [k for k in got if k not in ("G", "g", "H", "h", "yy")] if family in LC.GRAM_LOADED else list(got)
        if c.dtype == LC.F64:
            packed = list(got)            # the same Gram kernel too
        if family == "perm":
            # phi starts from G, H of the Gram pass: the float32 kernel's are within the bound above, not the same bits
            packed = [k for k in packed if c.dtype == LC.F64 or k in ("gperm", "hperm")]
        assert packed or family in MANY
        for k in packed:
            np.testing.assert_array_equal(got[k], out[0][k], err_msg=f"{LC.name(c)}: {k} against the float64 load")


# ---- 4. a load after a load ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,p_first,p_second", [("boot", 30, 16), ("perm", 32, 17)])
def test_a_second_load_of_the_same_packed_width_leaves_nothing_of_the_first(eng, family, p_first, p_second):
    """p = 30 then 16 pack to ldz = 32, p = 32 then 17 to ldx = 32: more rows of large values first, then the shorter,
    narrower case on the same buffers -- with the bits of the same load on a fresh engine."""
    first = LC.Case(family, LC.F64, LC.DEVICE, p_first, 1, 40, 30, 1, 3, 0)
    big = tuple((X * 2.0 ** 20, Y * 2.0 ** 20) for X, Y in LC.case_data(first))
    second = LC.Case(family, LC.F32, LC.DEVICE, p_second, 1, 17, 5, 3, 1, 0)
    load(eng, first, big, reg=0.0)
    load(eng, second)
    got = read(eng, second)
    if family == "boot":
        got.update(_boot_run(eng, family, p_second, 17, 5, 0, 5))
    fresh = HipEngine(0)
    try:
        load(fresh, second)
        want = read(fresh, second)
        if family == "boot":
            want.update(_boot_run(fresh, family, p_second, 17, 5, 0, 5))
    finally:
        fresh.close()
    same_bits(got, want, f"{family}: p = {p_first} then p = {p_second} against a fresh engine")
    t = truth(second)
    for k in t:
        np.testing.assert_array_equal(got[k], t[k], err_msg=k)


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", LC.FAMILIES)
def test_refused_loads_leave_the_loaded_state(eng, family):
    """ld < p, ldy < m, a dtype and a location that do not exist: refused on either side, and what was loaded before
    still runs and still gives its bits."""
    c = LC.baseline(next(c for c in LC.CASES if c.family == family and c.p > 1 and (c.m > 1 or family not in MANY)))
    load(eng, c)
    before = read(eng, c)
    args, keep = load_args(c, LC.case_data(c))
    fn = getattr(eng._lib, "lsspa_%s_load" % family)
    ld_at = (1, 6) if family in MANY else (1, 5)
    bad = [(at, c.p - 1) for at in ld_at] + ([(3, c.m - 1), (8, c.m - 1)] if family in MANY else [])
    calls = []
    for at, v in bad:
        a = list(args)
        assert a[at] in (c.p, c.m)
        a[at] = v
        calls.append((a, N.F64, N.HOST))
    calls += [(args, 7, N.HOST), (args, N.F64, 5), (args, -1, N.DEVICE)]
    for a, dtype, location in calls:
        with pytest.raises(ValueError, match="lsspa_%s_load" % family):
            eng._check(fn(eng._h, *a, LC.reg_of(c), dtype, location))
    del keep
    same_bits(read(eng, c), before, f"{family}: after the refused loads")
