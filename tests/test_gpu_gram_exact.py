"""The Gram reduction  C = [X | y]^T [X | y]  (csrc/k_gram.hip, reduce_rows in csrc/lsspa_api.hip) against an exact truth.

The data are integers small enough that every correct fp64 evaluation of every sum has the same bits (tests/gram_cases.py),
so the unscaled sums -- read as the raw all-reduce buffer of lsspa_reduce_partial, padding included -- are compared with
np.testing.assert_array_equal: no tolerance.  The cases walk the three unit classes, the three load forms, the per-class
slice counts, both reduce kernels and their accumulating forms, rows with ld > p and the streamed host path cut into short
chunks (lsspa_debug_reduce_chunk_rows); tests/test_gram_host.py checks on the CPU that the list reaches all of that under
the library's own plan.  Of every side's [P1pad][P1pad] buffer (P1pad = p + 1 rounded up to 128) the tests assert:
the lower triangle of the logical (p + 1)^2 matrix, the mirror images of the off-diagonal tiles, and zeros in all
the padding.  Inside a diagonal tile the 16 x 16 blocks above the block diagonal are nobody's (never written, never read).

One family is not integer: test_real_data_within_the_rounding_bound, against a long-double Gram and the standard bound of a
sum of n products in any order.  It prints its worst err / bound (GRAMACC ...); DESIGN.md has the figures of the MI355X."""
import numpy as np
import pytest

import gram_cases as GC
from ls_spa import _native as N
from ls_spa._engine import HipEngine

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
BY_NAME = {c[0]: c for c in GC.CASES}


def _place(X, y, location, ld_extra):
    """(X pointer, ld, y pointer, keep-alive) of rows laid out with stride ld = p + ld_extra.  The allocation ends with
    column p - 1 of the last row -- a vector that reached beyond a row's p columns would leave it there -- and the unused
    columns are NaN."""
    n, p = X.shape
    ld = p + ld_extra
    if n == 0:
        return None, ld, None, None
    count = (n - 1) * ld + p
    if location == GC.HOST:
        flat = np.full(count, np.nan, dtype=X.dtype)
        np.lib.stride_tricks.as_strided(flat, (n, p), (ld * flat.itemsize, flat.itemsize))[...] = X
        yk = np.ascontiguousarray(y)
        return flat.ctypes.data, ld, yk.ctypes.data, (flat, yk)
    import torch
    flat = torch.full((count,), float("nan"), dtype=getattr(torch, X.dtype.name), device="cuda")
    flat.as_strided((n, p), (ld, 1)).copy_(torch.from_numpy(np.ascontiguousarray(X)))
    yk = torch.from_numpy(np.ascontiguousarray(y)).to("cuda")
    torch.cuda.synchronize()
    return flat.data_ptr(), ld, yk.data_ptr(), (flat, yk)


def raw_sums(eng, train, test, p, location=GC.DEVICE, ld_extra=0, m_total=None):
    """lsspa_reduce_partial of (X, y) train and test rows, then the raw buffer as a host array [2][P1pad][P1pad]."""
    import torch
    (Xa, ya), (Xe, ye) = train, test
    assert Xa.dtype == Xe.dtype == ya.dtype == ye.dtype
    pa, lda, pya, keep_a = _place(Xa, ya, location, ld_extra)
    pe, lde, pye, keep_e = _place(Xe, ye, location, ld_extra)
    m_total = max(p, len(Xe)) if m_total is None else m_total
    eng._check(eng._lib.lsspa_reduce_partial(eng._h, pa, lda, pya, len(Xa), pe, lde, pye, len(Xe), m_total, p,
                                             N.F32 if Xa.dtype == np.float32 else N.F64, location))
    eng.synchronize()
    P1pad = (p + 1 + 127) // 128 * 128
    buf = torch.as_tensor(eng.reduce_buffer(), device="cuda").cpu().numpy().reshape(2, P1pad, P1pad).copy()
    del keep_a, keep_e
    return buf


def check_raw(C1, p, want, what):
    """One side's raw buffer [P1pad][P1pad] against the (p + 1)^2 matrix `want`."""
    P1 = p + 1
    L = C1[:P1, :P1]
    lo = np.tril_indices(P1)
    np.testing.assert_array_equal(L[lo], want[lo], err_msg=f"{what}: lower triangle")
    tile = np.arange(P1) // 128
    mirror = tile[:, None] < tile[None, :]
    np.testing.assert_array_equal(L[mirror], want[mirror], err_msg=f"{what}: mirror images of the off-diagonal tiles")
    np.testing.assert_array_equal(C1[P1:, :], 0.0, err_msg=f"{what}: padding rows")
    np.testing.assert_array_equal(C1[:, P1:], 0.0, err_msg=f"{what}: padding columns")


def finish_and_check(eng, n_total, p, reg=0.0):
    eng.reduce_finish(max(n_total, p), reg)
    G, g, H, h = eng.gram()
    np.testing.assert_array_equal(G, G.T, err_msg="G is not bitwise symmetric")
    np.testing.assert_array_equal(H, H.T, err_msg="H is not bitwise symmetric")
    return G, g, H, h


def case_data(name, dt, p, n):
    return GC.integer_data(GC.seed_of(name), n, p, dt), GC.integer_data(GC.seed_of(name) + 1, n, p, dt)


@pytest.mark.parametrize("case", GC.CASES, ids=[c[0] for c in GC.CASES])
def test_raw_sums_are_exact(engine, case):
    name, dt, p, n, location, ld_extra, chunk_rows = case
    train, test = case_data(name, dt, p, n)
    want = (GC.truth(*train), GC.truth(*test))
    try:
        engine.set_flags(0)
        engine.debug_reduce_chunk_rows(chunk_rows)
        buf = raw_sums(engine, train, test, p, location, ld_extra)
        for side in range(2):
            check_raw(buf[side], p, want[side], f"{name} side {side}")
        _, _, H, h = finish_and_check(engine, n, p)
        np.testing.assert_array_equal(H, want[1][:p, :p])          # the test side is scaled by 1.0
        np.testing.assert_array_equal(h, want[1][p, :p])
        assert engine.y_norm_sq == want[1][p, p]
        if chunk_rows:
            # the same rows in one chunk (default sizing): bit for bit the same buffer
            engine.debug_reduce_chunk_rows(0)
            one = raw_sums(engine, train, test, p, location, ld_extra)
            np.testing.assert_array_equal(buf, one)
            finish_and_check(engine, n, p)
    finally:
        engine.debug_reduce_chunk_rows(0)
        engine.set_flags(0)


def test_chunk_rows_hook_refuses_what_is_no_multiple_of_16(engine):
    try:
        for bad in (8, 17, -16, 1, 24):
            with pytest.raises(ValueError):
                engine.debug_reduce_chunk_rows(bad)
        for good in (16, 48, 1024, 0):
            engine.debug_reduce_chunk_rows(good)
        assert engine._lib.lsspa_debug_reduce_chunk_rows(None, 16) == 1
    finally:
        engine.debug_reduce_chunk_rows(0)


@pytest.fixture(scope="module")
def second_engine():
    eng = HipEngine(0)
    yield eng
    eng.close()


@pytest.mark.parametrize("case", GC.RANK_CASES, ids=[c[0] for c in GC.RANK_CASES])
def test_two_engines_as_two_ranks(engine, second_engine, case):
    """Each context reduces its rows, the buffers are added as the all-reduce would add them (zero-copy torch views of
    lsspa_reduce_buffer): the sum is the truth of the stacked rows, exactly."""
    import torch
    name, dt, p, n, cut = case
    train, test = case_data(name, dt, p, n)
    want = (GC.truth(*train), GC.truth(*test))
    cut_e = n // 2
    parts = [((train[0][:cut], train[1][:cut]), (test[0][:cut_e], test[1][:cut_e])),
             ((train[0][cut:], train[1][cut:]), (test[0][cut_e:], test[1][cut_e:]))]
    engs = (engine, second_engine)
    try:
        for eng, (tr, te) in zip(engs, parts):
            eng.set_flags(0)
            eng.debug_reduce_chunk_rows(0)
            raw_sums(eng, tr, te, p, GC.HOST, 0, m_total=n)
        t0 = torch.as_tensor(engs[0].reduce_buffer(), device="cuda")
        t1 = torch.as_tensor(engs[1].reduce_buffer(), device="cuda")
        t0 += t1
        t1.copy_(t0)
        torch.cuda.synchronize()
        P1pad = (p + 1 + 127) // 128 * 128
        for t in (t0, t1):
            buf = t.cpu().numpy().reshape(2, P1pad, P1pad)
            for side in range(2):
                check_raw(buf[side], p, want[side], f"{name} side {side}")
        out = [finish_and_check(eng, n, p, 0.05) for eng in engs]
        for a, b in zip(*out):
            np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(out[0][2], want[1][:p, :p])
    finally:
        for eng in engs:
            eng.set_flags(0)


@pytest.mark.parametrize("case", GC.RECT_CASES, ids=[c[0] for c in GC.RECT_CASES])
def test_rect_mode_keeps_the_test_rows_and_their_norm(engine, case):
    """Fewer than p test rows: the test side is the rows themselves (F_te, q_te of lsspa_get_factors) and ||y_test||^2."""
    name, dt, p, n, m, location = case
    (Xa, ya), _ = case_data(name, dt, p, n)
    Xe, ye = GC.integer_data(GC.seed_of(name) + 2, m, p, dt)
    try:
        engine.set_flags(0)
        engine.debug_reduce_chunk_rows(0)
        pa, lda, pya, keep_a = _place(Xa, ya, location, 0)
        pe, lde, pye, keep_e = _place(Xe, ye, location, 0)
        engine._check(engine._lib.lsspa_reduce(engine._h, pa, lda, pya, n, pe, lde, pye, m, p, 1.0,
                                               N.F32 if dt == GC.F32 else N.F64, location))
        engine._refresh_dims()
        assert not engine.tri and engine.m == m
        assert engine.y_norm_sq == float(np.sum(ye.astype(np.int64) ** 2))
        F, qt = np.empty((m, p)), np.empty(m)
        engine._check(engine._lib.lsspa_get_factors(engine._h, None, None, N.dptr(F), N.dptr(qt)))
        np.testing.assert_array_equal(F, Xe.astype(np.float64))
        np.testing.assert_array_equal(qt, ye.astype(np.float64))
        del keep_a, keep_e
    finally:
        engine.set_flags(0)


@pytest.mark.parametrize("name", GC.FINALIZE_CASES)
@pytest.mark.parametrize("reg", [0.0, 0.125, 1e-3])
def test_finalize(engine, name, reg):
    """G = C / N + reg I and g = C[p] / N against their long-double values: 3 u (|C_ab| / N + reg), u = 2^-53 -- one
    rounding of 1 / N, one of the product, one of the sum (a fused multiply-add only lowers it).  H, h and ||y_test||^2 are
    scaled by 1.0: they equal C."""
    _, dt, p, n, location, ld_extra, _ = BY_NAME[name]
    assert n >= p
    train, test = case_data(name, dt, p, n)
    want = (GC.truth(*train), GC.truth(*test))
    try:
        engine.set_flags(0)
        engine.debug_reduce_chunk_rows(0)
        buf = raw_sums(engine, train, test, p, location, ld_extra)
        check_raw(buf[0], p, want[0], name)
        G, g, H, h = finish_and_check(engine, n, p, reg)
    finally:
        engine.set_flags(0)
    Cl = want[0].astype(np.longdouble)
    nl, rl = np.longdouble(n), np.longdouble(reg)
    Gl = Cl[:p, :p] / nl + rl * np.eye(p, dtype=np.longdouble)
    bound = 3 * U * (np.abs(Cl[:p, :p]) / nl + rl * np.eye(p, dtype=np.longdouble))
    err = np.abs(G.astype(np.longdouble) - Gl)
    print(f"GRAMACC finalize {name} reg={reg}: worst err/bound G "
          f"{float(np.max(err / np.maximum(bound, np.longdouble(1e-300)))):.3f}")
    assert np.all(err <= bound)
    gl = Cl[p, :p] / nl
    assert np.all(np.abs(g.astype(np.longdouble) - gl) <= 3 * U * np.abs(gl))
    np.testing.assert_array_equal(H, want[1][:p, :p])
    np.testing.assert_array_equal(h, want[1][p, :p])
    assert engine.y_norm_sq == want[1][p, p]


def _poisoned(train, r, c, v):
    """(data with v at row r, column c (c == p: y), the (p + 1)^2 matrix it must give): row and column c are
    truth-with-0-there + v * (row r of Z), everything else the truth with that value set to 0."""
    X, y = train[0].copy(), train[1].copy()
    p = X.shape[1]
    if c == p:
        y[r] = 0
    else:
        X[r, c] = 0
    want = GC.truth(X, y)
    zr = np.concatenate([X[r].astype(np.float64), [float(y[r])]])
    with np.errstate(invalid="ignore"):
        line = want[c, :] + v * zr
        line[c] = want[c, c] + v * v
    want[c, :] = line
    want[:, c] = line
    if c == p:
        y[r] = v
    else:
        X[r, c] = v
    return (X, y), want


@pytest.mark.parametrize("p,n,dt", GC.NONFINITE_SHAPES, ids=[f"p{p}_n{n}_{dt}" for p, n, dt in GC.NONFINITE_SHAPES])
def test_non_finite_values_stay_in_their_row_and_column(engine, p, n, dt):
    """The guarded loads fetch real data where a zero belongs (the clamped last row, y for the columns at or beyond p,
    column 0 for the vectors beyond y) and clear it afterwards: a NaN there must not leak.  One NaN at a time at the
    places those loads touch, and +Inf once; n is no multiple of 16, so row n - 1 is the last row of a slice whose last
    chunk has an empty remainder.  Exactly row and column c of the logical matrix are NaN (+-Inf, or NaN where Inf
    meets a zero factor), every other entry is the truth without that value, the padding stays zero."""
    assert n % 16 != 0
    name = f"nonfinite_{dt}_p{p}_n{n}"
    train, test = case_data(name, dt, p, n)
    want_test = GC.truth(*test)
    spots = [(n - 1, 0, np.nan), (n - 1, p - 1, np.nan), (0, p - 1, np.nan), (n - 1, p, np.nan), (n - 1, p // 2, np.nan),
             (n - 1, p - 1, np.inf)]
    try:
        engine.set_flags(0)
        engine.debug_reduce_chunk_rows(0)
        for r, c, v in spots:
            bad, want = _poisoned(train, r, c, v)
            buf = raw_sums(engine, bad, test, p)
            what = f"{name} {v} at row {r} column {c}"
            assert np.isnan(want[c, :]).all() if np.isnan(v) else not np.isfinite(want[c, :]).any()
            assert np.isfinite(np.delete(np.delete(want, c, 0), c, 1)).all()
            check_raw(buf[0], p, want, what)
            check_raw(buf[1], p, want_test, what + " (the other side)")
        # leave a finite problem behind
        raw_sums(engine, train, test, p)
        finish_and_check(engine, n, p)
    finally:
        engine.set_flags(0)


@pytest.mark.parametrize("dt,p,n", GC.REAL_CASES, ids=[f"{dt}_p{p}_n{n}" for dt, p, n in GC.REAL_CASES])
def test_real_data_within_the_rounding_bound(engine, dt, p, n):
    """Columns 1e6 + N(0, 1) scaled by 1.7 * 2^e, e over -40 .. 40, against the long-double Gram of the fp64-widened
    inputs:  |C_ab - truth| <= gamma_n sum_k |z_ka| |z_kb|,  gamma_n = n u / (1 - n u) -- the bound of a sum of n products
    in any order, so it covers slices, chunks and the matrix instruction's own order alike.  (The truth's own error is
    2^-11 of it.)"""
    name = f"real_{dt}_p{p}_n{n}"
    train = GC.real_data(GC.seed_of(name), n, p, dt)
    test = GC.integer_data(GC.seed_of(name) + 1, n, p, dt)
    try:
        engine.set_flags(0)
        engine.debug_reduce_chunk_rows(0)
        buf = raw_sums(engine, train, test, p)
        finish_and_check(engine, n, p)
    finally:
        engine.set_flags(0)
    want, mag = GC.longdouble_gram(*train)
    gamma = np.longdouble(n * U) / (1 - np.longdouble(n * U))
    P1 = p + 1
    tile = np.arange(P1) // 128
    asserted = np.tril(np.ones((P1, P1), dtype=bool)) | (tile[:, None] < tile[None, :])
    ratio = np.abs(buf[0][:P1, :P1].astype(np.longdouble) - want) / (gamma * mag)
    worst = float(ratio[asserted].max())
    print(f"GRAMACC real {name}: worst err/bound {worst:.4f}")
    assert worst <= 1.0
    check_raw(buf[1], p, GC.truth(*test), name + " (the integer side)")
    assert not buf[0][P1:, :].any() and not buf[0][:, P1:].any()
