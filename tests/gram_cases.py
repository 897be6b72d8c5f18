"""The cases of the exact-sum tests of the Gram reduction (csrc/k_gram.hip, reduce_rows in csrc/lsspa_api.hip), their
data and their truth.  Importable without a GPU: tests/test_gram_host.py checks on the CPU that the list reaches the unit
classes, load forms, slice plans and chunk counts it was written for (through lsspa_debug_gram_plan, the library's own
rule); tests/test_gpu_gram_exact.py runs it.

The data are integers uniform in [-2^15, 2^15], stored as fp64 or fp32 (both hold them exactly).  With n <= 2^17 rows every
partial sum of  sum_k z_ki z_kj  is an integer below 2^48 < 2^53, so EVERY correct fp64 evaluation -- any slice plan, any
chunking, any order inside the matrix instruction, any split over ranks -- has the same bits, and so has the fp64 BLAS
product  Z^T Z  the tests compare with (vetted against an int64 product on the CPU).  Products reach 2^30: one fp32
product or sum anywhere is visible.  The comparison is np.testing.assert_array_equal."""
import numpy as np

HOST, DEVICE = 0, 1
F64, F32 = "float64", "float32"
LIM = 1 << 15
N_BIG = 1003        # no multiple of 16: several slices and a ragged last chunk below six tiles
N_BIG6 = 1291       # six and seven tiles: three different per-class slice counts (6 / 7 / 8), every last slice ragged


def _layouts():
    # p -> what it is (tiles of 128 columns of [X | y]; xlive = live 16-column blocks of the last tile)
    return [(100, "1tile"), (200, "2tiles_ragged"), (255, "2tiles_full"), (257, "3tiles_ragged_classA"),
            (383, "3tiles_full"), (640, "6tiles_y_alone"), (641, "6tiles_xlive1"), (660, "6tiles_xlive2"),
            (680, "6tiles_xlive3"), (700, "6tiles_xlive4"), (710, "6tiles_xlive5"), (730, "6tiles_xlive6"),
            (750, "6tiles_xlive7"), (767, "6tiles_xlive8"), (769, "7tiles_xlive1"), (895, "7tiles_full")]


def _cases():
    out = []
    # fewer features than one 16-byte vector (all loads guarded), and exactly one (the smallest ragged load, colv = 0)
    for dt, p in ((F64, 1), (F32, 1), (F32, 2), (F32, 3), (F64, 2), (F32, 4)):
        for n in (1, 15, 16, 17, 33):
            out.append((f"tiny_{dt}_p{p}_n{n}", dt, p, n, DEVICE, 0, 0))
    # every residue m = p - col0 of the vector that holds column p (zfix_ragged): inside one tile, two and three tiles
    for dt, ps in ((F32, (101, 102, 103, 129, 130, 131, 132, 257, 258, 259, 260)), (F64, (101, 129, 130))):
        for p in ps:
            out.append((f"residue_{dt}_p{p}", dt, p, 100, DEVICE, 0, 0))
    # every class layout x rows
    for p, what in _layouts():
        big = N_BIG6 if p >= 640 else N_BIG
        for n in (5, 16, 100, big):
            for dt in (F64, F32):
                out.append((f"layout_{what}_{dt}_p{p}_n{n}", dt, p, n, DEVICE, 0, 0))
    # device rows with ld > p: unused columns are NaN, the allocation ends with the last row's column p - 1
    for p in (200, 641):
        for extra in (1, 3, 24):
            for dt in (F64, F32):
                out.append((f"strided_{dt}_p{p}_ld+{extra}", dt, p, 117, DEVICE, extra, 0))
    # streamed host rows: 3 or 4 chunks, the last of 1 .. 15 rows; p <= 254: the small reduce kernel accumulates
    for p in (100, 200, 257, 641):
        for rows, n in ((16, 16 * 3 + 7), (48, 48 * 3 + 5), (256, 256 * 2 + 9)):
            for dt in (F64, F32):
                out.append((f"chunks_{dt}_p{p}_rows{rows}_n{n}", dt, p, n, HOST, 0, rows))
    out.append(("chunks_float64_p200_rows48_n149_ld+5", F64, 200, 149, HOST, 5, 48))
    out.append(("chunks_float32_p257_rows16_n55_ld+2", F32, 257, 55, HOST, 2, 16))
    return out


# (name, dtype, p, n, location, ld_extra, chunk_rows)
CASES = _cases()
# two engines as two ranks: (name, dtype, p, n, training rows of rank 0)
RANK_CASES = [("ranks_6tiles_third", F64, 641, N_BIG, N_BIG // 3), ("ranks_6tiles_none", F64, 641, N_BIG, 0),
              ("ranks_1tile_third", F32, 100, 100, 100 // 3), ("ranks_1tile_none", F32, 100, 100, 0)]
# rect mode (fewer than p test rows): (name, dtype, p, n, m, location)
RECT_CASES = [("rect_float64_host", F64, 20, 40, 7, HOST), ("rect_float32_host", F32, 20, 40, 7, HOST),
              ("rect_float64_device", F64, 20, 40, 7, DEVICE), ("rect_float32_device", F32, 130, 140, 129, DEVICE)]
# test_finalize: names of CASES
FINALIZE_CASES = ["layout_1tile_float64_p100_n100", f"layout_6tiles_xlive1_float32_p641_n{N_BIG6}"]
# test_non_finite...: one tile, two tiles ragged, six tiles
NONFINITE_SHAPES = [(p, n, dt) for p in (100, 200, 641) for n in (17, 100) for dt in (F64, F32)]
# test_real_data...: (dtype, p, n)
REAL_CASES = [(F64, 130, 300), (F32, 130, 300), (F64, 641, 300), (F32, 641, 300)]


def seed_of(name):
    return int.from_bytes(name.encode(), "little") % (2 ** 32)


def integer_data(seed, n, p, dtype):
    """X [n][p], y [n]: integers uniform in [-2^15, 2^15] in the given dtype."""
    rng = np.random.default_rng(seed)
    X = rng.integers(-LIM, LIM + 1, size=(n, p)).astype(dtype)
    y = rng.integers(-LIM, LIM + 1, size=n).astype(dtype)
    return X, y


def truth(X, y):
    """[X | y]^T [X | y] in fp64: exact on integer_data (module docstring)."""
    Z = np.concatenate([np.asarray(X, dtype=np.float64), np.asarray(y, dtype=np.float64)[:, None]], axis=1)
    return Z.T @ Z


def truth_int64(X, y):
    Z = np.concatenate([np.asarray(X).astype(np.int64), np.asarray(y).astype(np.int64)[:, None]], axis=1)
    return Z.T @ Z


def real_data(seed, n, p, dtype):
    """The one non-integer family: column j = (1e6 + N(0, 1)) * 1.7 * 2^e_j, e_j spread over -40 .. 40 (no power of two, a
    large common offset, 80 binary orders between columns; inside the fp32 range as well)."""
    rng = np.random.default_rng(seed)
    e = np.round(np.linspace(-40, 40, p + 1)).astype(int)
    rng.shuffle(e)
    Z = (1e6 + rng.standard_normal((n, p + 1))) * (1.7 * np.exp2(e.astype(np.float64)))
    Z = Z.astype(dtype)
    return np.ascontiguousarray(Z[:, :p]), np.ascontiguousarray(Z[:, p])


def longdouble_gram(X, y):
    """(truth, sum_k |z_ka| |z_kb|) of the fp64-widened inputs in np.longdouble."""
    Z = np.concatenate([np.asarray(X, dtype=np.longdouble), np.asarray(y, dtype=np.longdouble)[:, None]], axis=1)
    A = np.abs(Z)
    return Z.T @ Z, A.T @ A


def chunk_plan(n, chunk_rows):
    """Row counts of the streamed chunks."""
    return [min(chunk_rows, n - r0) for r0 in range(0, n, chunk_rows)]
