"""The cases of the truth tests of the five row loaders of the C API -- lsspa_boot_load, lsspa_boot_groups_load,
lsspa_perm_load (load_rows and the pack kernels of csrc/k_boot.hip, csrc/k_perm.hip), lsspa_multi_load,
lsspa_multi_lift_load and the Gram pass of lsspa_perm_load (multi_reduce_sides in csrc/lsspa_api.hip) -- their data and
their truth.  Importable without a GPU: tests/test_loader_cases_host.py proves on the CPU that the table reaches the
edges it was written for, tests/test_gpu_row_loaders.py runs it.

A case is (family, dtype, location, p, m, N, M, ld_extra_train, ld_extra_test, ldy_extra): N training and M test rows of
p columns and m responses (m = 1: a vector y), stored with strides ld = p + ld_extra and, for the two many-response
loads, ldy = m + ldy_extra on the training side and m + LDY_TEST[ldy_extra] on the test side.

The data are gram_cases.integer_data's: integers in [-2^15, 2^15], the same values whatever the dtype and the strides
(the seed is that of the shape).  With at most 513 rows every partial sum of a Gram entry is an integer below 2^40, so
every correct fp64 evaluation has the int64 truth's bits, and every variant of a shape must give the bits of its
baseline variant: float64 rows on the host with ld = p and ldy = m, the only form the array methods of the engine pass.
"""
import collections
import itertools

import numpy as np

import gram_cases as GC

HOST, DEVICE = GC.HOST, GC.DEVICE
F64, F32 = GC.F64, GC.F32
FAMILIES = ("boot", "boot_groups", "perm", "multi", "multi_lift")
ROW_LOADED = ("boot", "boot_groups", "perm")      # through load_rows and a pack kernel
GRAM_LOADED = ("perm", "multi", "multi_lift")     # through multi_reduce_sides
CELLS = tuple(itertools.product((F64, F32), (HOST, DEVICE)))

Case = collections.namedtuple("Case", "family dtype location p m N M ld_extra_train ld_extra_test ldy_extra")

# load_rows' comment: host rows go through the staging buffers "at most ~64 MB of X at a time"; its rule is
# rows = max(1, min(n, (64 << 20) / (ld * esz)))
CHUNK_BYTES = 64 << 20
STREAM_LD = 32768           # 256 rows of float64 and 512 of float32 to a chunk: the smallest arrays that cross the constant

P_AXIS = {
    "boot": (1, 15, 16, 17, 32),             # ldz = 16 * floor((p + 16) / 16) steps at 15 | 16 and 31 | 32
    "boot_groups": (33, 47, 48, 63, 64),     # ... at 47 | 48 and 63 | 64
    "perm": (1, 16, 17, 32, 33, 48, 49, 64),  # ldx = 16 * ceil(p / 16) steps at 16 | 17, 32 | 33, 48 | 49
    "multi": (1, 7, 32),
    "multi_lift": (1, 16, 104),
}
M_AXIS = (1, 2, 5)
N_AXIS = (1, 3, 4, 5, 17)
N_SLICES = 513              # tests/test_gpu_bootstrap.py: three row slices of the weighted Gram kernel, the last of one row
LD_EXTRA = (0, 1, 3, 24)
LDY_EXTRA = (0, 1, 3)
LDY_TEST = {0: 0, 1: 3, 3: 1}     # the test side's ldy_extra: another one whenever there is padding
PERM_ENUM_MAX_P = 17        # perm_run enumerates 2^p subsets a replicate: beyond, the run names PERM_GROUPS groups
PERM_GROUPS = 3
PERM_R = 17
REG = 0.25
# the shapes (family, p, m) loaded with reg = REG; 0 elsewhere
REG_SHAPES = {("perm", 17, 1), ("multi", 7, 2), ("multi_lift", 16, 2)}

# (N, M): different on the two sides, each value of N_AXIS on either side
_ROWS = ((1, 3), (3, 4), (4, 5), (5, 17), (17, 1), (3, 1), (5, 4), (17, 5))
# (ld_extra_train, ld_extra_test): never equal when either is padded
_STRIDES = ((0, 1), (1, 0), (3, 24), (24, 3), (1, 3), (3, 1), (0, 24), (24, 0), (0, 3), (3, 0), (1, 24), (24, 1), (0, 0))


def _shapes(family):
    """(p, m, N, M) of a family."""
    out = []
    if family in ROW_LOADED:
        for k, p in enumerate(P_AXIS[family]):
            out.append((p, 1) + _ROWS[k % len(_ROWS)])
        if family == "boot":
            out.append((16, 1, N_SLICES, 5))
    elif family == "multi":
        for k, (p, m) in enumerate(itertools.product(P_AXIS[family], M_AXIS)):
            out.append((p, m) + _ROWS[k % len(_ROWS)])
    else:
        # lsspa_multi_lift_load takes M >= p test rows: the smallest M of the axis that does, and M = p = 104
        for k, (p, m) in enumerate(itertools.product(P_AXIS[family], M_AXIS)):
            N, M = _ROWS[k % len(_ROWS)]
            if M < p:
                M = 17 if p <= 17 else p
                N = N if N != M else 5
            out.append((p, m, N, M))
    return out


# Shape i of a family takes, in cell j, the strides _STRIDES[(i + 3 * j) % 13]: every cell of every family then sees
# every padding on either side, no padding on either side, and odd float32 strides on both sides
# (tests/test_loader_cases_host.py asserts all of it)
def _cases():
    out = []
    for family in FAMILIES:
        for i, (p, m, N, M) in enumerate(_shapes(family)):
            for j, (dt, loc) in enumerate(CELLS):
                ea, ee = _STRIDES[(i + 3 * j) % len(_STRIDES)]
                # (i = 3 * (index of p) + (index of m): every m meets every ldy_extra in every cell)
                ey = LDY_EXTRA[(i // 3 + i + j) % len(LDY_EXTRA)] if family in ("multi", "multi_lift") else 0
                out.append(Case(family, dt, loc, p, m, N, M, ea, ee, ey))
    # streamed host rows: the training side in two or three chunks, the last of one row; a small test side, other stride
    for family, p in (("boot", 17), ("boot_groups", 33), ("perm", 16)):
        for dt, N in ((F64, 257), (F64, 513), (F32, 513)):
            out.append(Case(family, dt, HOST, p, 1, N, 5, STREAM_LD - p, 3, 0))
    return out


CASES = _cases()
STREAMED = [c for c in CASES if c.p + c.ld_extra_train == STREAM_LD]
# (dtype, N) -> the chunks the training side of a streamed case is claimed to take
STREAMED_CLAIMS = {(F64, 257): [256, 1], (F64, 513): [256, 256, 1], (F32, 513): [512, 1]}


def name(c):
    loc = "host" if c.location == HOST else "device"
    ldy = f"_ldy+{c.ldy_extra}" if c.family in ("multi", "multi_lift") else ""
    return f"{c.family}_{c.dtype}_{loc}_p{c.p}_m{c.m}_N{c.N}_M{c.M}_ld+{c.ld_extra_train}+{c.ld_extra_test}{ldy}"


def shape_of(c):
    return (c.family, c.p, c.m, c.N, c.M)


def baseline(c):
    """The variant the array methods of the engine pass: float64 rows on the host, ld = p, ldy = m."""
    return c._replace(dtype=F64, location=HOST, ld_extra_train=0, ld_extra_test=0, ldy_extra=0)


def strides(c):
    """((ld_train, ldy_train), (ld_test, ldy_test)); ldy = 1 for a vector y."""
    if c.family in ("multi", "multi_lift"):
        return (c.p + c.ld_extra_train, c.m + c.ldy_extra), (c.p + c.ld_extra_test, c.m + LDY_TEST[c.ldy_extra])
    return (c.p + c.ld_extra_train, 1), (c.p + c.ld_extra_test, 1)


def reg_of(c):
    return REG if (c.family, c.p, c.m) in REG_SHAPES else 0.0


def perm_labels(p):
    """The labels perm_run gets: none while the enumeration over columns is small, else PERM_GROUPS groups round-robin
    (the load and the gathered X^T y[pi] do not know about groups; tests/perm_ref.py: XTY_CASES does the same)."""
    return None if p <= PERM_ENUM_MAX_P else (np.arange(p) % PERM_GROUPS).astype(np.int32)


def chunk_rows(ld, dtype):
    """Rows of a chunk of load_rows' staging loop (before the clamp to 1 .. n)."""
    return CHUNK_BYTES // (ld * np.dtype(dtype).itemsize)


def chunk_plan(n, ld, dtype):
    """Row counts of the chunks n host rows of stride ld take."""
    return GC.chunk_plan(n, max(1, min(n, chunk_rows(ld, dtype))))


def side_data(shape, side, n):
    """(X [n][p], Y [n][m]) in float64 of side 0 (training) or 1 (test): gram_cases.integer_data of the shape's seed,
    its last m columns the responses."""
    family, p, m = shape[:3]
    seed = GC.seed_of("loader_%s_p%d_m%d_N%d_M%d" % tuple(shape)) + side
    X, y = GC.integer_data(seed, n, p + m - 1, F64)
    return np.ascontiguousarray(X[:, :p]), np.ascontiguousarray(np.concatenate([X[:, p:], y[:, None]], axis=1))


def case_data(c):
    """((X_train, Y_train), (X_test, Y_test)) in float64: the same values for every variant of a shape."""
    return side_data(shape_of(c), 0, c.N), side_data(shape_of(c), 1, c.M)


def truth_int64(X, Y):
    """[X | Y]^T [X | Y] in int64."""
    Z = np.concatenate([X, Y], axis=1).astype(np.int64)
    return Z.T @ Z


def reduced_truth(c, T_train, T_test):
    """(G, g [m][p], H, h [m][p], yy [m]) that multi_reduce_sides must give on the integer truths of the two sides: the
    training side times the rounded 1 / N, reg on G's diagonal, the test side as it is."""
    p, m = c.p, c.m
    scale = 1.0 / c.N
    A, B = T_train.astype(np.float64), T_test.astype(np.float64)
    G = A[:p, :p] * scale + reg_of(c) * np.eye(p)
    return G, A[p:, :p] * scale, B[:p, :p], B[p:, :p].copy(), np.diagonal(B)[p:].copy()
