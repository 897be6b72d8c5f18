"""The cases of the truth tests of the one-response fused per-ordering kernels (csrc/k_small.hip: small_reg_kernel<NB>,
NB = 1 .. 7, one wave a matrix in registers; small_p_kernel, both matrices in LDS, at nb = 8 or under developer flag
16384), their data and their orderings.  Importable without a GPU: tests/test_small_cases_host.py checks on the CPU
that the list reaches every class it was written for and that no truth case may be flagged NOT_PD;
tests/test_gpu_small_edges.py runs it.

What the kernels decide from p and where a case has to sit to see the decision:

    nb = (p + 1 + 15) // 16 block rows; the augmented row p sits last in a block (p + 1 = 16 k), opens one (16 k + 1)
        or sits one before the last (16 k - 1): P_BLOCK_EDGES, three residues for every nb where they exist
    register form: the gather's column pairs are clamped to min(2 lane, (p - 1) & ~1) (odd and even p), and at nb = 1
        there is no trailing block at all: P_TINY
    flags = 0: the register form up to p = 111 (nb <= 7), the LDS form from 112; flags = 16384: the LDS form everywhere

Data: hp_ref.gen(p, n, m, kappa, seed) with n, m = 4 p + 50, 3 p + 40 (shape() of tests/test_gpu_accuracy.py); the seed
depends on (p, kappa) alone, so that the forms, the ridge and the batch kinds of one shape share one long-double truth.
Orderings: hp_ref.orderings(p, seed) -- identity, reversed and three seeded."""
from collections import namedtuple

import numpy as np

Case = namedtuple("Case", "name p n m kappa reg flags form nb")

FLAG_LDS = 16384
REG, LDS = "reg", "lds"
REG_MAX_P = 111             # nb <= 7: the register form wherever flag 16384 is not set
SMALL_P_MAX = 127

P_BLOCK_EDGES = (14, 15, 16, 30, 31, 32, 46, 47, 48, 62, 63, 64, 78, 79, 80, 94, 95, 96, 110, 111, 112, 126, 127)
P_TINY = (1, 2, 3)
P_EDGES = P_TINY + P_BLOCK_EDGES
KAPPAS = (1.0, 1e4)
RIDGE, RIDGE_P = 0.25, (47, 127)        # one shape per form under flags = 0

BITS_P = (15, 16, 63, 111, 112, 127)    # test c
N_BIT_ORDERS = 32                       # bit_orderings(p, B) is a prefix of one sequence of this many per p
NOT_PD_RUNS = ((111, 0), (127, 0), (111, FLAG_LDS))     # test d: (p, flags)
DUP_SRC = 3                             # the column that is copied
HISTORY_P = (127, 17, 47)               # test e

SEED_OVERRIDE = {}          # (p, kappa) -> seed, for a generated case whose pivots come too near the threshold (none did)


def nb_of(p):
    return (p + 1 + 15) // 16


def form_of(p, flags):
    return LDS if (flags & FLAG_LDS or p > REG_MAX_P) else REG


def shape(p):
    return 4 * p + 50, 3 * p + 40


def seed_of(p, kappa):
    return SEED_OVERRIDE.get((p, kappa), 11000 + 10 * p + (0 if kappa == 1.0 else 1))


def _case(p, kappa, flags, reg=0.0):
    n, m = shape(p)
    form = form_of(p, flags)
    name = f"p{p}_k{kappa:g}_f{flags}" + (f"_ridge{reg:g}" if reg else "")
    return Case(name, p, n, m, kappa, reg, flags, form, nb_of(p))


def _cases():
    out = [_case(p, kappa, flags) for p in P_EDGES for kappa in KAPPAS for flags in (0, FLAG_LDS)]
    out += [_case(p, kappa, flags, RIDGE) for p in RIDGE_P for kappa in KAPPAS for flags in (0, FLAG_LDS)]
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}


def data_of(p, kappa):
    import hp_ref
    return hp_ref.gen(p, *shape(p), kappa, seed_of(p, kappa))


def orderings_of(p, kappa):
    import hp_ref
    return hp_ref.orderings(p, seed_of(p, kappa))


def with_reverses(orders):
    orders = np.asarray(orders)
    return np.concatenate([orders, orders[:, ::-1]])


def pivot_ratio(ref, orders):
    """Smallest relative pivot L_jj^2 / S_jj of G_pi and H_pi that the hp_ref.Problem `ref` meets over `orders` (as
    given: pass with_reverses() for what an antithetical batch factors), i.e. its min_pivot and min_pivot_test after
    their lifts, over the engine's threshold 16 p eps."""
    with np.errstate(all="ignore"):              # (a failed pivot gives NaN lifts; the pivots are what is asked for)
        ref.lifts(orders, False)
    return min(ref.min_pivot, ref.min_pivot_test) / (16 * ref.p * 2.220446049250313e-16)


def bit_orderings(p, B, first=0):
    """Rows first .. first + B of one sequence per p: the identity, its reverse and seeded orderings."""
    assert 1 <= B and first + B <= N_BIT_ORDERS
    rng = np.random.default_rng(500 + p)
    rows = [np.arange(p), np.arange(p)[::-1]] + [rng.permutation(p) for _ in range(N_BIT_ORDERS - 2)]
    return np.ascontiguousarray(np.array(rows[first:first + B], dtype=np.int32))


# ---- test d: a duplicated column, and a nearly duplicated one -------------------------------------------------------------
def dup_col(p):
    return p - 5


def dup_positions(p):
    """Where the second copy sits while the first sits at position 0: inside the first block, at its end, at the next
    block's first two rows, on both sides of every later block edge, and last."""
    edges = [b for k in range(2, p // 16 + 2) for b in (16 * k - 1, 16 * k)]
    return sorted({b for b in [1, 15, 16, 17] + edges + [p - 1] if 1 <= b <= p - 1})


def dup_orderings(p):
    """One ordering per position b of dup_positions(p): column DUP_SRC first, column dup_col(p) at b, the others seeded."""
    src, dup = DUP_SRC, dup_col(p)
    rng = np.random.default_rng(700 + p)
    rows = []
    for b in dup_positions(p):
        rest = [int(c) for c in rng.permutation(p) if c not in (src, dup)]
        row = [src] + rest
        row.insert(b, dup)
        rows.append(row)
    return np.ascontiguousarray(np.array(rows, dtype=np.int32))


DUP_WHERE = ("both_sets", "training_set_only", "test_set_only")


def dup_data(p, where):
    """data_of(p, 1.0) with column dup_col(p) an exact copy of column DUP_SRC in the set(s) named."""
    Xa, Xe, ya, ye = data_of(p, 1.0)
    Xa, Xe = Xa.copy(), Xe.copy()
    if where in ("both_sets", "training_set_only"):
        Xa[:, dup_col(p)] = Xa[:, DUP_SRC]
    if where in ("both_sets", "test_set_only"):
        Xe[:, dup_col(p)] = Xe[:, DUP_SRC]
    return Xa, Xe, ya, ye


# t of the near copy x_dup = x_src + t noise (both sets, noise ~ N(0, 1) seeded): chosen on the CPU so that the true smallest
# relative pivot over dup_orderings(p) and their reverses is between 1e3 and 1e4 times the threshold
# (tests/test_small_cases_host.py vets it and records the ratio)
NEAR_T = {111: 4.5e-5, 127: 4.5e-5}


def near_data(p):
    Xa, Xe, ya, ye = data_of(p, 1.0)
    Xa, Xe = Xa.copy(), Xe.copy()
    rng = np.random.default_rng(800 + p)
    Xa[:, dup_col(p)] = Xa[:, DUP_SRC] + NEAR_T[p] * rng.standard_normal(len(Xa))
    Xe[:, dup_col(p)] = Xe[:, DUP_SRC] + NEAR_T[p] * rng.standard_normal(len(Xe))
    return Xa, Xe, ya, ye
