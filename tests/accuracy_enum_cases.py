"""The case table of tests/test_gpu_accuracy_enum.py: data, long-double truths and the fp64 host routes' errors.

TESTS ONLY.  Every case is hp_ref.gen(p, *shape(p), kappa, 7100 + p) (the seed rule of test_gpu_accuracy.values_case)
over KAPPAS; what differs is the game played on it.  A truth function returns a Truth: per result array the long-double
value rounded to fp64 and e_plain, the error of the fp64 NumPy / LAPACK route of the same game against it, and the
problem's (or every fold's / replicate's) true smallest relative pivot over the engine's threshold 16 p eps.  They are
cached, so the CPU test of the table (tests/test_hp_games_host.py) and a GPU test of one process share a truth.
No engine is touched here: the plans come from the host-only debug hooks."""
from functools import lru_cache

import numpy as np
import scipy.linalg as sla

import hp_games as HG
import hp_ref
import owen_ref
import perm_ref
from test_gpu_accuracy import KAPPAS, MG, T0, masks_of, shape, threshold
from test_groups_host import group_shapley, group_values, labels_of
from test_multi_groups_host import multi_group_values, multi_shapley_of_table
from test_multi_host import multi_gram_problem, multi_shapley_from_values, multi_subset_values, with_responses
from test_subsets_host import exact_shapley, gram_problem, subset_values

MULTI_RB = 8                                        # csrc/kernels.h; HipEngine.MULTI_RB (asserted by the plan test)
M_RESP = MULTI_RB + 1                               # two chunks of responses, the last with one
LABELS_G10 = labels_of([2] * 10, 4, seed=10)        # g = 10, p = 24, baseline of 4 (test_sweep_groups_shapley_g10_p24)
LABELS_G12 = labels_of([3] * 12, 4, seed=12)        # g = 12, p = 40 (test_sweep_group_values_g12_p40)
LABELS_OWEN = owen_ref.GPU_CASES["sizes_8_3_3_3"][0]    # p = 17: the smallest labelling of tests/test_gpu_owen.py whose
#                                                         refined games all have gh > 1 high groups, hence 2^gh > 1 units
LABELS_P10 = labels_of([2, 3, 1, 2], 2, seed=4)     # the groups of the resampling cases: g = 4 on p = 10, baseline of 2
MASKS_P20 = masks_of(20, 256, 20)
MASKS_G10 = masks_of(10, 128, 10)
MASKS_G12 = masks_of(12, 128, 12)
MASKS_P10 = masks_of(10, 64, 10)
PERM_SEED, PERM_R = 5, 3
BOOT_R = 4
CV_K = 3
PATH_KAPPA = 1e6
PATH_REGS = [0.0, 1e-12, 1e-6, 1.0, 1e6]            # times the mean diagonal of G
N_BEST = 3


def seed_of(p):
    return 7100 + p


def tol_of(e_plain):
    return max(T0["float64"], MG * e_plain)


class Truth:
    """want[name], e_plain[name] per result array; ratio: true smallest pivot / threshold, a float or one per fold /
    replicate; extra: whatever else a case needs (data, masks, margins)."""

    def __init__(self, ratio, **extra):
        self.want, self.e_plain, self.ratio = {}, {}, ratio
        self.__dict__.update(extra)

    def put(self, name, want, *plain):
        """e_plain: the error of the fp64 host route `plain`; of several routes, all of them references, the largest."""
        want = np.asarray(want, dtype=np.float64)
        self.want[name] = want
        worst = 0.0
        for route in plain:
            with np.errstate(invalid="ignore"):
                err = np.abs(np.asarray(route, dtype=np.float64) - want)
            if np.isfinite(err).any():
                worst = max(worst, float(np.nanmax(err)))
        self.e_plain[name] = worst

    def ratios(self):
        return np.atleast_1d(np.asarray(self.ratio, dtype=np.float64)).ravel()


def data_of(p, kappa):
    return hp_ref.gen(p, *shape(p), kappa, seed_of(p))


def multi_data_of(p, kappa):
    return with_responses(*data_of(p, kappa), M_RESP, seed_of(p))


def _plain(fn, *a):
    """An fp64 host route, quiet about what ill-conditioning does to it."""
    with np.errstate(all="ignore"):
        return fn(*a)


# ---- a, b: many responses ------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def multi_values_truth(kappa):
    D = multi_data_of(20, kappa)
    ref = HG.MultiProblem(*D)
    want = ref.values(MASKS_P20)
    t = Truth(ref.min_pivot / threshold(20), data=D)
    plain = _plain(multi_subset_values, *multi_gram_problem(*D), MASKS_P20)
    for r in range(M_RESP):
        t.put(r, want[:, r], plain[:, r])
    return t


@lru_cache(maxsize=None)
def multi_shapley_truth(kappa):
    D = multi_data_of(10, kappa)
    ref = HG.MultiProblem(*D)
    want = ref.shapley()
    t = Truth(ref.min_pivot / threshold(10), data=D)
    plain = multi_shapley_from_values(_plain(multi_subset_values, *multi_gram_problem(*D),
                                             np.arange(1 << 10, dtype=np.uint64)), 10)
    for r in range(M_RESP):
        t.put(r, want[r], plain[r])
    t.put("sums", ref.total(), plain.sum(axis=1))
    return t


# ---- c: many responses over groups -----------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def multi_groups_truth(kappa):
    D = multi_data_of(24, kappa)
    ref = HG.MultiProblem(*D)
    prob = multi_gram_problem(*D)
    want_v = ref.group_values(MASKS_G10, LABELS_G10)
    want_phi = ref.shapley(LABELS_G10)
    t = Truth(ref.min_pivot / threshold(24), data=D)
    plain_v = _plain(multi_group_values, *prob, LABELS_G10, MASKS_G10)
    plain_phi = multi_shapley_of_table(_plain(multi_group_values, *prob, LABELS_G10, np.arange(1 << 10)), 10)
    for r in range(M_RESP):
        t.put(("values", r), want_v[:, r], plain_v[:, r])
        t.put(("phi", r), want_phi[r], plain_phi[r])
    t.put("sums", ref.total(LABELS_G10), plain_phi.sum(axis=1))
    return t


@lru_cache(maxsize=None)
def multi_group_values_p40_truth(kappa):
    D = multi_data_of(40, kappa)
    ref = HG.MultiProblem(*D)
    want = ref.group_values(MASKS_G12, LABELS_G12)
    t = Truth(ref.min_pivot / threshold(40), data=D)
    plain = _plain(multi_group_values, *multi_gram_problem(*D), LABELS_G12, MASKS_G12)
    for r in range(M_RESP):
        t.put(r, want[:, r], plain[:, r])
    return t


# ---- d: Owen values (the GPU test goes through test_gpu_accuracy.values_case, which makes the same data) -----------------
@lru_cache(maxsize=None)
def owen_truth(kappa):
    d = data_of(17, kappa)
    ref = hp_ref.Problem(*d)
    want = HG.owen(ref, LABELS_OWEN)
    t = Truth(ref.min_pivot / threshold(17), data=d)
    t.put("owen", want, _plain(owen_ref.owen_values, *gram_problem(*d), LABELS_OWEN))
    return t


# ---- e: the permutation test -----------------------------------------------------------------------------------------------
def permuted(d):
    """(Xa, Xe, Ya, Ye): the responses of replicates 0 .. PERM_R - 1 with both sides permuted."""
    Xa, Xe, ya, ye = d
    return (Xa, Xe, perm_ref.permuted_responses(ya, PERM_SEED, range(PERM_R), 0),
            perm_ref.permuted_responses(ye, PERM_SEED, range(PERM_R), 1))


@lru_cache(maxsize=None)
def perm_truth(kappa, grouped):
    p, labels = (24, LABELS_G10) if grouped else (10, None)
    d = data_of(p, kappa)
    D = permuted(d)
    obs, ref = HG.MultiProblem(*d), HG.MultiProblem(*D)
    t = Truth(0.0, data=d)
    if grouped:
        full = np.arange(1 << 10)
        t.put("observed", obs.shapley(labels)[0], _plain(group_shapley, *gram_problem(*d), labels))
        plain = multi_shapley_of_table(_plain(multi_group_values, *multi_gram_problem(*D), labels, full), 10)
    else:
        t.put("observed", obs.shapley()[0], _plain(exact_shapley, *gram_problem(*d)))
        plain = multi_shapley_from_values(_plain(multi_subset_values, *multi_gram_problem(*D),
                                                 np.arange(1 << 10, dtype=np.uint64)), 10)
    want = ref.shapley(labels)
    for r in range(PERM_R):
        t.put(r, want[r], plain[r])
    t.ratio = min(obs.min_pivot, ref.min_pivot) / threshold(p)      # one design: the same pivots
    return t


# ---- f: the bootstrap --------------------------------------------------------------------------------------------------------
def cholesky_value(G, g, H, h, yy, cols):
    """v(cols) by a Cholesky solve of G_SS in fp64: the route the library's host code takes for a replicate's r2 and
    r2_base (include/lsspa.h, lsspa_boot_run).  A second reference beside the LU solves of subset_values / group_values:
    one number's fp64 error scatters by an order of magnitude around its bound, and at kappa = 1e6 this route is 12 x
    further from the truth than the LU route on the replicate where the library is (Numerics)."""
    cols = np.asarray(cols, dtype=np.int64)
    if len(cols) == 0:
        return 0.0
    sub = np.ix_(cols, cols)
    th = sla.cho_solve(sla.cho_factor(G[sub], lower=True), g[cols])
    return float(2.0 * th @ h[cols] - th @ H[sub] @ th) / yy


def boot_weights(X, seed):
    """[BOOT_R][n] for the rows X: all ones; two multinomial draws of n; and a hand-made pattern that starves the
    design's smallest singular direction v -- the third of the rows with the largest |x.v| left out, the others taken
    7 times (the smallest |x.v|) down to once (the largest left): the worst-conditioned replicate these weights can
    make of full-rank data, several times nearer the threshold than its siblings."""
    n = len(X)
    rng = np.random.default_rng(seed)
    lever = np.abs(X @ np.linalg.svd(X, full_matrices=False)[2][-1])
    order = np.argsort(lever, kind="stable")                     # ascending |x.v|
    kept = n - n // 3
    hand = np.zeros(n)
    hand[order[:kept]] = 7 - (6 * np.arange(kept)) // max(kept - 1, 1)
    return np.stack([np.ones(n), rng.multinomial(n, np.full(n, 1.0 / n)), rng.multinomial(n, np.full(n, 1.0 / n)),
                     hand]).astype(np.float64)


@lru_cache(maxsize=None)
def boot_truth(kappa):
    p = 10
    Xa, Xe, ya, ye = d = data_of(p, kappa)
    Za, Ze = np.column_stack([Xa, ya]), np.column_stack([Xe, ye])
    wa, we = boot_weights(Xa, 1), boot_weights(Xe, 2)
    ng = int(LABELS_P10.max()) + 1
    t = Truth(None, data=d, w_train=wa, w_test=we)
    ratios = []
    for r in range(BOOT_R):
        ref = HG.RowsProblem(Za, wa[r], Ze, we[r])
        prob = HG.plain_rows_problem(Za, wa[r], Ze, we[r])
        t.put(("phi", r), ref.shapley(), _plain(exact_shapley, *prob))
        everything, baseline = np.arange(p), np.nonzero(LABELS_P10 == -1)[0]
        t.put(("r2", r), float(ref.mask_value((1 << p) - 1)), _plain(subset_values, *prob, np.array([(1 << p) - 1]))[0],
              _plain(cholesky_value, *prob, everything))
        t.put(("gphi", r), ref.shapley(LABELS_P10), _plain(group_shapley, *prob, LABELS_P10))
        gv = _plain(group_values, *prob, LABELS_P10, np.array([0, (1 << ng) - 1]))
        t.put(("gr2", r), float(ref.group_value((1 << ng) - 1, LABELS_P10)), gv[1], _plain(cholesky_value, *prob, everything))
        t.put(("gbase", r), float(ref.group_value(0, LABELS_P10)), gv[0], _plain(cholesky_value, *prob, baseline))
        ratios.append(ref.min_pivot / threshold(p))
    t.ratio = np.array(ratios)
    return t


# ---- g, h: K-fold cross-validation --------------------------------------------------------------------------------------------
def cv_folds(n, p):
    """ids [n]: fold 0 has p + 2 rows (a nearly square test side, a large complement), fold 1 half the rows (a small
    training complement), fold 2 the rest; the rows shuffled."""
    order = np.random.default_rng(n).permutation(n)
    ids = np.full(n, 2, dtype=np.int32)
    ids[order[:p + 2]] = 0
    ids[order[p + 2:p + 2 + n // 2]] = 1
    return ids


LOPSIDED_N, LOPSIDED_SEED = 2000, 0


def lopsided_folds(n, p, seed):
    """ids [n]: fold 0 holds all rows but p, which folds 1 and 2 share.  Fold 0 trains on p rows -- a square training
    side: with the seed chosen its true pivot is 219 x the NOT_PD threshold at kappa 1e4 (no excuse), 2 x at 1e5 and
    0.02 x / 0.003 x at 1e6 / 3e6 (it must be flagged, its siblings at 4e3 x / 5e2 x must not) -- and a complement that
    a pooled-sum-minus-own-fold finalise would leave n / p = 200 times less accurate than the sum of the others."""
    order = np.random.default_rng(seed).permutation(n)
    ids = np.zeros(n, dtype=np.int32)
    ids[order[:p // 2]] = 1
    ids[order[p // 2:p]] = 2
    return ids


def cv_data_of(kappa, layout="issue"):
    """(X, y, ids): "issue" -- the training half of the case's data in the folds of cv_folds; "lopsided" -- 2000 rows of
    the same generator in the folds of lopsided_folds (the issue's folds cancel one bit at most and are all as well
    conditioned as the pooled problem: DESIGN.md, Numerics)."""
    if layout == "issue":
        Xa, _, ya, _ = data_of(10, kappa)
        return Xa, ya, cv_folds(len(ya), 10)
    Xa, _, ya, _ = hp_ref.gen(10, LOPSIDED_N, 1, kappa, seed_of(10) + 1)
    return Xa, ya, lopsided_folds(LOPSIDED_N, 10, LOPSIDED_SEED)


def path_regs(X):
    return np.array(PATH_REGS) * float(np.mean(np.einsum("ij,ij->j", X, X)) / len(X))


@lru_cache(maxsize=None)
def cv_truth(kappa, reg=0.0, layout="issue"):
    p, K = 10, CV_K
    X, y, ids = cv_data_of(kappa, layout)
    refs = HG.RowsProblem.of_folds(X, y, ids, K, reg)
    probs = HG.plain_fold_problems(X, y, ids, K, reg)
    full, all_masks = np.array([(1 << p) - 1], dtype=np.uint64), np.arange(1 << p, dtype=np.uint64)
    ng = int(LABELS_P10.max()) + 1
    gends = np.array([0, (1 << ng) - 1], dtype=np.uint64)
    t = Truth(None, X=X, y=y, ids=ids, refs=refs)
    # two fp64 host routes, both references: the oracles' LU solves and the Cholesky form of the same route.  On a fold
    # that trains on p rows the fit interpolates, |phi| reaches 6e4 and either route can be 20 x the other (measured on
    # the CPU: LU 1.2e-7 / Cholesky 1.2e-6 at kappa 1, 0.03 / 0.71 at kappa 1e3): e_plain is the larger.
    tabs, plain_tabs, chol_tabs, pivs = [], [], [], []
    all_bits, group_bits = HG.bits_of(all_masks, p), HG.group_members(np.arange(1 << ng), LABELS_P10)
    chol_g = []
    for f in range(K):
        v, piv = refs[f].all_values(with_pivots=True)
        tabs.append(v[:, 0])
        pivs.append(piv)
        plain_tabs.append(_plain(subset_values, *probs[f], all_masks))
        chol_tabs.append(_plain(HG.table, *probs[f], all_bits, HG.FP64)[0][:, 0])
        chol_g.append(_plain(HG.table, *probs[f], group_bits, HG.FP64)[0])
    want_fold = np.stack([HG.shapley_of_table(tabs[f][:, None], p)[0] for f in range(K)])
    plain_fold = np.stack([_plain(exact_shapley, *probs[f]) for f in range(K)])
    want_g = np.stack([refs[f].shapley(LABELS_P10, raw=True) for f in range(K)])
    plain_g = np.stack([_plain(group_shapley, *probs[f], LABELS_P10) for f in range(K)])
    want_ge = np.stack([refs[f].group_values(gends, LABELS_P10)[:, 0] for f in range(K)])
    plain_ge = np.stack([_plain(group_values, *probs[f], LABELS_P10, gends) for f in range(K)])
    chol_fold = np.stack([HG.shapley_of_table(chol_tabs[f][:, None], p, HG.FP64)[0] for f in range(K)])
    chol_gphi = np.stack([HG.shapley_of_table(chol_g[f], ng, HG.FP64)[0] for f in range(K)])
    sel = MASKS_P10.astype(np.int64)
    for f in range(K):
        t.put(("phi_fold", f), want_fold[f], plain_fold[f], chol_fold[f])
        t.put(("r2_fold", f), tabs[f][-1], plain_tabs[f][-1], chol_tabs[f][-1])
        t.put(("v_fold", f), tabs[f][sel], plain_tabs[f][sel], chol_tabs[f][sel])
        t.put(("gphi_fold", f), want_g[f], plain_g[f], chol_gphi[f])
        t.put(("gr2_fold", f), want_ge[f, 1], plain_ge[f, 1], chol_g[f][-1, 0])
        t.put(("gbase_fold", f), want_ge[f, 0], plain_ge[f, 0], chol_g[f][0, 0])
    t.put("phi", want_fold.sum(axis=0), plain_fold.sum(axis=0), chol_fold.sum(axis=0))
    t.put("gphi", want_g.sum(axis=0), plain_g.sum(axis=0), chol_gphi.sum(axis=0))
    v_cv, plain_cv, chol_cv = sum(tabs[1:], tabs[0]), sum(plain_tabs[1:], plain_tabs[0]), sum(chol_tabs[1:], chol_tabs[0])
    t.put("v", v_cv[sel], plain_cv[sel], chol_cv[sel])
    t.put("v_all", v_cv, plain_cv, chol_cv)
    t.table, t.pivots = v_cv, np.min(pivs, axis=0)
    t.ratio = np.array([refs[f].min_pivot for f in range(K)]) / threshold(p)
    return t


@lru_cache(maxsize=None)
def path_truths():
    X, _, _ = cv_data_of(PATH_KAPPA)
    return [cv_truth(PATH_KAPPA, float(reg)) for reg in path_regs(X)]


# ---- i: selection ------------------------------------------------------------------------------------------------------------
def ranking(v, p, T):
    """Per size k the T + 1 best (value, mask) of the table v [2^p], best first: the larger value, then the smaller mask
    (fewer where a size has fewer subsets)."""
    masks = np.arange(1 << p)
    size = HG.bits_of(masks, p).sum(axis=1)
    out = []
    for k in range(p + 1):
        sel = masks[size == k]
        order = sel[np.lexsort((sel, -v[sel].astype(np.float64)))][:T + 1]
        out.append([(v[m], int(m)) for m in order])
    return out


def margins(rank, T):
    """[p + 1][T]: how far rank t's true value is from both neighbours' (inf where there is none)."""
    out = np.full((len(rank), T), np.nan)
    for k, row in enumerate(rank):
        vals = [float(v) for v, _ in row]
        for t in range(min(T, len(row))):
            up = vals[t - 1] - vals[t] if t else np.inf
            down = vals[t] - vals[t + 1] if t + 1 < len(vals) else np.inf
            out[k, t] = min(up, down)
    return out


@lru_cache(maxsize=None)
def selection_truth(kappa):
    """The table of all 2^10 values of the one-problem game: v_all, every subset's own smallest pivot, the ranking."""
    p = 10
    d = data_of(p, kappa)
    ref = HG.MultiProblem(*d)
    v, piv = ref.all_values(with_pivots=True)
    t = Truth(ref.min_pivot / threshold(p), data=d)
    t.put("v_all", v[:, 0], _plain(subset_values, *gram_problem(*d), np.arange(1 << p, dtype=np.uint64)))
    t.table, t.pivots = v[:, 0], piv
    return t


def selection_cases(kappa):
    """[(name, truth)]: the one-problem table and the cross-validated one; both have .table, .pivots, e_plain['v_all']."""
    return [("subsets", selection_truth(kappa)), ("cv", cv_truth(kappa))]


def all_truths(kappa):
    """[(name, Truth)] of every case at this kappa, for the conditions of tests/test_hp_games_host.py."""
    out = [("multi_values", multi_values_truth(kappa)), ("multi_shapley", multi_shapley_truth(kappa)),
           ("multi_groups", multi_groups_truth(kappa)), ("multi_group_values_p40", multi_group_values_p40_truth(kappa)),
           ("owen", owen_truth(kappa)), ("perm", perm_truth(kappa, False)), ("perm_groups", perm_truth(kappa, True)),
           ("boot", boot_truth(kappa)), ("cv", cv_truth(kappa)), ("cv_lopsided", cv_truth(kappa, 0.0, "lopsided")),
           ("selection", selection_truth(kappa))]
    if kappa == PATH_KAPPA:
        out += [(f"cv_path reg[{l}]", t) for l, t in enumerate(path_truths())]
    return out
