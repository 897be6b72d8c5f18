"""The sampled paths behind ls_spa_interactions_sampled and ls_spa_groups past their first loop trip: the pair kernels of
csrc/k_pairs.hip at every tile and chunk count up to d = 4096 and past the delta kernel's grid, against the exact integer
truth of tests/pairs_truth.py (vetted on the CPU by tests/test_pairs_truth_host.py); lsspa_pairs_batch with a sample whose
three rows fall into two launch sequences, with and without a player map, and on ill-conditioned data; the group fold of
csrc/k_players.hip past its grid and across launch sequences.

    B. the pair kernels alone (debug_pairs_inject, two successive batches so that the Chan merge runs)
    C. the whole path (pairs_batch): split sample, split sample under a player map, conditioning
    D. the group fold: singletons against the run without a map, non-trivial groups against the NumPy fold of the
       engine's own un-folded lifts -- bit for bit

Launch sequences: lift_launch cuts a batch into sequences of at most min(4096, 8 GB / bytes_per_ordering) orderings.  In
fp64 at p_pad = 384 (p = 257 .. 383) an ordering takes 4.06 MB, a sequence 2114 orderings at most, and the fold's grid of
4096 x 256 threads is never exceeded (2114 x 383 cells): its stride loop takes a second trip only where the work is
fp32 (2.05 MB an ordering, 4096 a sequence).  The fold itself is fp64 in both.  Section D runs both precisions and asserts
from the profile how many sequences there were (the k_players.hip section)."""
import numpy as np
import pytest

import hp_ref
import pair_ref
import pairs_truth as PT
from test_gpu_accuracy import MG, T0, shape, threshold
from test_gpu_group_sampling import even_sizes
from test_gpu_pairs import EPS, LIFT_TOL, MEAN_TOL, golden_p12, load_identity
from test_group_sampling_host import expand as expand_groups
from test_groups_host import labels_of
from test_subsets_host import data

pytestmark = pytest.mark.gpu

FOLD_GRID = 4096 * 256          # csrc/k_players.hip: threads of the fold's capped grid
DELTA_GRID = 8192 * 256         # csrc/k_pairs.hip: threads of the delta kernel's capped grid


def seeded_perms(d, B, seed):
    return np.random.default_rng(seed).permuted(np.tile(np.arange(d, dtype=np.int32), (B, 1)), axis=1)


# ---- B. the pair kernels alone -----------------------------------------------------------------------------------------
def inject_twice(engine, d, batches):
    """Two runs of reset + every batch through the pair kernels alone; the five results of each."""
    load_identity(engine, d)
    engine.pairs_enable(True)
    try:
        runs = []
        for _ in range(2):
            engine.pairs_reset()
            for lifts, perms in batches:
                engine.debug_pairs_inject(lifts, perms)
            runs.append(engine.pairs_get())
    finally:
        engine.pairs_enable(False)
    return runs


def check_integer_case(engine, d, B, seed):
    batches = PT.integer_batches(d, B, seed)
    truth = PT.PairTruth(d)
    for lifts, perms in batches:
        truth.add_batch(lifts, perms)
    t_count, t_mean, t_m2, max_delta = truth.tables(symmetric=False)      # the upper triangle, as the device keeps it
    runs = inject_twice(engine, d, batches)
    n, phi, count, mean, m2 = runs[0]
    assert n == 2 * B
    for a, b in zip(runs[0][1:], runs[1][1:]):          # two runs: the same bits
        np.testing.assert_array_equal(a, b)
    del runs
    for t in (count, mean, m2):                         # symmetric, zero diagonal
        np.testing.assert_array_equal(t, t.T)
        assert not np.diagonal(t).any()
    count, mean, m2 = np.triu(count), np.triu(mean), np.triu(m2)
    np.testing.assert_array_equal(count, t_count)
    assert np.count_nonzero(count) == np.count_nonzero(t_count)
    mean_err, m2_err = np.abs(mean - t_mean), np.abs(m2 - t_m2)
    print(f"d = {d}, B = {B}: pairs hit {np.count_nonzero(t_count)}, max count {t_count.max()}, "
          f"max |mean - truth| = {float(mean_err.max()):.2e}, max |M2 - truth| = {float(m2_err.max()):.2e}")
    assert np.all(mean_err <= 8 * t_count * EPS * max_delta)
    assert np.all(m2_err <= 8 * t_count * EPS * max_delta ** 2)
    np.testing.assert_allclose(phi, truth.phi.astype(np.float64), rtol=0, atol=8 * 6 * B * EPS * 1024)


@pytest.mark.parametrize("d", [191, 192, 193, 256, 257])
def test_pair_kernels_tile_counts(engine, d):
    """Three, four and five 64 x 64 tiles a side; a last tile that is full (192, 256), lacks one player (191) or holds one
    (193, 257: the diagonal tile of one player stores nothing, its column tiles one column)."""
    check_integer_case(engine, d, 5, seed=1000 * d + 5)


@pytest.mark.parametrize("B", [255, 256, 512, 513])
def test_pair_kernels_chunk_counts(engine, B):
    """The accumulate kernel stages 256 samples at a time: one chunk short of full, one full, two full, and a third of
    one sample.  d = 65: two tiles a side, the second with one player."""
    check_integer_case(engine, 65, B, seed=65000 + B)


def test_pair_kernels_top_of_the_range_and_the_stride_loop(engine):
    """d = LSSPA_PAIRS_MAX_D = 4096 and B = 513: B d = 2 101 248 cells against the delta kernel's 2 097 152 threads, so
    its grid-stride loop takes a second trip (the last 4096 cells: sample 512); tile row 63; int16 positions up to 4095;
    three chunks.  Every one of the 8 386 560 pairs is compared."""
    assert 513 * 4096 > DELTA_GRID >= 512 * 4096
    check_integer_case(engine, 4096, 513, seed=4096)


def test_pair_kernels_just_below_the_top(engine):
    """d = 4095: the last tile holds 63 players, so the sentinels -30000 / 30000 of the one missing player stand in LDS
    beside real positions up to 4094."""
    check_integer_case(engine, 4095, 3, seed=4095)


def test_pair_kernels_common_offset(engine):
    """Every Delta = 2^30 + u, |u| <= 8 (pairs_truth.offset_batches): mean^2 ~ 2^60 against M2 of some 100.  The
    tolerance is the project's rule max(floor, MG e_plain): e_plain the error of pair_ref (fp64 NumPy, the kernel's own
    order) against the exact truth, floors 8 n eps max|Delta| (mean) and 8 n eps max|u|^2 (M2).  M2 formed as
    sum x^2 - n mean^2 in fp64 misses this by seven orders of magnitude (tests/test_pairs_truth_host.py)."""
    d, B = PT.OFFSET_D, PT.OFFSET_B
    batches = PT.offset_batches()
    ref, truth = pair_ref.PairTables(d), PT.PairTruth(d, shift=PT.OFFSET)
    for lifts, perms in batches:
        ref.add_batch(lifts, perms)
        truth.add_batch(lifts, perms)
    t_count, t_mean, t_m2, max_delta = truth.tables()
    assert truth.max_u <= 8
    runs = inject_twice(engine, d, batches)
    n, phi, count, mean, m2 = runs[0]
    for a, b in zip(runs[0][1:], runs[1][1:]):
        np.testing.assert_array_equal(a, b)
    assert n == 2 * B
    np.testing.assert_array_equal(count, t_count)
    np.testing.assert_array_equal(count, ref.count)
    nmax = int(t_count.max())
    for name, got, plain, want, floor in (("mean", mean, ref.mean, t_mean, 8 * nmax * EPS * float(max_delta.max())),
                                          ("M2", m2, ref.m2, t_m2, 8 * nmax * EPS * 8.0 ** 2)):
        e_plain = float(np.abs(plain - want).max())
        err = float(np.abs(got - want).max())
        tol = max(floor, MG * e_plain)
        print(f"offset class {name}: e_plain {e_plain:.3e} err {err:.3e} r {err / max(e_plain, 4 * EPS):.2f} "
              f"tol {tol:.3e} (floor {floor:.3e})")
        assert err <= tol, f"{name}: |kernel - truth| = {err:.3e} > {tol:.3e} (e_plain {e_plain:.3e})"
    assert np.all(m2 >= 0)


# ---- C. the whole path ---------------------------------------------------------------------------------------------------
SPLIT_B = 1366          # 3 B = 4098 = 4096 + 2: sample 1365's rows are 4095 | 4096, 4097


def long_double_lifts(ref, rows):
    return np.array([ref.ordering_lift(r) for r in rows], dtype=np.longdouble)


def profiled_pairs_batch(engine, perms):
    """One pairs_batch; (result, launches per profile class)."""
    engine.pairs_enable(True)
    engine.profile(True)
    try:
        engine.profile_reset()
        engine.pairs_batch(perms)
        used = {k: v[1] for k, v in engine.profile_read().items()}
    finally:
        engine.profile(False)
    out = engine.pairs_get()
    assert engine.info() & 12 == 0
    return out, used


def test_split_sample_comes_back_whole(engine, golden):
    """p = 12 (golden p12, the register-resident kernel), B = 1366 in one call: 4098 unpaired rows in launch sequences of
    4096 and 2, the last sample's three rows in both.  Truth: the long-double lifts of all 4098 rows through the
    accumulation of pairs_truth; tolerances of test_one_batch_against_the_oracle."""
    d = golden_p12(golden)
    p = 12
    perms = seeded_perms(p, SPLIT_B, seed=1366)
    lifts = long_double_lifts(hp_ref.Problem(*d, 0.05), pair_ref.expand(perms))
    truth = PT.PairTruth(p, dtype=PT.LD).add_batch(lifts, perms)
    t_count, t_mean, _, _ = truth.tables()
    engine.load_data(*d, 0.05)
    engine.full_fit()                 # from here on every batch's lifts are checked against the full R^2
    try:
        (n, phi, count, mean, _), used = profiled_pairs_batch(engine, perms)
    finally:
        engine.pairs_enable(False)
    assert used["small_p"] == 2 and used["gather"] == 0, used          # the batch really was cut: 4096 + 2
    assert n == SPLIT_B
    np.testing.assert_array_equal(count, t_count)
    err = float(np.abs(mean - t_mean).max())
    phi_err = float(np.abs(phi - truth.phi).max())
    print(f"split sample p = 12: max |mean Delta - truth| = {err:.2e}, max |phi - truth| = {phi_err:.2e}, "
          f"min count {count[~np.eye(p, dtype=bool)].min()}")
    assert err <= MEAN_TOL and phi_err <= LIFT_TOL


def test_split_sample_under_a_player_map(engine, golden):
    """The same cut with g = 5 groups on the 12 columns (two baseline columns): each sequence folds its rows into
    L.folded + s_off g, and the pair kernels read [3 B][g].  Truth: long-double lifts of the expanded group orderings,
    folded by label.  Afterwards clear_players gives column orderings back."""
    d = golden_p12(golden)
    labels = labels_of([2, 3, 1, 2, 2], 2, seed=5)
    assert len(labels) == 12
    g = 5
    gperms = seeded_perms(g, SPLIT_B, seed=1367)
    ref = hp_ref.Problem(*d, 0.05)
    col = long_double_lifts(ref, [expand_groups(labels, r) for r in pair_ref.expand(gperms)])
    glifts = np.stack([col[:, labels == k].sum(axis=1) for k in range(g)], axis=1)
    truth = PT.PairTruth(g, dtype=PT.LD).add_batch(glifts, gperms)
    t_count, t_mean, _, _ = truth.tables()
    engine.load_data(*d, 0.05)
    engine.full_fit()
    try:
        engine.set_players(labels)
        (n, phi, count, mean, _), used = profiled_pairs_batch(engine, gperms)
    finally:
        engine.pairs_enable(False)
        engine.clear_players()
    assert used["small_p"] == 2 and used["lift"] == 2 and used["gather"] == 0, used     # two sequences, two folds
    assert n == SPLIT_B and count.shape == (g, g)
    np.testing.assert_array_equal(count, t_count)
    err = float(np.abs(mean - t_mean).max())
    phi_err = float(np.abs(phi - truth.phi).max())
    print(f"split sample g = 5 on p = 12: max |mean Delta - truth| = {err:.2e}, max |phi - truth| = {phi_err:.2e}")
    assert err <= MEAN_TOL and phi_err <= LIFT_TOL
    back = engine.run_batch(np.arange(12, dtype=np.int32)[None, :], False, want_lifts=True, accumulate=False)
    assert back.shape == (1, 12)
    np.testing.assert_allclose(back[0], np.asarray(ref.ordering_lift(np.arange(12)), dtype=np.float64), rtol=0,
                               atol=LIFT_TOL)


CONDITIONING = [("registers", 12, None), ("lds", 120, None), ("rect", 150, 100)]
_cond_rows = []


@pytest.mark.parametrize("kappa", [1e2, 1e4, 1e6])
@pytest.mark.parametrize("path,p,m", CONDITIONING, ids=[c[0] for c in CONDITIONING])
def test_pairs_batch_on_ill_conditioned_data(engine, path, p, m, kappa):
    """A Delta is the difference of two lifts: B = 8 samples on hp_ref.gen data of kappa_X = 1e2, 1e4, 1e6.  Truth: the
    means of the Delta of long-double lifts; tol = max(2 T0, MG e_plain), e_plain the same means from hp_ref.plain_lifts
    (NumPy / LAPACK fp64 on the same route).  The true smallest relative pivot is at least 100 x the NOT_PD threshold in
    every case (measured on the CPU: 361 x at worst, p = 120 at 1e6), so none may be flagged."""
    n, mm = shape(p, m)
    d = hp_ref.gen(p, n, mm, kappa, 7200 + p)
    perms = seeded_perms(p, 8, seed=p)
    rows = pair_ref.expand(perms)
    ref = hp_ref.Problem(*d)
    truth = PT.PairTruth(p, dtype=PT.LD).add_batch(long_double_lifts(ref, rows), perms)
    plain = PT.PairTruth(p, dtype=PT.LD).add_batch(hp_ref.plain_lifts(*d, 0.0, rows, False), perms)
    t_count, t_mean, _, _ = truth.tables()
    ratio = min(ref.min_pivot, ref.min_pivot_test) / threshold(p)
    assert ratio >= 100, f"the truth itself is {ratio:.3g} x the NOT_PD threshold: not a case for this test"
    e_plain = float(np.abs(plain.tables()[1] - t_mean).max())
    engine.load_data(*d, 0.0)
    assert engine.tri == (mm >= p)
    engine.full_fit()
    engine.pairs_enable(True)
    try:
        engine.pairs_batch(perms)
        _, phi, count, mean, _ = engine.pairs_get()
        info = engine.info()
    finally:
        engine.pairs_enable(False)
    err = float(np.abs(mean - t_mean).max())
    tol = max(2 * T0["float64"], MG * e_plain)
    r = err / max(e_plain, 4 * EPS)
    _cond_rows.append((path, p, kappa, err, e_plain, r, ratio))
    print(f"PAIRS {path} p={p} kappa={kappa:g}: err {err:.3e} e_plain {e_plain:.3e} r {r:.2f} tol {tol:.3e} "
          f"pivot/threshold {ratio:.3g} info {info}")
    assert info & 1 == 0, "NOT_PD on a positive definite problem"
    assert info & 12 == 0, f"sum deviation {engine.sum_deviation():.3e}"
    np.testing.assert_array_equal(count, t_count)
    assert np.all(np.isfinite(mean)) and err <= tol, f"|mean Delta - truth| = {err:.3e} > {tol:.3e}"
    assert float(np.abs(phi - truth.phi).max()) <= max(T0["float64"], MG * e_plain)


# ---- D. the group fold ---------------------------------------------------------------------------------------------------
FOLD_SAMPLES = 4096
FOLD_M = 384            # test rows: tri mode (m >= p) at the smallest m_pad, so that a sequence is as long as the rule allows


def profiled_lifts(engine, perms, anti):
    engine.profile(True)
    try:
        engine.profile_reset()
        out = engine.run_batch(perms, anti, want_lifts=True, accumulate=False)
        used = {k: v[1] for k, v in engine.profile_read().items()}
    finally:
        engine.profile(False)
    return out, used


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_fold_of_singletons_is_the_identity(engine, dtype):
    """p = g = 264 (general path, tri), 4096 seeded orderings in one run_batch, every column its own group: the fold is the
    identity, so the [4096][264] result equals the run without a map cell for cell.  fp32 work: one launch sequence of
    4096, 1 081 344 cells against the fold's 1 048 576 threads -- the stride loop's second trip.  fp64 work: the
    workspace rule cuts the batch (two sequences), the fold writes the second at L.folded + s_off g."""
    p = 264
    d = data(p, n=800, m=FOLD_M, seed=264)
    perms = seeded_perms(p, FOLD_SAMPLES, seed=264)
    engine.set_precision(dtype)
    try:
        engine.load_data(*d, 0.0)
        assert engine.tri
        want, used0 = profiled_lifts(engine, perms, False)
        engine.set_players(np.arange(p))
        try:
            got, used = profiled_lifts(engine, perms, False)
        finally:
            engine.clear_players()
        assert engine.info() == 0
    finally:
        engine.set_precision("float64")
    seqs = used["gather"]
    print(f"fold of singletons {dtype}: {seqs} launch sequence(s), {used['lift'] - seqs} fold launches")
    assert used0["gather"] == seqs and used0["small_p"] == 0 and used["lift"] == 2 * seqs and used0["lift"] == seqs
    if dtype == "float32":
        assert seqs == 1 and FOLD_SAMPLES * p > FOLD_GRID          # the launch sequence held all 4096 samples
    else:
        assert seqs == 2                                           # 2114 + 1982: no fold launch beyond the grid
    assert got.shape == (FOLD_SAMPLES, p) and np.all(np.isfinite(want))
    np.testing.assert_array_equal(got, want)


def numpy_fold(rows, labels, g, per):
    """The kernel's order: a group's columns ascending, from 0.0, the sample's rows one after the other, then
    0.5 (a + b)."""
    out = np.zeros((len(rows), g))
    for k in range(g):
        acc = np.zeros(len(rows))
        for c in np.nonzero(labels == k)[0]:
            acc = acc + rows[:, c]
        out[:, k] = acc
    return 0.5 * (out[0::2] + out[1::2]) if per == 2 else out


FOLD_CASES = [("float32", False, 1), ("float64", False, 2), ("float64", True, 4)]


@pytest.mark.parametrize("dtype,anti,seqs", FOLD_CASES, ids=[f"{c[0]}-{'anti' if c[1] else 'plain'}" for c in FOLD_CASES])
def test_fold_of_groups_equals_the_numpy_fold(engine, dtype, anti, seqs):
    """p = 300 in 257 groups (38 of two columns, 219 of one) and a baseline of five; 4096 group orderings.  Truth: the
    NumPy fold of the engine's own un-folded lifts of the expanded orderings (those are held to the long-double truth by
    tests/test_gpu_panel_edges.py), in the kernel's order -- so bit for bit.  Plain, fp32 work: one sequence, 1 052 672
    cells, the stride loop's second trip.  Plain, fp64: two sequences.  Antithetical (a baseline: the per = 2 rows, the
    pair run as two unpaired orderings and averaged by the fold), fp64: four sequences of 1057 samples at most."""
    p, g, nb = 300, 257, 5
    labels = labels_of(even_sizes(p - nb, g), nb, seed=p + g)
    d = data(p, n=900, m=FOLD_M, seed=300)
    gperms = seeded_perms(g, FOLD_SAMPLES, seed=257)
    per = 2 if anti else 1
    cols = np.array([expand_groups(labels, o[::-1] if rev else o) for o in gperms for rev in range(per)], dtype=np.int32)
    engine.set_precision(dtype)
    try:
        engine.load_data(*d, 0.0)
        unfolded = engine.run_batch(cols, False, want_lifts=True, accumulate=False)
        engine.set_players(labels)
        try:
            got, used = profiled_lifts(engine, gperms, anti)
        finally:
            engine.clear_players()
        assert engine.info() == 0
    finally:
        engine.set_precision("float64")
    print(f"fold of 257 groups {dtype} anti={anti}: {used['gather']} launch sequence(s)")
    assert used["gather"] == seqs and used["lift"] == 2 * seqs, used
    if seqs == 1:
        assert FOLD_SAMPLES * g > FOLD_GRID
    assert got.shape == (FOLD_SAMPLES, g) and np.all(np.isfinite(unfolded))
    np.testing.assert_array_equal(got, numpy_fold(unfolded, labels, g, per))


def test_report():
    """Not a check: the conditioning table for DESIGN.md."""
    for path, p, kappa, err, e_plain, r, ratio in _cond_rows:
        print(f"PAIRS table {path} p={p} kappa={kappa:g} err {err:.2e} e_plain {e_plain:.2e} r {r:.2f} pivot/thr {ratio:.3g}")
