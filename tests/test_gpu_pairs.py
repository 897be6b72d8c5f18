"""ls_spa_interactions_sampled on the MI355X: the pair kernels of csrc/k_pairs.hip alone on chosen lift vectors against
the NumPy restatement (tests/pair_ref.py), the whole path -- three orderings a sample through the gather / Cholesky /
lift kernels, then the pair kernels -- against the CPU oracle on every kernel path, all orderings against the exact
enumeration, a 40-player additive game beyond the enumeration's limit against the definition, and what the pair calls
leave untouched."""
import itertools

import numpy as np
import pytest

import lsspa_oracle as O
import pair_ref
from ls_spa import LSSPANativeError, ls_spa, ls_spa_interactions, ls_spa_interactions_sampled
from ls_spa._driver import prepare_sampling
from test_groups_host import labels_of
from test_subsets_host import data, subset_values

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
MEAN_TOL = 2e-10        # twice the stated per-lift tolerance (README, tests/test_gpu_parity.py): a Delta is two lifts
LIFT_TOL = 1e-10
LIFT_TOL_F32 = 1e-4     # fp32 per-ordering work against fp64 (tests/test_gpu_group_sampling.py)
OFF = lambda d: ~np.eye(d, dtype=bool)      # noqa: E731


def load_identity(engine, d):
    """Any problem of dimension d: the pair kernels alone never factor an ordering."""
    engine.load_reduced(np.eye(d), np.full(d, 0.1), 1.0 + d, 1.0, H=np.eye(d), h=np.full(d, 0.1))


# ---- 1. the pair kernels alone ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 5, 257])
@pytest.mark.parametrize("d", [2, 3, 63, 64, 65, 129])
def test_pair_kernels_against_the_restatement(engine, d, B):
    """Integer lifts (|value| <= 2^10), two successive batches (the Chan merge runs), counts equal, mean within
    8 n eps max|Delta| and M2 within 8 n eps max|Delta|^2 of pair_ref (n the pair's count, max over the pair's own
    values: a rounding-count bound in the manner of tests/hp_stats.py), two runs bitwise equal."""
    rng = np.random.default_rng(1000 * d + B)
    batches = []
    for _ in range(2):
        perms = np.array([rng.permutation(d) for _ in range(B)], dtype=np.int32)
        batches.append((rng.integers(-1024, 1025, size=(3 * B, d)).astype(np.float64), perms))
    ref = pair_ref.PairTables(d)
    for lifts, perms in batches:
        ref.add_batch(lifts, perms)
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
    n, phi, count, mean, m2 = runs[0]
    assert n == 2 * B
    np.testing.assert_array_equal(count, ref.count)
    assert np.all(np.diag(count) == 0) and np.all(np.diag(mean) == 0) and np.all(np.diag(m2) == 0)
    np.testing.assert_array_equal(mean, mean.T)
    np.testing.assert_array_equal(m2, m2.T)
    mean_err, m2_err = np.abs(mean - ref.mean), np.abs(m2 - ref.m2)
    print(f"d = {d}, B = {B}: max |mean - ref| = {mean_err.max():.2e}, max |M2 - ref| = {m2_err.max():.2e}, "
          f"max count = {count.max()}")
    assert np.all(mean_err <= 8 * count * EPS * ref.max_abs)
    assert np.all(m2_err <= 8 * count * EPS * ref.max_abs ** 2)
    np.testing.assert_allclose(phi, ref.phi, rtol=0, atol=8 * 6 * B * EPS * 1024)      # 6 B integers a player, then / 6 B
    for a, b in zip(runs[0], runs[1]):
        np.testing.assert_array_equal(a, b)


# ---- 2. the whole path against the CPU oracle ------------------------------------------------------------------------
def golden_p12(golden):
    g = golden("p12")
    return tuple(g[k] for k in ("X_train", "X_test", "y_train", "y_test"))


ORACLE_CASES = {
    "p12_registers": lambda golden: golden_p12(golden),
    "p120_lds": lambda golden: data(120, n=400, m=300, seed=120),
    "p200_tri": lambda golden: data(200, n=600, m=400, seed=200),
    "p200_rect": lambda golden: data(200, n=600, m=150, seed=201),
}
_oracle_cache = {}


def oracle_case(name, golden):
    """(data, perms (8, p), pair_ref tables of the oracle's 24 lift vectors): computed once, shared, left unchanged."""
    if name not in _oracle_cache:
        d = ORACLE_CASES[name](golden)
        p = d[0].shape[1]
        rng = np.random.default_rng(p)
        perms = np.array([rng.permutation(p) for _ in range(8)], dtype=np.int32)
        red, yy = O.reduce(*d, 0.05), float(np.asarray(d[3]) @ np.asarray(d[3]))
        lifts = np.array([O.ordering_lift(*red, yy, r) for r in pair_ref.expand(perms)])
        _oracle_cache[name] = (d, perms, pair_ref.PairTables(p).add_batch(lifts, perms))
    return _oracle_cache[name]


def run_one_batch(engine, d, perms):
    engine.load_data(*d, 0.05)
    engine.full_fit()                 # from here on every batch's lifts are checked against the full R^2
    engine.pairs_enable(True)
    engine.pairs_batch(perms)
    out = engine.pairs_get()
    assert engine.info() & 12 == 0
    return out


@pytest.mark.parametrize("name", list(ORACLE_CASES))
def test_one_batch_against_the_oracle(engine, golden, name):
    d, perms, ref = oracle_case(name, golden)
    p = perms.shape[1]
    try:
        n, phi, count, mean, m2 = run_one_batch(engine, d, perms)
        assert engine.tri == (d[1].shape[0] >= p)
        again = None
        if name == "p200_tri":        # two lanes: the batch runs on a lane's own stream, the pair kernels behind it
            engine.set_lanes(2)
            engine.pairs_reset()
            engine.pairs_batch(perms)
            engine.pairs_batch(perms)      # ... and the next one on the other lane
            again = engine.pairs_get()
    finally:
        engine.set_lanes(1)
        engine.pairs_enable(False)
    assert n == 8
    np.testing.assert_array_equal(count, ref.count)
    err = np.abs(mean - ref.mean).max()
    print(f"{name}: max |mean Delta - oracle| = {err:.2e}, max |phi - oracle| = {np.abs(phi - ref.phi).max():.2e}")
    assert err <= MEAN_TOL
    np.testing.assert_allclose(phi, ref.phi, rtol=0, atol=LIFT_TOL)
    if again is not None:
        assert again[0] == 16
        np.testing.assert_array_equal(again[2], 2 * count)
        np.testing.assert_allclose(again[3], mean, rtol=0, atol=1e-15)      # the same values twice: the same mean
        np.testing.assert_allclose(again[1], phi, rtol=0, atol=1e-14)


# ---- 6. fp32 per-ordering work ---------------------------------------------------------------------------------------
def test_fp32_agrees_with_fp64(engine, golden):
    d, perms, _ = oracle_case("p120_lds", golden)
    try:
        _, phi, count, mean, _ = run_one_batch(engine, d, perms)
        engine.set_precision("float32")
        engine.pairs_reset()
        engine.pairs_batch(perms)
        _, phi32, count32, mean32, _ = engine.pairs_get()
    finally:
        engine.set_precision("float64")
        engine.pairs_enable(False)
    np.testing.assert_array_equal(count32, count)
    print(f"fp32: max |mean - fp64| = {np.abs(mean32 - mean).max():.2e}, max |phi - fp64| = {np.abs(phi32 - phi).max():.2e}")
    assert np.abs(mean32 - mean).max() <= 2 * LIFT_TOL_F32
    assert np.abs(phi32 - phi).max() <= 2 * LIFT_TOL_F32
    assert np.abs(mean32 - mean).max() > 0          # it did run in fp32


# ---- 3. all orderings against the enumeration ------------------------------------------------------------------------
def test_all_orderings_equal_the_enumeration():
    d = data(6, seed=66)
    perms = np.array(list(itertools.permutations(range(6))), dtype=np.int32)
    got = ls_spa_interactions_sampled(*d, perms=perms, batch_size=256)
    ref = ls_spa_interactions(*d)
    print(f"p = 6: max |sampled over 720 orderings - enumeration| = {np.abs(got.interactions - ref.interactions).max():.2e}")
    np.testing.assert_allclose(got.interactions, ref.interactions, rtol=0, atol=1e-10)
    np.testing.assert_allclose(got.attribution, ref.attribution, rtol=0, atol=1e-10)
    assert got.n_samples == 720 and np.all(got.counts[OFF(6)] == 240) and np.all(np.diag(got.counts) == 0)
    np.testing.assert_allclose(got.interactions.sum(axis=1), got.attribution, rtol=0, atol=1e-13)
    assert abs(got.interactions.sum() - got.r_squared) < 1e-10
    assert got.r_squared == ref.r_squared
    np.testing.assert_array_equal(got.theta, ref.theta)


def test_all_group_orderings_equal_the_grouped_enumeration():
    labels = labels_of([2] * 5, 2, seed=5)
    assert len(labels) == 12
    d = data(12, seed=67)
    perms = np.array(list(itertools.permutations(range(5))), dtype=np.int32)
    got = ls_spa_interactions_sampled(*d, perms=perms, groups=labels, batch_size=64)
    ref = ls_spa_interactions(*d, groups=labels)
    print(f"g = 5, p = 12: max |sampled over 120 orderings - enumeration| = "
          f"{np.abs(got.interactions - ref.interactions).max():.2e}")
    np.testing.assert_allclose(got.interactions, ref.interactions, rtol=0, atol=1e-10)
    np.testing.assert_allclose(got.attribution, ref.attribution, rtol=0, atol=1e-10)
    assert got.n_samples == 120 and np.all(got.counts[OFF(5)] == 48) and got.theta.shape == (12,)


# ---- 4. beyond the exact limit: an additive game of five blocks of eight ------------------------------------------------
BLOCKS, WIDTH, BLOCK_SEED, BLOCK_SAMPLES = 5, 8, 7, 4096
_block_cache = {}


def block_game():
    """Block-diagonal reduced problem (d = 40): G, g, aug, H, h, yy, the 2^8 table of every block's own game, the
    driver's seeded 'random' orderings and pair_ref's tables of the game's exact lifts for them."""
    if not _block_cache:
        rng = np.random.default_rng(40)
        d = BLOCKS * WIDTH
        G, H, g, h = np.zeros((d, d)), np.zeros((d, d)), np.zeros(d), np.zeros(d)
        y, ye = rng.standard_normal(200), rng.standard_normal(150)
        for c in range(BLOCKS):
            sl = slice(c * WIDTH, (c + 1) * WIDTH)
            Xa, Xe = rng.standard_normal((200, WIDTH)), rng.standard_normal((150, WIDTH))
            w = rng.standard_normal(WIDTH)
            y, ye = y + Xa @ w, ye + Xe @ w
            G[sl, sl], H[sl, sl] = Xa.T @ Xa / 200, Xe.T @ Xe
            g[sl], h[sl] = Xa.T @ y / 200, Xe.T @ ye
        yy = float(ye @ ye)
        aug = max(float(y @ y) / 200, 1.1 * float(g @ np.linalg.solve(G, g)))
        masks = np.arange(1 << WIDTH, dtype=np.uint64)
        tables = []
        for c in range(BLOCKS):
            sl = slice(c * WIDTH, (c + 1) * WIDTH)
            tables.append(subset_values(G[sl, sl], g[sl], H[sl, sl], h[sl], yy, masks))
        src = prepare_sampling(d, max_samples=BLOCK_SAMPLES, batch_size=256, seed=BLOCK_SEED, perms=None,
                               antithetical=False, method="random")[1]
        perms = np.asarray(src.take(BLOCK_SAMPLES), dtype=np.int32)
        rows = pair_ref.expand(perms)
        lifts = np.empty(rows.shape)
        mask = np.zeros((len(rows), BLOCKS), dtype=np.int64)
        at = np.arange(len(rows))
        vt = np.array(tables)
        for k in range(d):
            j = rows[:, k]
            c, bit = j // WIDTH, 1 << (j % WIDTH)
            lifts[at, j] = vt[c, mask[at, c] | bit] - vt[c, mask[at, c]]
            mask[at, c] |= bit
        _block_cache["v"] = (G, g, aug, H, h, yy, tables, perms, pair_ref.PairTables(d).add_batch(lifts, perms))
    return _block_cache["v"]


def check_block_game(count, mean, m2, tables, what):
    d = BLOCKS * WIDTH
    block = np.arange(d) // WIDTH
    same = (block[:, None] == block[None, :]) & OFF(d)
    cross = block[:, None] != block[None, :]
    truth = np.zeros((d, d))
    for c in range(BLOCKS):
        sl = slice(c * WIDTH, (c + 1) * WIDTH)
        truth[sl, sl] = pair_ref.interaction_index(tables[c], WIDTH)
    se = np.sqrt(m2[same] / (count[same] * (count[same] - 1.0)))
    dev = np.abs(mean[same] - truth[same]) / se
    print(f"{what}: cross-block max |mean| = {np.abs(mean[cross]).max():.2e}, within-block min count = "
          f"{count[same].min()}, largest deviation = {dev.max():.2f} standard errors")
    assert np.abs(mean[cross]).max() <= MEAN_TOL
    assert count[same].min() >= 100
    assert np.all(np.abs(mean[same] - truth[same]) <= 5 * se)      # every within-block pair


def test_block_game_beyond_the_exact_limit(engine):
    G, g, aug, H, h, yy, tables, perms, ref = block_game()
    check_block_game(ref.count, ref.mean, ref.m2, tables, "CPU, the driver's seeded orderings")      # before the GPU run
    engine.load_reduced(G, g, aug, yy, H=H, h=h)
    engine.full_fit()
    engine.pairs_enable(True)
    try:
        for s in range(0, BLOCK_SAMPLES, 256):
            engine.pairs_batch(perms[s:s + 256])
        n, phi, count, mean, m2 = engine.pairs_get()
        assert engine.info() & 12 == 0
    finally:
        engine.pairs_enable(False)
    assert n == BLOCK_SAMPLES
    np.testing.assert_array_equal(count, ref.count)
    check_block_game(count, mean, m2, tables, "GPU")
    np.testing.assert_allclose(phi.sum(), sum(t[-1] for t in tables), rtol=0, atol=1e-10)


# ---- 5. isolation ----------------------------------------------------------------------------------------------------
def test_pair_calls_leave_the_sampling_path_alone(engine):
    d = data(150, n=600, m=400, seed=15)
    kw = dict(method="argsort", seed=7, max_samples=64, batch_size=32, tolerance=0.0, lanes=1, _engine=engine)
    before = ls_spa(*d, **kw)
    stats0, info0 = engine.stats(), engine.info()
    rng = np.random.default_rng(5)
    perms = np.array([rng.permutation(150) for _ in range(8)], dtype=np.int32)
    engine.pairs_enable(True)
    try:
        engine.pairs_batch(perms)
        n, phi, count, _, _ = engine.pairs_get()
        assert n == 8 and count.sum() == 2 * 8 * 149 and abs(phi.sum() - before.r_squared) < 1e-9
        stats1, info1 = engine.stats(), engine.info()
        assert stats1[0] == stats0[0] and info1 == info0
        np.testing.assert_array_equal(stats1[1], stats0[1])
        np.testing.assert_array_equal(stats1[2], stats0[2])
        # a launched batch that nobody collected: refused, and the batch is still the caller's to collect
        ticket = engine.launch_batch(perms, False)
        with pytest.raises(LSSPANativeError, match="status 3"):
            engine.pairs_batch(perms)
        engine.discard_batch(ticket)
        engine.pairs_batch(perms)
        assert engine.pairs_get(tables=False)[0] == 16
        # the state belongs to the dimension it was enabled at
        engine.set_players(np.arange(150, dtype=np.int32) // 2)
        with pytest.raises(LSSPANativeError, match="status 3"):
            engine.pairs_batch(perms[:, :75] // 2)
        engine.clear_players()
        with pytest.raises(LSSPANativeError, match="status 3"):
            engine.pairs_get()
        engine.pairs_enable(True)
        engine.load_reduced(np.eye(150), np.full(150, 0.1), 200.0, 1.0, H=np.eye(150), h=np.full(150, 0.1))
        with pytest.raises(LSSPANativeError, match="status 3"):
            engine.pairs_batch(perms)
    finally:
        engine.clear_players()
        engine.pairs_enable(False)
        engine.load_data(*d, 0.0)
        engine.history_enable(0)
    after = ls_spa(*d, **kw)
    np.testing.assert_array_equal(before.attribution, after.attribution)
    np.testing.assert_array_equal(before.error_history, after.error_history)
    np.testing.assert_array_equal(before.attribution_errors, after.attribution_errors)


def test_dimension_limits_of_the_library(engine):
    load_identity(engine, 1)
    with pytest.raises(ValueError, match="LSSPA_PAIRS_MAX_D = 4096"):
        engine.pairs_enable(True)
