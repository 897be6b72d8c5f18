"""ls_spa_interactions: exact pairwise Shapley interaction values over all 2^p feature subsets -- CPU side.

An oracle of the interaction index written from its definition (the four-term difference over S without i and j, on the
subset values of tests/test_subsets_host.py), vetted by the identities the index must satisfy and against the fold over
subsets that the kernel uses; then the driver's plumbing through a test double whose enumeration is that oracle."""
import dataclasses
import os
import sys
from math import comb

import numpy as np
import pytest
import torch.multiprocessing as mp

import ls_spa as package
from ls_spa import InteractionResults, ShapleyResults, _driver, ls_spa, ls_spa_interactions
from test_subsets_host import SubsetsOracleEngine, data, exact_shapley, gram_problem, mask_bits, subset_values

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the test oracle -------------------------------------------------------------------------------------------------
def all_values(G, g, H, h, yy):
    p = len(g)
    masks = np.arange(1 << p, dtype=np.uint64)
    return subset_values(G, g, H, h, yy, masks), mask_bits(masks, p).sum(axis=1)


def exact_interactions(G, g, H, h, yy):
    """The raw index, I_ij = sum over S without i, j of |S|! (p - 2 - |S|)! / (p - 1)! (v(S+i+j) - v(S+i) - v(S+j) + v(S)),
    symmetric [p][p] with a zero diagonal."""
    p = len(g)
    v, size = all_values(G, g, H, h, yy)
    out = np.zeros((p, p))
    if p < 2:
        return out
    w2 = np.array([1.0 / ((p - 1) * comb(p - 2, s)) for s in range(p - 1)])
    masks = np.arange(1 << p, dtype=np.int64)
    for i in range(p):
        for j in range(i + 1, p):
            bi, bj = 1 << i, 1 << j
            S_ = masks[(masks & (bi | bj)) == 0]
            out[i, j] = out[j, i] = np.sum(w2[size[S_]] * (v[S_ | bi | bj] - v[S_ | bi] - v[S_ | bj] + v[S_]))
    return out


def shap_matrix(raw, phi):
    """SHAP's matrix from the raw index: I_ij / 2 off the diagonal, phi_i minus the rest of row i on it."""
    Phi = 0.5 * np.array(raw, dtype=np.float64)
    np.fill_diagonal(Phi, 0.0)
    np.fill_diagonal(Phi, np.asarray(phi) - Phi.sum(axis=1))
    return Phi


def folded_interactions(G, g, H, h, yy):
    """The same index by the fold over subsets K, k = |K| (csrc/k_subsets.hip):
    I_ij = T0 - T1_i - T1_j + T2_ij with weights gamma, beta + gamma, alpha + 2 beta + gamma."""
    p = len(g)
    v, size = all_values(G, g, H, h, yy)
    w2 = lambda s: 1.0 / ((p - 1) * comb(p - 2, s)) if 0 <= s <= p - 2 else 0.0
    al = np.array([w2(k - 2) for k in range(p + 1)])[size]
    be = np.array([w2(k - 1) for k in range(p + 1)])[size]
    ga = np.array([w2(k) for k in range(p + 1)])[size]
    bits = mask_bits(np.arange(1 << p, dtype=np.uint64), p)
    T0 = np.sum(ga * v)
    T1 = np.array([np.sum(((be + ga) * v)[bits[:, i]]) for i in range(p)])
    out = np.zeros((p, p))
    for i in range(p):
        for j in range(i + 1, p):
            out[i, j] = out[j, i] = T0 - T1[i] - T1[j] + np.sum(((al + 2 * be + ga) * v)[bits[:, i] & bits[:, j]])
    return out


@pytest.fixture(scope="module", params=[2, 3, 6, 9])
def case(request):
    p = request.param
    prob = gram_problem(*data(p, seed=40 + p), reg=0.05 * (p % 2))
    return p, prob, exact_interactions(*prob), exact_shapley(*prob)


def test_p2_is_the_four_term_difference():
    prob = gram_problem(*data(2, seed=42))
    v = subset_values(*prob, np.arange(4, dtype=np.uint64))
    assert abs(exact_interactions(*prob)[0, 1] - (v[3] - v[1] - v[2] + v[0])) < 1e-15


def test_oracle_is_symmetric_with_a_zero_diagonal(case):
    p, _, raw, _ = case
    np.testing.assert_array_equal(raw, raw.T)
    np.testing.assert_array_equal(np.diag(raw), np.zeros(p))
    assert np.abs(raw).max() > 1e-4


def test_oracle_rows_sum_to_the_attribution(case):
    p, prob, raw, phi = case
    Phi = shap_matrix(raw, phi)
    np.testing.assert_allclose(Phi.sum(axis=1), phi, rtol=0, atol=1e-14)
    v_full = subset_values(*prob, np.array([(1 << p) - 1], dtype=np.uint64))[0]
    assert abs(Phi.sum() - v_full) < 1e-13
    # the main effects are not a restatement of phi: sum_j I_ij / 2 is what separates them
    assert np.abs(np.diag(Phi) - phi).max() > 1e-4


def test_the_fold_over_subsets_reproduces_the_definition(case):
    _, prob, raw, _ = case
    np.testing.assert_allclose(folded_interactions(*prob), raw, rtol=0, atol=1e-13)


@pytest.mark.parametrize("p", [2, 3, 6, 9])
def test_an_additive_game_has_no_interactions(p):
    """Diagonal G and H: v(S) is a sum of per-feature terms, so every second difference vanishes."""
    rng = np.random.default_rng(p)
    G, H = np.diag(rng.uniform(0.5, 2.0, p)), np.diag(rng.uniform(0.5, 2.0, p))
    g, h = rng.standard_normal(p), rng.standard_normal(p)
    yy = 4.0 * float(h @ h)
    raw = exact_interactions(G, g, H, h, yy)
    assert np.abs(raw).max() <= 1e-14
    np.testing.assert_allclose(np.diag(shap_matrix(raw, exact_shapley(G, g, H, h, yy))),
                               exact_shapley(G, g, H, h, yy), rtol=0, atol=1e-14)


# ---- driver plumbing on a test double ----------------------------------------------------------------------------------
class InteractionsOracleEngine(SubsetsOracleEngine):
    """SubsetsOracleEngine with the interactions entry point, computed by the oracle above."""

    def __init__(self, info=0):
        super().__init__(info)
        self.interactions_calls = 0

    def subsets_interactions(self):
        self.interactions_calls += 1
        G, g, H, h = self.gram()
        prob = (G, g, H, h, self.y_norm_sq)
        return exact_shapley(*prob), exact_interactions(*prob), self._info


def test_result_fields_and_shapes():
    d = data(7, seed=4)
    eng = InteractionsOracleEngine()
    res = ls_spa_interactions(*d, _engine=eng)
    ref = ls_spa(*d, method="subsets", _engine=SubsetsOracleEngine())
    assert isinstance(res, InteractionResults)
    assert [f.name for f in dataclasses.fields(res)] == ["interactions", "attribution", "theta", "r_squared"]
    assert eng.interactions_calls == 1 and eng.subsets_calls == 0
    assert res.interactions.shape == (7, 7) and res.attribution.shape == (7,) and res.theta.shape == (7,)
    np.testing.assert_array_equal(res.attribution, ref.attribution)
    np.testing.assert_array_equal(res.theta, ref.theta)
    assert res.r_squared == ref.r_squared and isinstance(res.r_squared, float)
    prob = gram_problem(*d)
    np.testing.assert_allclose(res.interactions, shap_matrix(exact_interactions(*prob), exact_shapley(*prob)),
                               rtol=0, atol=1e-13)
    np.testing.assert_array_equal(res.interactions, res.interactions.T)
    np.testing.assert_allclose(res.interactions.sum(axis=1), res.attribution, rtol=0, atol=1e-14)
    assert abs(res.interactions.sum() - res.r_squared) < 1e-12
    assert "p = 7" in repr(res)


def test_ridge_reaches_the_engine():
    d = data(5, seed=6)
    res = ls_spa_interactions(*d, reg=0.3, _engine=InteractionsOracleEngine())
    prob = gram_problem(*d, reg=0.3)
    np.testing.assert_allclose(res.interactions, shap_matrix(exact_interactions(*prob), exact_shapley(*prob)),
                               rtol=0, atol=1e-13)


def test_p1():
    d = data(1, seed=1)
    res = ls_spa_interactions(*d, _engine=InteractionsOracleEngine())
    ref = ls_spa(*d, method="subsets", _engine=SubsetsOracleEngine())
    assert res.interactions.shape == (1, 1)
    np.testing.assert_array_equal(res.interactions, ref.attribution.reshape(1, 1))
    np.testing.assert_array_equal(res.attribution, ref.attribution)


def test_p33_refused_before_any_engine(monkeypatch):
    def no_engine(*a, **k):
        raise AssertionError("an engine was acquired")
    monkeypatch.setattr(_driver, "_acquire_engine", no_engine)
    with pytest.raises(ValueError, match="at most p = 32"):
        ls_spa_interactions(*data(33, n=80, m=50, seed=1))


def test_duplicated_column_warns():
    Xa, Xe, ya, ye = data(5, seed=2)
    Xa[:, 4], Xe[:, 4] = Xa[:, 1], Xe[:, 1]
    with pytest.warns(RuntimeWarning, match="not numerically positive definite"):
        with np.errstate(all="ignore"):
            ls_spa_interactions(Xa, Xe, ya, ye, _engine=InteractionsOracleEngine(info=1))


def test_kept_engine_back_to_float64():
    class Float32Engine(InteractionsOracleEngine):
        precision = "float32"

        def set_precision(self, dtype):
            self.precision = np.dtype(dtype).name

    eng = Float32Engine()
    ls_spa_interactions(*data(4, seed=3), _engine=eng)
    assert eng.precision == "float64"


def test_shapley_results_keeps_its_seven_fields():
    assert [f.name for f in dataclasses.fields(ShapleyResults)] == [
        "attribution", "theta", "overall_error", "attribution_errors", "r_squared", "error_history",
        "attribution_history"]


def test_public_names():
    assert "ls_spa_interactions" in package.__all__ and "InteractionResults" in package.__all__
    assert package.ls_spa_interactions is ls_spa_interactions


def _worker(rank, world, port, out_dir):
    for sub in ("ls-spa_amd", "oracle", "tests"):
        sys.path.insert(0, os.path.join(ROOT, sub))
    import torch.distributed as dist
    from ls_spa import ls_spa_interactions as run
    from ls_spa._dist import TorchComm
    from test_interactions_host import InteractionsOracleEngine as Eng
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    d = data(8, seed=8)
    whole = run(*d, _engine=Eng(), comm=TorchComm())
    shard = run(d[0][rank::world], d[1][rank::world], d[2][rank::world], d[3][rank::world], row_sharded=True,
                _engine=Eng(), comm=TorchComm())
    np.savez(os.path.join(out_dir, f"int{rank}.npz"), whole=whole.interactions, shard=shard.interactions,
             r2=shard.r_squared)
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_two_ranks_return_the_same_matrix(tmp_path):
    port = 33500 + (os.getpid() % 2000)
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    single = ls_spa_interactions(*data(8, seed=8), _engine=InteractionsOracleEngine())
    r0, r1 = (np.load(tmp_path / f"int{r}.npz") for r in (0, 1))
    np.testing.assert_array_equal(r0["whole"], r1["whole"])
    np.testing.assert_array_equal(r0["shard"], r1["shard"])
    np.testing.assert_allclose(r0["whole"], single.interactions, rtol=0, atol=1e-13)
    np.testing.assert_allclose(r0["shard"], single.interactions, rtol=0, atol=1e-11)
    assert abs(float(r0["r2"]) - single.r_squared) < 1e-11
