"""The host side of ls_spa_bootstrap, without a GPU: the NumPy restatement of the row draws (tests/boot_ref.py), the
summary logic of BootstrapResults on hand-made replicates, the argument checks that need no engine, the block planner
(lsspa_debug_boot_plan) and the export."""
import numpy as np
import pytest

import boot_ref
import ls_spa as package
from ls_spa import BootstrapResults, ls_spa_bootstrap
from ls_spa._driver import _bootstrap_options
from ls_spa._engine import debug_boot_plan
from test_subsets_host import data


def test_bootstrap_is_exported():
    assert "ls_spa_bootstrap" in package.__all__ and "BootstrapResults" in package.__all__
    assert callable(package.ls_spa_bootstrap)


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1000])
def test_count_reference_against_bincount_of_its_own_indices(n):
    for seed, r, side in ((42, 0, 0), (42, 0, 1), (7, 2 ** 31, 0), (2 ** 64 - 1, 2 ** 40 + 3, 1)):
        idx = boot_ref.indices(seed, r, side, n)
        assert idx.shape == (n,) and idx.min() >= 0 and idx.max() < n
        cnt = boot_ref.counts(seed, r, side, n)
        np.testing.assert_array_equal(cnt, np.bincount(idx, minlength=n))
        assert cnt.sum() == n and cnt.dtype == np.uint32
    if n == 1000:
        a, b = boot_ref.counts(42, 0, 0, n), boot_ref.counts(42, 0, 1, n)
        assert not np.array_equal(a, b) and not np.array_equal(a, boot_ref.counts(42, 1, 0, n))
        # a bootstrap sample leaves about 1 / e of the rows out
        assert 0.30 < (a == 0).mean() < 0.43


def test_count_reference_uses_word_k_for_draw_4j_plus_k():
    from philox_ref import philox4x32_10
    n, seed, r = 10, 5, 3
    w = philox4x32_10(np.array([[2, 1, r, 0]], dtype=np.uint64), (seed, 0))[0]
    assert boot_ref.indices(seed, r, 1, n)[8:10].tolist() == [int(w[0]) * n >> 32, int(w[1]) * n >> 32]


def test_results_summaries_on_hand_made_replicates():
    rep = np.array([[1.0, 5.0, 2.0], [2.0, 4.0, 2.0], [9.0, 9.0, 9.0], [3.0, 3.0, 2.5], [4.0, 2.0, 3.0]])
    r2 = rep.sum(axis=1)
    failed = np.array([False, False, True, False, False])
    res = BootstrapResults.from_replicates(np.zeros(3), np.ones(3), 0.5, rep, r2, failed, confidence=0.5)
    ok = rep[~failed]
    assert res.n_failed == 1 and np.isnan(res.replicates[2]).all() and np.isnan(res.r_squared_replicates[2])
    np.testing.assert_array_equal(res.replicates[~failed], ok)
    np.testing.assert_array_equal(res.lower, np.quantile(ok, 0.25, axis=0))
    np.testing.assert_array_equal(res.upper, np.quantile(ok, 0.75, axis=0))
    np.testing.assert_array_equal(res.std_error, ok.std(axis=0, ddof=1))
    assert res.r_squared_interval == (np.quantile(r2[~failed], 0.25), np.quantile(r2[~failed], 0.75))
    # feature 0 beats feature 1 in one of the four valid replicates (4 > 2), ties in one (3 == 3)
    assert res.prob_greater[0, 1] == 0.25 and res.prob_greater[1, 0] == 0.5
    assert res.prob_greater[0, 2] == 0.5 and res.prob_greater[2, 0] == 0.25      # ties at 2 == 2: neither
    assert np.all(np.diag(res.prob_greater) == 0.0)
    assert rep[2, 0] == 9.0                                # the caller's array is not written
    assert "4 bootstrap" not in repr(res) and "5 bootstrap replicates (1 failed)" in repr(res)
    with pytest.raises(RuntimeError, match="3 of 5"):
        BootstrapResults.from_replicates(np.zeros(3), np.ones(3), 0.5, rep, r2, [True, True, True, False, False])
    none = BootstrapResults.from_replicates(np.zeros(3), np.ones(3), 0.5, rep, r2, np.zeros(5, dtype=bool))
    assert none.n_failed == 0 and none.confidence == 0.95
    np.testing.assert_array_equal(none.upper, np.quantile(rep, 1.0 - (1.0 - 0.95) / 2.0, axis=0))


def test_argument_checks_need_no_engine():
    d = data(4, n=30, m=20, seed=1)

    class NoEngine:
        def __getattr__(self, name):
            raise AssertionError(f"the engine was asked for {name} before the arguments were checked")

    def call(*a, **k):
        return ls_spa_bootstrap(*a, _engine=NoEngine(), **k)

    with pytest.raises(ValueError, match="at most p = 32.*group the columns"):
        call(*data(33, n=40, m=40, seed=1))
    for kw, what in ((dict(n_boot=1), "n_boot"), (dict(n_boot=2.5), "n_boot"), (dict(confidence=1.0), "confidence"),
                     (dict(confidence=0.0), "confidence"), (dict(resample=()), "resample"),
                     (dict(resample=("train", "valid")), "resample"), (dict(resample=("test", "test")), "resample"),
                     (dict(weights=(None,)), "pair"), (dict(n_boot=3, weights=(np.ones((3, 29)), None)), "w_train"),
                     (dict(n_boot=3, weights=(None, -np.ones((3, 20)))), "w_test must be finite and >= 0"),
                     (dict(n_boot=3, weights=(np.full((3, 30), np.nan), None)), "w_train must be finite"),
                     (dict(n_boot=3, weights=(np.zeros((3, 30)), None)), "replicate 0 sum to zero")):
        with pytest.raises(ValueError, match=what):
            call(*d, **kw)
    with pytest.raises(Exception, match="same number of columns"):
        call(d[0], d[1][:, :3], d[2], d[3])                 # validate_data's own refusal
    wa, we, sides = _bootstrap_options(3, 0.9, (None, np.ones((3, 20), dtype=np.float32)), "train", 30, 20)
    assert wa is None and we.dtype == np.float64 and sides == ("train",)


def test_block_planner():
    """Blocks by memory, not by R: the bytes of a block stay under 256 MB, R only sets the number of blocks; the slices
    depend on the rows alone."""
    small = debug_boot_plan(1000, 10 ** 4, 10 ** 4, 12)
    assert small["cb"] == 1 and small["rpw"] == 4 and small["block"] * small["rep_bytes"] <= 256 << 20
    assert small["n_blocks"] == -(-1000 // small["block"]) and small["slices_train"] * small["rps_train"] >= 10 ** 4
    big = debug_boot_plan(10 ** 6, 10 ** 5, 10 ** 5, 24)
    assert big["block"] == debug_boot_plan(10 ** 3, 10 ** 5, 10 ** 5, 24)["block"] and big["n_blocks"] > 1000
    assert big["block"] * big["rep_bytes"] <= 256 << 20 and big["slices_train"] <= 128 and big["rps_train"] % 4 == 0
    for R in (1, 7, 10 ** 4):
        for block in (0, 1, 3, 10 ** 6):
            a = debug_boot_plan(R, 513, 77, 16, block)
            assert (a["slices_train"], a["rps_train"], a["slices_test"], a["rps_test"]) == (3, 256, 1, 256)
            assert 1 <= a["block"] <= min(R, 1024) and (block == 0 or a["block"] <= block)
            assert a["units"] * a["enum_reps"] <= 1 << 20 and a["enum_reps"] <= a["block"]
    huge = debug_boot_plan(5, 2 ** 31 - 1, 2 ** 31 - 1, 32)        # one replicate does not fit the bound: one a block
    assert huge["block"] == 1 and huge["cb"] == 3 and huge["rpw"] == 2 and huge["slices_train"] == 128
    assert huge["per"] * huge["units"] == 1 << 26 and huge["steps"] * huge["units"] == 1 << 20
    for bad in ((0, 5, 5, 3, 0), (1, 0, 5, 3, 0), (1, 5, 2 ** 31, 3, 0), (1, 5, 5, 33, 0), (1, 5, 5, 0, 0), (1, 5, 5, 3, -1)):
        with pytest.raises(ValueError):
            debug_boot_plan(*bad)
