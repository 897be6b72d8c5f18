"""tests/gram_cases.py has to reach what it was written for, and its truth has to be one, before
tests/test_gpu_gram_exact.py leans on either -- checked on the CPU.  The plans are the library's own
(lsspa_debug_gram_plan: gram_default_split and gram_plan of csrc/k_gram.hip): a case that stops reaching its target after
someone retunes the split fails here instead of passing silently on the GPU."""
import numpy as np
import pytest

import gram_cases as GC
from ls_spa._engine import debug_gram_plan

DEVICE_PLANS = [(c, debug_gram_plan(c[3], c[2])) for c in GC.CASES if c[6] == 0]


def _slice_rows(n, slices, rps):
    return [max(0, min(n, (k + 1) * rps) - k * rps) for k in range(slices)]


def test_case_names_are_unique_and_shapes_small():
    names = [c[0] for c in GC.CASES]
    assert len(names) == len(set(names))
    assert set(GC.FINALIZE_CASES) <= set(names)
    for name, dt, p, n, loc, extra, rows in GC.CASES:
        assert 1 <= n <= 1300 and 1 <= p <= 900 and n <= 2 ** 17, name     # a few MB a case; sums stay below 2^48
        assert dt in (GC.F64, GC.F32) and loc in (GC.HOST, GC.DEVICE) and extra >= 0
        assert rows == 0 or (loc == GC.HOST and rows % 16 == 0), name


def test_every_unit_class_and_tile_count_is_reached():
    plans = [pl for _, pl in DEVICE_PLANS]
    for cls in range(3):
        assert any(pl["cnt"][cls] > 0 for pl in plans), cls
    assert any(pl["cnt"][0] == 0 for pl in plans)                                # one or two tiles: no class-A unit
    assert any(pl["cnt"][0] > 0 and pl["cnt"][1] > 0 for pl in plans)            # classes A and B side by side
    assert any(pl["cnt"][1] == 0 and pl["nt"] > 1 for pl in plans)               # a full last tile
    assert {1, 2, 3, 6, 7} <= {pl["nt"] for pl in plans}
    assert any(pl["nt"] >= 6 and pl["nt"] % 2 == 1 for pl in plans)              # a "single" under split costs
    assert any(pl["nt"] >= 6 and pl["nt"] % 2 == 0 for pl in plans)
    assert {pl["xlive"] for pl in plans if pl["nt"] == 6} == set(range(1, 9))
    assert any(c[2] == 640 for c, _ in DEVICE_PLANS)                             # the last tile holds y alone
    assert any(c[2] == 767 and pl["xlive"] == 8 and pl["nt"] == 6 for c, pl in DEVICE_PLANS)   # y ends a full-width tile


@pytest.mark.parametrize("nt", [6, 7])
def test_three_slice_counts_with_ragged_last_slices(nt):
    """From six tiles on the classes have their own slice counts: some case per tile count has three different ones,
    every class's last live slice ends in a chunk of fewer than 16 rows, and some slice has whole chunks before it."""
    hits = 0
    for (name, dt, p, n, *_), pl in DEVICE_PLANS:
        if pl["nt"] != nt or len(set(pl["slices"])) != 3:
            continue
        rows = [[r for r in _slice_rows(n, pl["slices"][c], pl["rps"][c]) if r > 0] for c in range(3)]
        if all(r[-1] % 16 != 0 and r[-1] > 16 and len(r) > 1 for r in rows):
            hits += 1
    assert hits >= 2          # both dtypes


def test_rows_below_one_chunk():
    assert any(c[3] < 16 and pl["nt"] >= 6 for c, pl in DEVICE_PLANS)
    assert {c[3] for c, _ in DEVICE_PLANS if c[2] <= 4} >= {1, 15, 16, 17, 33}


def test_fp32_vector_residues_below_and_above_one_tile():
    """m = p mod 4 is the number of feature columns in the vector that holds column p (zfix_ragged); it runs only where a
    16-row chunk is whole (n >= 16) and p >= 4."""
    for lo, hi in ((1, 1), (2, 99)):
        got = {c[2] % 4 for c, pl in DEVICE_PLANS if c[1] == GC.F32 and c[2] >= 4 and c[3] >= 16 and lo <= pl["nt"] <= hi}
        assert got == {0, 1, 2, 3}, (lo, hi, got)
    assert {c[2] % 2 for c, pl in DEVICE_PLANS if c[1] == GC.F64 and c[2] >= 2 and c[3] >= 16} == {0, 1}
    # fewer features than one vector, and exactly one
    assert {(c[1], c[2]) for c, _ in DEVICE_PLANS if c[2] <= 4} == {(GC.F64, 1), (GC.F64, 2), (GC.F32, 1), (GC.F32, 2),
                                                                   (GC.F32, 3), (GC.F32, 4)}


def test_strided_cases():
    for p in (200, 641):
        for dt in (GC.F64, GC.F32):
            assert {c[5] for c in GC.CASES if c[2] == p and c[1] == dt and c[4] == GC.DEVICE and c[5]} == {1, 3, 24}
    assert any(c[4] == GC.HOST and c[5] > 0 for c in GC.CASES)
    assert debug_gram_plan(117, 200)["cnt"][1] > 0 and debug_gram_plan(117, 641)["nt"] == 6


def test_streamed_cases_reach_both_reduce_kernels_with_three_chunks():
    """launch_gram takes gram_reduce_small_kernel up to 3 tile pairs, gram_reduce_kernel beyond."""
    for small in (True, False):
        for dt in (GC.F64, GC.F32):
            seen = set()
            for name, d, p, n, loc, extra, rows in GC.CASES:
                nt = debug_gram_plan(n, p)["nt"]
                if rows == 0 or d != dt or (nt * (nt + 1) // 2 <= 3) != small:
                    continue
                plan = GC.chunk_plan(n, rows)
                assert len(plan) >= 3 and 1 <= plan[-1] <= 15, name
                seen.add(rows)
            assert seen == {16, 48, 256}, (small, dt, seen)


def test_plans_cover_their_rows():
    """rps * slices >= n for every class, or launch_gram refuses the launch."""
    for p in (1, 2, 3, 4, 5, 100, 127, 128, 200, 255, 257, 383, 640, 641, 767, 769, 895, 1000, 2000):
        for n in list(range(1, 70)) + [100, 255, 256, 257, 1003, 1291, 4097, 10 ** 4, 10 ** 5 + 3, 10 ** 6 + 1]:
            pl = debug_gram_plan(n, p)
            for c in range(3):
                assert pl["rps"][c] % 16 == 0 and pl["rps"][c] * pl["slices"][c] >= n, (p, n, pl)
            assert pl["cnt"][0] + pl["cnt"][1] == pl["nt"] * (pl["nt"] - 1) // 2 and pl["cnt"][2] == (pl["nt"] + 1) // 2


def test_plan_hook_refuses_bad_arguments():
    for n, p in ((0, 5), (-1, 5), (5, 0)):
        with pytest.raises(ValueError):
            debug_gram_plan(n, p)


@pytest.mark.parametrize("p,n", [(641, 1003), (100, 1291), (895, 117)])
def test_truth_is_exact_and_an_fp32_step_shows(p, n):
    """The fp64 BLAS product of the integer data equals the int64 product bit for bit; an fp32 product of the same data
    differs almost everywhere (products reach 2^30, fp32 carries 24 bits)."""
    X, y = GC.integer_data(GC.seed_of(f"truth{p}"), n, p, np.float64)
    want = GC.truth_int64(X, y)
    assert np.abs(want).max() < 2 ** 48
    got = GC.truth(X, y)
    np.testing.assert_array_equal(got, want.astype(np.float64))
    np.testing.assert_array_equal(got.astype(np.int64), want)
    X32, y32 = X.astype(np.float32), y.astype(np.float32)
    np.testing.assert_array_equal(GC.truth(X32, y32), got)          # fp32 storage holds the data exactly
    Z32 = np.concatenate([X32, y32[:, None]], axis=1)
    low = (Z32.T @ Z32).astype(np.float64)
    assert np.mean(low != got) > 0.9


def test_real_data_family():
    for dt, p, n in GC.REAL_CASES:
        X, y = GC.real_data(5, n, p, dt)
        Z = np.concatenate([X, y[:, None]], axis=1).astype(np.float64)
        assert np.isfinite(Z).all() and X.dtype == np.dtype(dt)
        m = np.abs(Z).mean(axis=0)
        assert m.max() / m.min() > 2.0 ** 79
        frac, _ = np.frexp(m / 1e6)
        assert np.all(np.abs(frac - 0.5) > 0.1)                     # no column scale near a power of two
