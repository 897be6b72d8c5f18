"""The table of tests/loader_cases.py reaches what tests/test_gpu_row_loaders.py needs it to reach (no GPU): every
(family, dtype, location) cell, the feature counts on both sides of every step of the packed widths, the row counts, the
strides, the chunk counts of the streamed cases under the constant of load_rows, and data on which every sum is exact."""
import numpy as np
import pytest

import loader_cases as LC

BY_FAMILY = {f: [c for c in LC.CASES if c.family == f] for f in LC.FAMILIES}


def test_every_cell_of_every_family_is_occupied_with_and_without_padding():
    for f in LC.FAMILIES:
        for dt, loc in LC.CELLS:
            cell = [c for c in BY_FAMILY[f] if (c.dtype, c.location) == (dt, loc)]
            assert cell, (f, dt, loc)
            assert any(c.ld_extra_train and c.ld_extra_test for c in cell), (f, dt, loc)
            assert any(c.ld_extra_train == 0 for c in cell) and any(c.ld_extra_test == 0 for c in cell), (f, dt, loc)
            # every shape of the family in every cell
            assert {LC.shape_of(c) for c in cell} >= {LC.shape_of(c) for c in BY_FAMILY[f]
                                                      if c not in LC.STREAMED}, (f, dt, loc)
    assert len({LC.name(c) for c in LC.CASES}) == len(LC.CASES)


def test_feature_counts_straddle_every_step_of_the_packed_widths():
    def ldz(p):
        return 16 * ((p + 16) // 16)         # boot_plan: cb = (p + 16) / 16 column blocks of [X | y]

    def ldx(p):
        return 16 * ((p + 15) // 16)         # perm_plan: cb = ceil(p / 16) column blocks of X

    have = {f: {c.p for c in BY_FAMILY[f]} for f in LC.FAMILIES}
    assert have["boot"] >= {1, 15, 16, 17, 32} and max(have["boot"]) == 32
    assert have["boot_groups"] >= {33, 47, 48, 63, 64} and max(have["boot_groups"]) == 64
    assert have["perm"] >= {1, 16, 17, 32, 33, 48, 49, 64} and max(have["perm"]) == 64
    assert have["multi"] == {1, 7, 32} and have["multi_lift"] == {1, 16, 104}
    boot = have["boot"] | have["boot_groups"]
    for lo in (15, 31, 47, 63):              # every step of ldz up to p = 64
        assert ldz(lo) + 16 == ldz(lo + 1) and {lo, lo + 1} <= boot | {31}, lo
    assert ldz(31) == 32 and ldz(32) == 48 and {17, 32} <= boot      # 31 | 32: 17 and 32 are on its two sides
    assert {ldz(p) for p in boot} == {16, 32, 48, 64, 80}
    for lo in (16, 32, 48):                  # every step of ldx
        assert ldx(lo) + 16 == ldx(lo + 1) and {lo, lo + 1} <= have["perm"], lo
    assert {ldx(p) for p in have["perm"]} == {16, 32, 48, 64}
    for f in ("multi", "multi_lift"):
        assert {(c.p, c.m) for c in BY_FAMILY[f]} == {(p, m) for p in LC.P_AXIS[f] for m in LC.M_AXIS}
    # perm_run without labels up to the largest enumeration the cases afford, with labels beyond
    for p in have["perm"]:
        assert (LC.perm_labels(p) is None) == (p <= 17)
        if p > 17:
            assert set(LC.perm_labels(p)) == set(range(LC.PERM_GROUPS)) and LC.PERM_GROUPS <= 8


def test_row_counts():
    for f in LC.FAMILIES:
        for c in BY_FAMILY[f]:
            assert c.N != c.M and c.N >= 1 and c.M >= 1, LC.name(c)
        assert {c.N for c in BY_FAMILY[f]} >= set(LC.N_AXIS), f
        if f != "multi_lift":
            assert {c.M for c in BY_FAMILY[f]} >= set(LC.N_AXIS), f
    # lsspa_multi_lift_load refuses M < p: the test side is as short as it may be at p = 104, and on the axis otherwise
    for c in BY_FAMILY["multi_lift"]:
        assert c.M >= c.p and (c.M in LC.N_AXIS or c.M == c.p == 104), LC.name(c)
    assert any(c.M == c.p for c in BY_FAMILY["multi_lift"])
    # three row slices of the bootstrap's Gram kernel, the last of one row, in every cell
    assert {(c.dtype, c.location) for c in BY_FAMILY["boot"] if c.N == LC.N_SLICES and c not in LC.STREAMED} == set(LC.CELLS)


def test_strides():
    for c in LC.CASES:
        a, b = c.ld_extra_train, c.ld_extra_test
        assert a >= 0 and b >= 0 and (a != b or a == b == 0), LC.name(c)
        (ld_a, ldy_a), (ld_e, ldy_e) = LC.strides(c)
        assert ld_a >= c.p and ld_e >= c.p and ldy_a >= c.m and ldy_e >= c.m
        if c.family in ("multi", "multi_lift"):
            assert c.ldy_extra in LC.LDY_EXTRA and (ldy_a - c.m != ldy_e - c.m or c.ldy_extra == 0), LC.name(c)
        else:
            assert c.ldy_extra == 0 and c.m == 1 and ldy_a == ldy_e == 1
        if c not in LC.STREAMED:
            assert a in LC.LD_EXTRA and b in LC.LD_EXTRA, LC.name(c)
        b0 = LC.baseline(c)
        assert LC.shape_of(b0) == LC.shape_of(c) and LC.strides(b0) == ((c.p, c.m if c.family in ("multi", "multi_lift") else 1),) * 2
    for f in LC.FAMILIES:
        for dt, loc in LC.CELLS:
            cell = [c for c in BY_FAMILY[f] if (c.dtype, c.location) == (dt, loc) and c not in LC.STREAMED]
            assert {c.ld_extra_train for c in cell} | {c.ld_extra_test for c in cell} == set(LC.LD_EXTRA), (f, dt, loc)
            if f in ("multi", "multi_lift"):
                assert {c.ldy_extra for c in cell} == set(LC.LDY_EXTRA), (f, dt, loc)
                # the column copies of Y: none beside X at m = 1, m - 1 > 0 of them otherwise, both with ldy > m
                assert any(c.m == 1 and c.ldy_extra for c in cell) and any(c.m > 1 and c.ldy_extra for c in cell)


@pytest.mark.parametrize("family", LC.FAMILIES)
@pytest.mark.parametrize("location", [LC.HOST, LC.DEVICE], ids=["host", "device"])
def test_float32_rows_that_are_4_byte_but_not_8_byte_aligned(family, location):
    """An odd float32 stride: every other row starts 4 bytes off an 8-byte boundary (the base of an allocation is
    aligned to more).  On both sides, with more than one row."""
    for side in range(2):
        odd = [c for c in BY_FAMILY[family] if c.dtype == LC.F32 and c.location == location
               and LC.strides(c)[side][0] % 2 == 1 and (c.N, c.M)[side] >= 2]
        assert odd, (family, location, side)
    if family in ("multi", "multi_lift"):
        assert any(c.dtype == LC.F32 and c.location == location and LC.strides(c)[0][1] % 2 == 1 and c.N >= 2
                   for c in BY_FAMILY[family])


def test_streamed_cases_cross_the_chunk_constant():
    assert LC.CHUNK_BYTES == 64 << 20
    assert {c.family for c in LC.STREAMED} == set(LC.ROW_LOADED)
    for f in LC.ROW_LOADED:
        assert {(c.dtype, c.N) for c in LC.STREAMED if c.family == f} == set(LC.STREAMED_CLAIMS), f
    for c in LC.STREAMED:
        ld = LC.strides(c)[0][0]
        assert c.location == LC.HOST and ld == 32768
        assert LC.chunk_rows(ld, c.dtype) == (256 if c.dtype == LC.F64 else 512)
        plan = LC.chunk_plan(c.N, ld, c.dtype)
        assert plan == LC.STREAMED_CLAIMS[(c.dtype, c.N)], LC.name(c)
        assert len(plan) >= 2 and plan[-1] == 1 and sum(plan) == c.N
        # the test side: one chunk, another stride
        ld_e = LC.strides(c)[1][0]
        assert ld_e != ld and ld_e > c.p and LC.chunk_plan(c.M, ld_e, c.dtype) == [c.M]
        # a row fewer is a chunk fewer (or no one-row chunk): no smaller N does what this one does
        assert LC.chunk_plan(c.N - 1, ld, c.dtype)[-1] != 1
    assert max(len(LC.chunk_plan(c.N, LC.strides(c)[0][0], c.dtype)) for c in LC.STREAMED) == 3
    # every other host case is one chunk a side
    for c in LC.CASES:
        if c.location == LC.HOST and c not in LC.STREAMED:
            assert LC.chunk_plan(c.N, LC.strides(c)[0][0], c.dtype) == [c.N]


def test_every_sum_is_exact_and_every_input_a_float32():
    seen = {}
    for c in LC.CASES:
        if LC.shape_of(c) in seen:
            continue
        sides = LC.case_data(c)
        seen[LC.shape_of(c)] = True
        for (X, Y), n in zip(sides, (c.N, c.M)):
            assert X.shape == (n, c.p) and Y.shape == (n, c.m) and X.dtype == Y.dtype == np.float64
            Z = np.concatenate([X, Y], axis=1)
            assert np.array_equal(Z, np.round(Z)) and np.abs(Z).max() < 2 ** 24
            assert np.array_equal(Z.astype(np.float32).astype(np.float64), Z)
            A = np.abs(Z).astype(np.int64)
            assert (A.T @ A).max() < 2 ** 53           # bounds every partial sum of every entry, in any order
            assert np.array_equal(LC.truth_int64(X, Y).astype(np.float64), Z.T @ Z)
        # a response that is identically zero on the test side is refused by the loads
        assert np.all(np.any(sides[1][1] != 0, axis=0)), LC.name(c)
    # the two sides of a shape, and two shapes, do not share their values
    c = LC.CASES[0]
    (Xa, _), (Xe, _) = LC.case_data(c)
    assert not np.array_equal(Xa[:1], Xe[:1])


def test_variants_of_a_shape_share_their_data_and_the_reduced_truth_is_what_the_host_code_computes():
    c = next(c for c in LC.CASES if LC.reg_of(c) and c.family == "multi")
    others = [d for d in LC.CASES if LC.shape_of(d) == LC.shape_of(c)]
    assert {(d.dtype, d.location) for d in others} == set(LC.CELLS)
    for d in others:
        for s, t in zip(LC.case_data(c), LC.case_data(d)):
            assert np.array_equal(s[0], t[0]) and np.array_equal(s[1], t[1])
    (Xa, Ya), (Xe, Ye) = LC.case_data(c)
    G, g, H, h, yy = LC.reduced_truth(c, LC.truth_int64(Xa, Ya), LC.truth_int64(Xe, Ye))
    assert G.shape == H.shape == (c.p, c.p) and g.shape == h.shape == (c.m, c.p) and yy.shape == (c.m,)
    np.testing.assert_allclose(G, Xa.T @ Xa / c.N + LC.REG * np.eye(c.p), rtol=1e-15)
    np.testing.assert_allclose(g, (Xa.T @ Ya).T / c.N, rtol=1e-15)
    assert np.array_equal(H, Xe.T @ Xe) and np.array_equal(h, (Xe.T @ Ye).T) and np.array_equal(yy, (Ye * Ye).sum(axis=0))
    assert {(f, p, m) for f, p, m in LC.REG_SHAPES} <= {(d.family, d.p, d.m) for d in LC.CASES}
    assert {f for f, _, _ in LC.REG_SHAPES} == set(LC.GRAM_LOADED)
