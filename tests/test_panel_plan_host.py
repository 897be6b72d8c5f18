"""tests/panel_cases.py has to reach what it was written for before tests/test_gpu_panel_edges.py leans on it -- checked on
the CPU.  The plans are the library's own (lsspa_debug_panel_plan: panel_plan of csrc/k_factor.hip, the function
launch_chol2_panel takes its decisions from, under run_slice's shape rules): a case that stops reaching its class after
someone retunes `grouped` or `xlast` fails here instead of passing silently on the GPU.

COVERAGE CONDITION: every class below is reached by at least one case of the table, with the plan the library gives it
today; dropping the last case of a class, or changing a rule so that the case leaves it, fails a test of this file."""
import numpy as np
import pytest

import panel_cases as PC
from ls_spa._engine import debug_panel_plan, debug_panel_plan_launch


def plan_of(c):
    return debug_panel_plan(c.p, PC.n_ord_of(c), PC.is_tri(c), c.flags)


PLANS = [(c, plan_of(c)) for c in PC.CASES]


def launches(pred=lambda c: True):
    return [(c, pl, ln) for c, pl in PLANS if pred(c) for ln in pl["launches"]]


def round_up(x, q):
    return (x + q - 1) // q * q


def test_case_names_are_unique_and_shapes_small():
    names = [c.name for c in PC.CASES]
    assert len(names) == len(set(names))
    for c in PC.CASES:
        assert 1 <= c.p <= 513 and c.n == 2 * c.p + 40 and 1 <= c.B <= PC.N_ORDERS, c.name
        assert c.m == c.p + 50 or c.m < c.p, c.name
        assert c.dtype in (PC.F64, PC.F32) and c.flags & ~(128 | 512 | 1024) == 0, c.name
        # the general path has to run: fp64 tri mode below one panel needs developer flag 1024
        small = PC.is_tri(c) and c.dtype == PC.F64 and c.p <= PC.SMALL_P_MAX
        assert bool(c.flags & 1024) == small, c.name
    assert len(PC.CASES) <= 200


def test_the_shape_rules_are_the_engines():
    for c, pl in PLANS:
        tri = PC.is_tri(c)
        assert pl["p_pad"] == round_up(c.p + 1, 128), c.name
        assert pl["n_mats"] == (2 if tri else 1) * PC.n_ord_of(c), c.name
        vt = tri and not c.flags & 128
        assert len(pl["launches"]) == pl["p_pad"] // 128 - 1 + (1 if vt else 0), c.name
        for k, ln in enumerate(pl["launches"]):
            assert ln["Jo"] == k and ln["p_live"] == round_up(c.p + 1, 16), c.name
            assert ln["n_x"] == (k + 1 if vt else 0), c.name
            assert ln["n_ord"] == (PC.n_ord_of(c) if vt else pl["n_mats"]), c.name


def test_grid_is_the_count_of_tiles():
    """A pure-Python count: 128-row L tiles of every matrix below panel Jo, and the X tiles (block column Jo of V^T:
    block rows 0 .. Jo) of every ordering where V^T is computed."""
    for c, pl in PLANS:
        nb = pl["p_pad"] // 128
        vt = PC.is_tri(c) and not c.flags & 128
        for ln in pl["launches"]:
            Jo = ln["Jo"]
            l_tiles = sum(1 for _ in range(pl["n_mats"]) for I in range(nb) if I > Jo)
            x_tiles = sum(1 for _ in range(PC.n_ord_of(c)) for I in range(nb) if I <= Jo) if vt else 0
            assert ln["grid"] == l_tiles + x_tiles, (c.name, ln)
            assert ln["n_lt"] == nb - 1 - Jo


def test_grouped_and_ungrouped_in_every_mode_and_precision():
    for tri in (True, False):
        for dt in (PC.F64, PC.F32):
            got = {ln["grouped"] for c, pl, ln in launches(lambda c: PC.is_tri(c) == tri and c.dtype == dt)}
            assert got == {True, False}, (tri, dt, got)
            # ... and the ungrouped map also in a launch the grouped one could take (more than one L tile)
            assert any(not ln["grouped"] and ln["n_lt"] > 1
                       for c, pl, ln in launches(lambda c: PC.is_tri(c) == tri and c.dtype == dt)), (tri, dt)
    for c, pl, ln in launches():
        assert ln["grouped"] == (pl["n_mats"] % 8 == 0 and ln["n_lt"] > 1), (c.name, ln)


def test_grouped_cases_have_partners_that_differ_in_B_only():
    grouped = [c for c, pl in PLANS if c.cls.startswith("grouped")]
    assert {c.cls for c in grouped} == {"grouped_8", "grouped_16", "grouped_24", "grouped_p512"}
    for tri in (True, False):
        for dt in (PC.F64, PC.F32):
            mats = {debug_panel_plan(c.p, PC.n_ord_of(c), tri, c.flags)["n_mats"] for c in grouped
                    if PC.is_tri(c) == tri and c.dtype == dt}
            assert {8, 16, 24} <= mats, (tri, dt, mats)
    for c in grouped:
        pl = plan_of(c)
        assert pl["p_pad"] >= 384 and pl["launches"][0]["grouped"] and pl["launches"][0]["Jo"] == 0, c.name
        partners = [d for d, pd in PLANS if d.cls == "ungrouped_partner" and d.B != c.B and
                    (d.p, d.n, d.m, d.dtype, d.flags, d.anti) == (c.p, c.n, c.m, c.dtype, c.flags, c.anti) and
                    not any(ln["grouped"] for ln in pd["launches"])]
        if not partners and c.p == PC.DISPATCH_P512 and PC.is_tri(c):        # B = 3: the panel-count case of p = 385
            partners = [d for d in PC.CASES if d.cls == "panel_count" and d.B != c.B and
                        (d.p, d.m, d.dtype, d.flags, d.anti) == (c.p, c.m, c.dtype, c.flags, c.anti)]
        if not partners and not c.anti and PC.is_tri(c):                     # 4 single orderings: partner "odd_count"
            partners = [d for d in PC.CASES if d.cls == "odd_count" and (d.p, d.m, d.dtype) == (c.p, c.m, c.dtype)]
        assert partners, c.name


def test_grouped_at_p_pad_512_has_three_and_two_tiles():
    for tri in (True, False):
        for dt in (PC.F64, PC.F32):
            cs = [(c, pl) for c, pl in PLANS if c.cls == "grouped_p512" and PC.is_tri(c) == tri and c.dtype == dt]
            assert cs, (tri, dt)
            for c, pl in cs:
                assert pl["p_pad"] == 512
                assert {ln["n_lt"] for ln in pl["launches"] if ln["grouped"]} == {3, 2}, c.name
                assert {ln["n_lt"] for ln in pl["launches"] if not ln["grouped"]} == ({1, 0} if tri else {1}), c.name


def test_every_dispatch_count():
    mats = {(PC.is_tri(c), pl["n_mats"]) for c, pl in PLANS}
    assert (True, 2) in mats and (False, 1) in mats                                 # one ordering alone
    assert any(n % 2 == 1 and n > 1 for tri, n in mats if not tri)                  # an odd count of matrices
    assert any(PC.n_ord_of(c) % 2 == 1 and PC.n_ord_of(c) > 1 for c in PC.CASES if PC.is_tri(c))
    # exactly eight: 2 antithetical samples in tri mode; 8 single orderings and 4 antithetical samples in rect mode
    eight = {(PC.is_tri(c), c.B, c.anti) for c, pl in PLANS if pl["n_mats"] == 8 and pl["p_pad"] >= 384}
    assert {(True, 2, True), (False, 8, False), (False, 4, True)} <= eight, eight
    # rect, p >= 257, a multiple of eight orderings
    assert any(not PC.is_tri(c) and c.p >= 257 and PC.n_ord_of(c) % 8 == 0 for c in PC.CASES)


def test_xlast_on_and_off_in_both_precisions():
    for dt in (PC.F64, PC.F32):
        got = {ln["xlast"] for c, pl, ln in launches(lambda c: c.dtype == dt) if ln["n_lt"] == 0}
        assert got == {True, False}, (dt, got)
        for p in PC.XLAST_ON_P:          # exactly one dead 16-column block: the smallest p_pad - p_live with xlast on
            hit = [ln for c, pl, ln in launches(lambda c: c.dtype == dt and c.p == p and c.cls == "xlast_on")
                   if ln["n_lt"] == 0]
            assert hit and all(ln["xlast"] and ln["p_live"] == round_up(p + 1, 128) - 16 for ln in hit), (dt, p)
        for p in PC.XLAST_OFF_P:         # p_live = p_pad
            hit = [ln for c, pl, ln in launches(lambda c: c.dtype == dt and c.p == p and c.cls == "xlast_off")
                   if ln["n_lt"] == 0]
            assert hit and all(not ln["xlast"] and ln["p_live"] == round_up(p + 1, 128) for ln in hit), (dt, p)
        for p in PC.ONE_LIVE_P:          # one live 16-row block in the last panel
            hit = [ln for c, pl, ln in launches(lambda c: c.dtype == dt and c.p == p and c.cls == "one_live_block")
                   if ln["n_lt"] == 0]
            assert hit and all(ln["xlast"] and ln["p_live"] == round_up(p + 1, 128) - 112 for ln in hit), (dt, p)
    for c, pl, ln in launches():
        assert ln["xlast"] == (ln["n_lt"] == 0 and ln["p_live"] <= pl["p_pad"] - 16), (c.name, ln)
        if ln["xlast"]:
            assert PC.is_tri(c) and not c.flags & 128            # the launch with X tiles alone exists in tri mode only


def test_every_tile_count_and_panel_count():
    for tri in (True, False):
        for dt in (PC.F64, PC.F32):
            sel = launches(lambda c: PC.is_tri(c) == tri and c.dtype == dt)
            assert {ln["n_lt"] for c, pl, ln in sel} >= ({0, 1, 2, 3} if tri else {1, 2, 3}), (tri, dt)
    for dt in (PC.F64, PC.F32):
        tri_p = {c.p for c in PC.CASES if c.cls == "panel_count" and PC.is_tri(c) and c.dtype == dt and c.flags & ~1024 == 0}
        assert tri_p == set(PC.PANEL_COUNT_P), (dt, tri_p)
        assert {pl["p_pad"] for c, pl in PLANS if c.dtype == dt and PC.is_tri(c)} >= {128, 256, 384, 512, 640}
    assert {pl["p_pad"] for c, pl in PLANS if not PC.is_tri(c)} >= {256, 384, 512}
    # p = 127: the lone launch with X tiles only, and with developer flag 128 no panel launch at all
    for c, pl in PLANS:
        if c.p == 127:
            if c.flags & 128:
                assert pl["launches"] == [], c.name
            else:
                assert [(ln["n_lt"], ln["n_x"], ln["xlast"]) for ln in pl["launches"]] == [(0, 1, False)], c.name
    assert any(c.p == 127 and c.dtype == PC.F64 and c.flags == 1024 for c in PC.CASES)


def test_p_live_edges_modes_and_small_fp32():
    for p in PC.P_LIVE_P:
        assert {(c.dtype, PC.is_tri(c)) for c in PC.CASES if c.p == p} >= {(PC.F64, True), (PC.F32, True), (PC.F64, False)}
    assert {(p + 1) % 16 for p in PC.P_LIVE_P} == {0, 1} and all((p + 1) % 128 > 1 for p in PC.P_LIVE_P)
    for dt in (PC.F64, PC.F32):
        for p in (127, 257, 385):
            got = {c.flags & (128 | 512) for c in PC.CASES if c.p == p and c.dtype == dt and PC.is_tri(c)}
            assert got >= {0, 128, 512}, (dt, p, got)
    assert {c.p for c in PC.CASES if c.dtype == PC.F32 and PC.is_tri(c) and c.flags == 0} >= set(PC.FP32_SMALL_P)
    for dt in (PC.F64, PC.F32):
        assert {c.m for c in PC.CASES if not PC.is_tri(c) and c.p >= 130 and c.dtype == dt} >= set(PC.RECT_M_EDGES)


def test_every_grouped_xlast_and_panel_count_class_has_an_fp32_twin():
    names = {c.name for c in PC.CASES}
    for c in PC.CASES:
        if c.dtype == PC.F64 and (c.cls.startswith("grouped") or c.cls in ("xlast_on", "xlast_off", "one_live_block")
                                  or (c.cls == "panel_count" and PC.is_tri(c))) and c.flags & 512 == 0:
            twin = c._replace(dtype=PC.F32, flags=c.flags & ~1024)
            assert any(d[1:] == twin[1:] for d in PC.CASES), c.name
    assert len(names) == len(PC.CASES)


def test_orderings_are_prefixes_of_one_sequence():
    for p in (15, 300):
        full = PC.orderings_of(p, PC.N_ORDERS)
        assert full.dtype == np.int32 and full.shape == (PC.N_ORDERS, p)
        np.testing.assert_array_equal(full[0], np.arange(p))
        np.testing.assert_array_equal(full[1], np.arange(p)[::-1])
        assert all(sorted(row) == list(range(p)) for row in full)
        np.testing.assert_array_equal(PC.orderings_of(p, 5), full[:5])


def test_plan_hook_refuses_what_the_launch_refuses():
    ok = debug_panel_plan_launch(384, 0, 8, 4, True, 304)
    assert ok == {"Jo": 0, "n_lt": 2, "n_x": 1, "grouped": True, "xlast": False, "grid": 20, "p_live": 304, "n_ord": 4}
    # p_live out of range counts as "none known"
    for p_live in (0, -5, 385):
        assert debug_panel_plan_launch(384, 2, 8, 4, True, p_live)["p_live"] == 384
    assert debug_panel_plan_launch(384, 2, 8, 4, True, 368)["xlast"]
    assert not debug_panel_plan_launch(384, 2, 8, 4, True, 369)["xlast"]
    assert debug_panel_plan_launch(384, 0, 5, 0, False, 304)["n_ord"] == 5            # without X tiles n_ord is n_mats
    bad = [(383, 0, 8, 4, True, 0),          # p_pad no multiple of 128
           (0, 0, 8, 4, True, 0), (-128, 0, 8, 4, True, 0),
           (384, -1, 8, 4, True, 0),         # Jo out of range
           (384, 3, 8, 4, True, 0),
           (384, 2, 8, 8, False, 0),         # the last launch has X tiles only
           (128, 0, 8, 8, False, 0),
           (384, 0, 0, 0, False, 0),         # no matrix
           (384, 0, 8, 0, True, 0),          # X tiles: n_mats = 2 n_ord
           (384, 0, 8, 3, True, 0), (384, 0, 7, 4, True, 0),
           (4096, 0, 2 ** 27, 2 ** 26, True, 0)]      # more than 2^31 - 1 workgroups
    for args in bad:
        with pytest.raises(ValueError):
            debug_panel_plan_launch(*args)
    for p, n_ord in ((0, 4), (-1, 4), (300, 0), (300, -2), (40000, 1)):
        with pytest.raises(ValueError):
            debug_panel_plan(p, n_ord, True)
    assert debug_panel_plan(127, 3, False)["launches"] == []                          # rect, one panel: nothing to launch
