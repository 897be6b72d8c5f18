"""Separable games (tests/separable_ref.py) -- CPU side: the blockwise long-double truths against the fp64 host oracles
of the WHOLE problem where those can still enumerate (p <= 14, g <= 10), and the proof that the cases of
tests/test_gpu_enum_top.py reach the slots, sizes and layouts they are there for, from the kernels' maps restated in
plain Python and the library's host-only planners."""
import numpy as np
import pytest

import separable_ref as SR
from ls_spa._engine import debug_boot_plan, debug_groups_best_plan, debug_owen_plan
from owen_ref import BIG_CASE, BIG_PLAN, owen_values
from test_group_interactions_host import group_interactions
from test_groups_host import group_shapley, group_values
from test_interactions_host import exact_interactions
from test_subsets_host import exact_shapley, gram_problem

TOL = dict(rtol=0, atol=1e-13)
EPS = 2.220446049250313e-16


def well_conditioned(sep):
    """Every block's true smallest relative pivot is at least 100 x the engine's NOT_PD threshold 16 p eps -- and, far
    stronger, kappa of every block's G and H is at most 1e4: a Gram / Cholesky route at c eps kappa with c of a few
    hundred then stays two orders under the 1e-11 of the GPU tests, whoever computes it."""
    assert sep.min_pivot() >= 100 * 16 * sep.p * EPS, sep.min_pivot()
    assert sep.worst_condition() <= 1e4, sep.worst_condition()


# ---- the construction is valid -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    """Blocks (5, 4, 5) dealt to permuted positions, p = 14, two responses."""
    return SR.make((5, 4, 5), 90, 60, seed=1, responses=2)


def test_gram_matrices_are_exactly_block_diagonal(small):
    G, _, H, _, _ = gram_problem(*small.data())
    off = small.block_of[:, None] != small.block_of[None, :]
    assert (G[off] == 0.0).all() and (H[off] == 0.0).all() and off.any()
    assert sorted(len(b) for b in small.blocks) == [4, 5, 5]
    assert any(np.any(np.diff(b) > 1) for b in small.blocks), "the blocks are not contiguous runs of columns"


@pytest.mark.parametrize("r", [0, 1])
def test_phi_and_interactions_are_the_whole_problems(small, r):
    prob = gram_problem(*small.data(r))
    np.testing.assert_allclose(small.phi(r), exact_shapley(*prob), **TOL)
    raw = exact_interactions(*prob)
    np.testing.assert_allclose(small.interactions(r), raw, **TOL)
    cross = small.block_of[:, None] != small.block_of[None, :]
    assert (small.interactions(r)[cross] == 0.0).all() and np.abs(raw[~cross]).max() > 1e-4
    assert abs(small.total(r) - exact_shapley(*prob).sum()) <= 1e-13
    assert np.abs(small.phi(0) - small.phi(1)).max() > 1e-3
    well_conditioned(small)


def test_the_games_are_not_additive_inside_a_block(small):
    b = small.blocks[0]
    assert np.abs(small.interactions()[np.ix_(b, b)]).max() > 1e-4


@pytest.mark.parametrize("groups, g", [
    ([[2, 3], [1, 2, 1], [2, 2, 1]], 8),              # no baseline
    ([[2, 2], [1, 2], [2, 1, 1]], 7),                 # baseline columns 1 + 1 + 1 from inside the blocks
    ([[1] * 4, [1] * 3, [1] * 3], 10),                # g = 10, baseline 1 + 1 + 2
])
@pytest.mark.parametrize("r", [0, 1])
def test_group_truths_are_the_whole_problems(small, groups, g, r):
    labels = small.labels(groups, seed=g)
    assert labels.max() + 1 == g and (labels == -1).sum() == 14 - sum(map(sum, groups))
    prob = gram_problem(*small.data(r))
    np.testing.assert_allclose(small.group_phi(labels, r), group_shapley(*prob, labels), **TOL)
    np.testing.assert_allclose(small.group_interactions(labels, r), group_interactions(*prob, labels), **TOL)
    u = group_values(*prob, labels, [0, (1 << g) - 1])
    assert abs(small.group_gain(labels, r) - (u[1] - u[0])) <= 1e-13
    assert np.abs(small.group_interactions(labels, r)).max() > 1e-4
    well_conditioned(small)


@pytest.mark.parametrize("groups", [[[2, 3], [1, 2, 1], [2, 2, 1]], [[3, 1], [2, 1], [2, 2]]])
def test_owen_truth_is_the_whole_problems(small, groups):
    labels = small.labels(groups, seed=5)
    want = owen_values(*gram_problem(*small.data()), labels)
    for k in range(labels.max() + 1):
        np.testing.assert_allclose(small.owen(labels, k), want[labels == k], **TOL)
    assert (want[labels == -1] == 0.0).all() and np.abs(want).max() > 1e-3


def test_place_puts_the_chosen_columns_where_they_are_asked():
    cols = SR.place(12, (5, 4, 3), {0: [0, 11], 2: [5]}, seed=3)
    assert {0, 11} <= set(cols[0]) and 5 in cols[2] and [len(c) for c in cols] == [5, 4, 3]
    assert sorted(c for b in cols for c in b) == list(range(12))


# ---- the cases reach what they claim -----------------------------------------------------------------------------------
def kinds_of_pairs(sep):
    """How many within-block pairs are low-low, low-high, high-high."""
    out = [0, 0, 0]
    for cols in sep.blocks:
        lo, hi = int((cols < SR.SQ).sum()), int((cols >= SR.SQ).sum())
        out[0] += lo * (lo - 1) // 2
        out[1] += lo * hi
        out[2] += hi * (hi - 1) // 2
    return out


@pytest.mark.parametrize("p", sorted(SR.PHI_SIZES))
def test_phi_cases_straddle_the_low_high_split(p):
    sep = SR.phi_case(p)
    assert sep.p == p and all(7 <= len(b) <= 9 for b in sep.blocks)
    assert sum(1 for b in sep.blocks if (b < SR.SQ).any() and (b >= SR.SQ).any()) >= 2
    sep.phi()
    well_conditioned(sep)


def test_p32_is_8192_units_of_8192_high_subsets_in_several_launches():
    """The library has no host hook for the cut of the one-problem call itself.  This is the bootstrap's plan (BOOT_UNITS
    and BOOT_SUBSETS_PER_LAUNCH of csrc/boot_plan.h), which a static_assert in csrc/lsspa_api.hip ties to the one-problem
    call's EXACT_UNITS and SUBSETS_PER_LAUNCH: the library does not compile with the two apart.  On the device
    test_phi_of_every_feature[32] asserts the 64 launches of the call under test (subsets_timing)."""
    plan = debug_boot_plan(1, 180, 144, 32)
    assert plan["units"] == 8192 and plan["per"] == 8192 == (1 << (32 - SR.SQ)) // 8192
    assert plan["per"] // plan["steps"] == 64


@pytest.mark.parametrize("p, top", [(30, 4), (32, 5)])
def test_interaction_cases_fill_every_slot_of_the_high_high_pairs(p, top):
    sep = SR.inter_case(p)
    pairs = SR.high_pairs(p)
    nh = p - SR.SQ
    assert len(pairs) == nh * (nh - 1) // 2 == {30: 276, 32: 325}[p] and (len(pairs) - 1) >> 6 == top
    assert pairs[0] == (6, 7) and pairs[nh - 2] == (6, p - 1) and pairs[nh - 1] == (7, 8) and pairs[-1] == (p - 2, p - 1)
    within, cross = [0] * (top + 1), [0] * (top + 1)
    for e, (i, j) in enumerate(pairs):
        (within if sep.block_of[i] == sep.block_of[j] else cross)[e >> 6] += 1
    assert min(within) >= 1 and min(cross) >= 1, (within, cross)
    assert min(kinds_of_pairs(sep)) >= 1, kinds_of_pairs(sep)
    raw = sep.interactions()
    for slot in range(top + 1):                        # ... and a within-block pair of every slot has a value to miss
        assert max(abs(raw[i, j]) for e, (i, j) in enumerate(pairs)
                   if e >> 6 == slot and sep.block_of[i] == sep.block_of[j]) > 1e-5
    well_conditioned(sep)


@pytest.mark.parametrize("p", sorted(SR.MULTI_RESPONSES))
def test_multi_cases(p):
    sep = SR.phi_case(p, SR.MULTI_RESPONSES[p])
    assert sep.responses == SR.MULTI_RESPONSES[p] and (sep.responses - 1) // 8 == {30: 1, 32: 0}[p]
    for r in range(sep.responses):
        sep.phi(r)
    well_conditioned(sep)


def test_value_masks_reach_the_last_entry_slot_of_the_sweep_matrix():
    masks = SR.top_masks(32, 256, seed=32)
    reach = [SR.sweep_slot(m, 32) for m in masks]
    assert max(reach) == (33, 17) and (1 << 32) - 1 in masks and 1 << 31 in masks
    sizes = {(bin(int(m) >> 6).count("1"), int(m) & 63) for m in masks}
    assert all((k, low) in sizes for k in range(27) for low in (0, 63))
    assert all(1 << j in masks for j in range(32)) and len(masks) >= 256 + 54 + 32
    assert {n for n, _ in reach} == set(range(7, 34)), "every number of rows of the sweep matrix"


@pytest.mark.parametrize("name", list(SR.GROUP_CASES))
def test_grouped_layouts_are_what_the_cases_say(name):
    sizes, groups, lay = SR.GROUP_CASES[name]
    m = SR.MULTI_GROUP_RESPONSES if name == "g24_p48" else 1
    sep, labels = SR.group_case(name, m)
    plan = debug_groups_best_plan(labels)
    assert (plan["gl"], plan["gh"], plan["ql"], plan["nb"]) == lay == SR.group_layout(labels)
    assert len(labels) == sum(sizes) == {"g24_p64": 64, "g28_p56": 56, "g24_p48": 48}[name]
    assert labels.max() + 1 == plan["gl"] + plan["gh"] == int(name[1:3])
    assert plan["units"] == 8192 and plan["launches"] > 1
    per_block = [len(set(labels[b][labels[b] >= 0])) for b in sep.blocks]
    assert all(7 <= k <= 8 for k in per_block)
    low = SR.low_groups(labels)
    for k in low:                                      # a low group shares its block with high groups
        b = sep.block_of[np.nonzero(labels == k)[0][0]]
        assert set(labels[sep.blocks[b]]) - set(low) - {-1}
    for r in range(m):
        sep.group_phi(labels, r)
    well_conditioned(sep)


def test_group_value_masks_at_g32():
    labels, masks = SR.G32_LABELS, SR.g32_masks(128, seed=32)
    assert len(labels) == 64 and labels.max() == 31 and SR.group_layout(labels) == (3, 29, 6, 0)
    assert (1 << 32) - 1 in masks and all(any((int(m) >> b) & 1 for m in masks) for b in range(28, 32))
    assert any(int(m) >> 28 == 15 for m in masks) and 0 in masks


def test_owen_case_is_the_big_case_made_separable():
    sep, parts = SR.owen_case(BIG_CASE, 14)
    plan = debug_owen_plan(BIG_CASE)
    for k, want in BIG_PLAN.items():
        assert {f: plan[k][f] for f in want} == want, (k, plan[k])
    assert plan[14]["launches"] >= 2 and sep.p == 64
    assert parts[0][0] == 14 and len(parts[0]) == 3 and [len(b) for b in sep.blocks] == [16, 12, 12, 12, 12]
    for part, cols in zip(parts, sep.blocks):
        assert set(BIG_CASE[cols]) == set(part)
    sep.owen(BIG_CASE, 14)
    sep.owen(BIG_CASE, parts[1][0])
    well_conditioned(sep)
