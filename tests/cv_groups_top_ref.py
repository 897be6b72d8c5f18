"""Truth of ls_spa_top_group_subsets_cv  --  TEST INFRASTRUCTURE, NOT PRODUCT CODE.

The T best sets of groups of every size by the K-fold cross-validated value: a table of all 2^g values (the truth of
tests/cv_groups_ref.py, or the device's own debug values) sorted by tests/top_ref.top_truth under (larger value, then
smaller mask; bit k = group k), with an optional `ok` mask of the candidates; the margins of such lists and the
one-standard-error statistics are tests/cv_top_ref.py's.  The cases are cv_groups_ref.case(name, K) for NAMES x KS."""
import numpy as np

import cv_groups_ref as CG
import cv_top_ref as CT
import top_ref

T_MAX = top_ref.T_MAX
NAMES, KS, MIN_GAP = CG.NAMES, CG.KS, CG.MIN_GAP
case, case_labels = CG.case, CG.case_labels
margin, one_se = CT.margin, CT.one_se


def n_groups(labels):
    return int(np.max(labels)) + 1


def all_masks(g):
    return np.arange(1 << g, dtype=np.uint64)


def top_lists(u_all, g, T, ok=None):
    """(u [g + 1][T] float64, masks [g + 1][T] uint32, count [g + 1]) of a table of all 2^g values: per size the T first
    masks under (larger value, smaller mask) among those that are ok (all, if None) and not NaN; NaN / 0 past count."""
    return top_ref.top_truth(np.asarray(u_all, dtype=np.float64), g, T, 0, ok)


def groups_of(masks, g):
    """bool [...][g] of the masks [...]"""
    return ((np.asarray(masks).astype(np.int64)[..., None] >> np.arange(g)) & 1).astype(bool)


def masks_of(group_subsets):
    return (np.asarray(group_subsets).astype(np.int64) << np.arange(group_subsets.shape[-1])).sum(axis=-1)


def columns_of(labels, group_subset):
    """bool [p]: the baseline's columns and those of the groups in group_subset [g] bool"""
    labels = np.asarray(labels)
    return np.array([l < 0 or bool(group_subset[l]) for l in labels])
