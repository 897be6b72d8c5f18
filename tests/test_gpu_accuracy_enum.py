"""The rule of tests/test_gpu_accuracy.py -- tol = max(T0, MG * e_plain) against a long-double truth, NOT_PD excused only
within 100 x of the engine's threshold -- for every exact entry point that has arithmetic or problems of its own:

    a  multi_values            p = 20, m = MULTI_RB + 1 (two chunks of responses, the last with one)
    b  multi_shapley           p = 10, the same m; every row and the rows' sums
    c  multi_group_values, multi_groups_shapley      g = 10 on p = 24 with a baseline of 4; values also at g = 12, p = 40
    d  groups_owen             p = 17, groups of 8, 3, 3, 3: several high groups and units in every refined game
    e  perm_observed, perm_run p = 10 and the groups of c; the null rows against the truth on the permuted responses
    f  boot_run, boot_groups_run        four replicates by weights, each on its own info word and its own true pivot
    g  cv_get_problem, cv_shapley, debug_cv_values, cv_groups_shapley   K = 3 unequal folds, each on its own word
    h  cv_path_shapley         the data of g at kappa = 1e6, five ridge values from 0 to 1e6 x the mean diagonal
    i  subsets_best, subsets_top, cv_best   the winner's value, and the winning mask wherever the truth's margin allows

The data are hp_ref.gen over KAPPAS, the truths tests/hp_games.py's, the case table tests/accuracy_enum_cases.py's;
tests/test_hp_games_host.py proves from the truth alone that no case at kappa <= 1e4 can be excused and that every
selection case at kappa <= 1e3 has clear winners.  The measured worst r = err / max(e_plain, 4 eps) of every entry point
is in DESIGN.md, Numerics."""
from math import comb

import numpy as np
import pytest

import accuracy_enum_cases as C
import hp_games as HG
import owen_ref
from ls_spa._engine import (HipEngine, debug_boot_groups_plan, debug_boot_plan, debug_cv_groups_plan,
                            debug_cv_path_plan, debug_cv_plan, debug_owen_plan, debug_perm_plan)
from ls_spa._native import LSSPANativeError
from test_gpu_accuracy import EPS, KAPPAS, MG, T0, judge, shape, threshold, values_case
from test_gpu_cv import check_problems

pytestmark = pytest.mark.gpu

WORST = {}          # entry point -> (worst r, the case that produced it), for DESIGN.md (Numerics)
GOVERNED = {}       # the same over the cases whose tolerance is MG * e_plain, not the floor T0
BY_MASK = {}        # (selection entry, kappa) -> (ranks compared by mask, ranks compared by value only)


def keep(entry, name, r, e_plain):
    for book in (WORST, GOVERNED) if MG * e_plain > T0["float64"] else (WORST,):
        if r == r and r >= book.get(entry, (-1.0, ""))[0]:
            book[entry] = (r, name)


def last(*entries):
    for entry in entries:
        r, name = WORST.get(entry, (float("nan"), "every case excused so far"))
        print(f"ACCENUM {entry} worst r = {r:.2f} ({name})")


def check(entry, name, got, t, key, not_pd, ratio):
    """One result array through judge, its r kept for the report."""
    name = f"{entry} {name}"
    keep(entry, name, judge(name, got, t.want[key], t.e_plain[key], int(bool(not_pd)), float(ratio)), t.e_plain[key])


def hook(call):
    """(result, not_pd) of a test hook that reports a failed pivot as an error."""
    try:
        return call(), 0
    except LSSPANativeError as e:
        assert "positive definite" in str(e), e
        return None, 1


def column(got, r):
    return None if got is None else got[:, r]


# ---- the shapes do what the table says ---------------------------------------------------------------------------------
def test_the_plans_are_what_the_cases_were_chosen_for():
    n, m = shape(10)
    assert C.MULTI_RB == HipEngine.MULTI_RB
    assert -(-C.M_RESP // HipEngine.MULTI_RB) == 2 and C.M_RESP % HipEngine.MULTI_RB == 1      # two chunks, 8 + 1
    # the cut of the 2^14 high subsets at p = 20 into units x per: exact_units() of lsspa_api.hip, which every exact
    # enumeration (the many-response one included) and the bootstrap's planner share; only the latter has a host hook
    cut20 = debug_boot_plan(1, *shape(20), 20)
    assert cut20["units"] > 1 and cut20["per"] > 1
    owen = debug_owen_plan(C.LABELS_OWEN)
    assert [row["launches"] for row in owen] == [1, 1, 1, 1]
    assert all(row["gh"] > 1 and row["high_subsets"] == 1 << row["gh"] for row in owen)        # 2^gh units of one each
    assert owen[0]["inner_high"] == 2 and owen[0]["inner_low"] == 6 and owen[0]["players"] == 11
    boot = debug_boot_plan(C.BOOT_R, n, m, 10)
    assert boot["block"] == C.BOOT_R and boot["enum_reps"] == C.BOOT_R and boot["units"] == 16  # one grid for all four
    gboot = debug_boot_groups_plan(C.BOOT_R, n, m, C.LABELS_P10)
    assert gboot["block"] == C.BOOT_R and gboot["enum_reps"] == C.BOOT_R
    cv = debug_cv_plan(10, C.CV_K)
    assert cv["units"] == 16 and cv["launches"] == 1
    gcv = debug_cv_groups_plan(C.LABELS_P10, C.CV_K)
    assert gcv["gl"] + gcv["gh"] == 4 and gcv["launches"] >= 1
    path = debug_cv_path_plan(10, C.CV_K, len(C.PATH_REGS))
    assert path["block"] * path["blocks"] >= len(C.PATH_REGS) and path["units"] == 16
    perm = debug_perm_plan(C.PERM_R, n, m, 10)
    assert perm["block"] == C.PERM_R and perm["n_blocks"] == 1                                  # three responses at once
    ids = C.cv_folds(n, 10)
    assert [(ids == f).sum() for f in range(C.CV_K)] == [12, n // 2, n - 12 - n // 2]


# ---- a, b: many responses ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kappa", KAPPAS)
def test_sweep_multi_values_p20(engine, kappa):
    t = C.multi_values_truth(kappa)
    engine.multi_load(*t.data, 0.0)
    try:
        got, not_pd = hook(lambda: engine.multi_values(C.MASKS_P20))
    finally:
        engine.multi_free()
    for r in range(C.M_RESP):
        check("multi_values", f"p=20 kappa={kappa:g} response {r}", column(got, r), t, r, not_pd, t.ratio)
    last("multi_values")


@pytest.mark.parametrize("kappa", KAPPAS)
def test_sweep_multi_shapley_p10(engine, kappa):
    t = C.multi_shapley_truth(kappa)
    engine.multi_load(*t.data, 0.0)
    try:
        phi, info = engine.multi_shapley()
    finally:
        engine.multi_free()
    for r in range(C.M_RESP):
        check("multi_shapley", f"p=10 kappa={kappa:g} response {r}", phi[r], t, r, info & 1, t.ratio)
    check("multi_shapley", f"p=10 kappa={kappa:g} row sums", phi.sum(axis=1), t, "sums", info & 1, t.ratio)
    last("multi_shapley")


# ---- c: many responses over groups -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kappa", KAPPAS)
def test_sweep_multi_groups_g10_p24(engine, kappa):
    t = C.multi_groups_truth(kappa)
    engine.multi_load(*t.data, 0.0)
    try:
        vals, v_pd = hook(lambda: engine.multi_group_values(C.LABELS_G10, C.MASKS_G10))
        phi, info = engine.multi_groups_shapley(C.LABELS_G10)
    finally:
        engine.multi_free()
    for r in range(C.M_RESP):
        check("multi_group_values", f"g=10 p=24 kappa={kappa:g} response {r}", column(vals, r), t, ("values", r), v_pd,
              t.ratio)
        check("multi_groups_shapley", f"g=10 p=24 kappa={kappa:g} response {r}", phi[r], t, ("phi", r), info & 1, t.ratio)
    check("multi_groups_shapley", f"g=10 p=24 kappa={kappa:g} row sums", phi.sum(axis=1), t, "sums", info & 1, t.ratio)
    last("multi_group_values", "multi_groups_shapley")


@pytest.mark.parametrize("kappa", KAPPAS)
def test_sweep_multi_group_values_g12_p40(engine, kappa):
    t = C.multi_group_values_p40_truth(kappa)
    engine.multi_load(*t.data, 0.0)
    try:
        vals, not_pd = hook(lambda: engine.multi_group_values(C.LABELS_G12, C.MASKS_G12))
    finally:
        engine.multi_free()
    for r in range(C.M_RESP):
        check("multi_group_values", f"g=12 p=40 kappa={kappa:g} response {r}", column(vals, r), t, r, not_pd, t.ratio)
    last("multi_group_values")


# ---- d: Owen values ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kappa", KAPPAS)
def test_sweep_groups_owen_p17(kappa):
    seen = {}

    def call(eng):
        ow, _, info = eng.groups_owen(C.LABELS_OWEN)
        seen["owen"], seen["info"] = ow, info
        return ow, info & 1

    values_case("groups_owen", 17, kappa, call, lambda ref: HG.owen(ref, C.LABELS_OWEN),
                lambda prob: owen_ref.owen_values(*prob, C.LABELS_OWEN))
    t = C.owen_truth(kappa)                   # the same data by the same seed rule: the table's conditions speak of it
    if not seen["info"] & 1:
        err = float(np.abs(seen["owen"] - t.want["owen"]).max())
        keep("groups_owen", f"groups_owen p=17 kappa={kappa:g}", err / max(t.e_plain["owen"], 4 * EPS["float64"]),
             t.e_plain["owen"])
        np.testing.assert_array_equal(seen["owen"][C.LABELS_OWEN == -1], 0.0)
    last("groups_owen")


# ---- e: the permutation test -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grouped", [False, True], ids=["p10", "g10_p24"])
@pytest.mark.parametrize("kappa", KAPPAS)
def test_sweep_permutation_test(engine, kappa, grouped):
    t = C.perm_truth(kappa, grouped)
    labels = C.LABELS_G10 if grouped else None
    tag = f"{'g=10 p=24' if grouped else 'p=10'} kappa={kappa:g}"
    engine.perm_load(*t.data, 0.0)
    try:
        obs, info_obs = engine.perm_observed(labels)
        phi, _, _, info = engine.perm_run(C.PERM_R, C.PERM_SEED, labels, sides=3)
    finally:
        engine.perm_free()
    check("perm_observed", tag, obs, t, "observed", info_obs & 1, t.ratio)
    for r in range(C.PERM_R):
        check("perm_run", f"{tag} replicate {r}", phi[r], t, r, info & 1, t.ratio)
    last("perm_observed", "perm_run")


# ---- f: the bootstrap --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kappa", KAPPAS)
def test_sweep_bootstrap_replicates(engine, kappa):
    t = C.boot_truth(kappa)
    engine.boot_load(*t.data, 0.0)
    try:
        phi, r2, info = engine.boot_run(C.BOOT_R, 0, t.w_train, t.w_test)
        gphi, gr2, gbase, ginfo = engine.boot_groups_run(C.LABELS_P10, C.BOOT_R, 0, t.w_train, t.w_test)
    finally:
        engine.boot_free()
    for r in range(C.BOOT_R):
        tag = f"p=10 kappa={kappa:g} replicate {r} info={info[r]}"
        check("boot_run", f"{tag} phi", phi[r], t, ("phi", r), info[r] & 1, t.ratio[r])
        if np.isfinite(r2[r]):                     # r2 is a host Cholesky solve: NaN where that fails, never a flag
            check("boot_run", f"{tag} r2", r2[r], t, ("r2", r), 0, t.ratio[r])
        tag = f"g=4 p=10 kappa={kappa:g} replicate {r} info={ginfo[r]}"
        check("boot_groups_run", f"{tag} phi", gphi[r], t, ("gphi", r), ginfo[r] & 1, t.ratio[r])
        if np.isfinite(gr2[r]) and np.isfinite(gbase[r]):
            check("boot_groups_run", f"{tag} r2", gr2[r], t, ("gr2", r), 0, t.ratio[r])
            check("boot_groups_run", f"{tag} r2_base", gbase[r], t, ("gbase", r), 0, t.ratio[r])
        if t.ratio[r] >= 100:
            assert np.isfinite(r2[r]) and np.isfinite(gr2[r]) and np.isfinite(gbase[r])
    last("boot_run", "boot_groups_run")


# ---- g: K-fold cross-validation ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["issue", "lopsided"])
@pytest.mark.parametrize("kappa", KAPPAS)
def test_sweep_cross_validation(engine, kappa, layout):
    """issue: folds of p + 2, half and the rest of 90 rows.  lopsided: fold 0 trains on p of 2000 rows -- the one fold
    whose word may (from kappa 1e5) and must (1e6, 3e6: the truth is 50 x under the threshold) be set while its siblings'
    must not, and whose training sums a subtraction from the pooled sum would leave 200 x less accurate."""
    t = C.cv_truth(kappa, 0.0, layout)
    K = C.CV_K
    engine.cv_load(t.X, t.y, t.ids, K, 0.0)
    try:
        check_problems(engine, t.X, t.y, t.ids, K, 0.0)        # 1e-13 relative, entries 12 orders of magnitude apart
        phi, phi_fold, r2_fold, info = engine.cv_shapley()
        v, v_fold = engine.debug_cv_values(C.MASKS_P10)
        gphi, gfold, gr2, gbase, ginfo = engine.cv_groups_shapley(C.LABELS_P10)
    finally:
        engine.cv_free()
    for f in range(K):
        tag = f"{layout} p=10 kappa={kappa:g} fold {f} info={info[f]}"
        check("cv_shapley", f"{tag} phi_fold", phi_fold[f], t, ("phi_fold", f), info[f] & 1, t.ratio[f])
        check("cv_shapley", f"{tag} r2_fold", r2_fold[f], t, ("r2_fold", f), info[f] & 1, t.ratio[f])
        check("debug_cv_values", f"{tag} v_fold", v_fold[:, f], t, ("v_fold", f), info[f] & 1, t.ratio[f])
        tag = f"{layout} g=4 p=10 kappa={kappa:g} fold {f} info={ginfo[f]}"
        check("cv_groups_shapley", f"{tag} phi_fold", gfold[f], t, ("gphi_fold", f), ginfo[f] & 1, t.ratio[f])
        check("cv_groups_shapley", f"{tag} r2_fold", gr2[f], t, ("gr2_fold", f), ginfo[f] & 1, t.ratio[f])
        check("cv_groups_shapley", f"{tag} base_fold", gbase[f], t, ("gbase_fold", f), ginfo[f] & 1, t.ratio[f])
    # what sums the folds is excused only if one of its folds is flagged, and then only within reach of the threshold
    flagged = t.ratio[(info & 1) == 1]
    if layout == "lopsided" and kappa >= 1e6:
        assert info[0] & 1 and ginfo[0] & 1, "fold 0's true pivot is 50 x under the threshold and it is not flagged"
    check("cv_shapley", f"{layout} p=10 kappa={kappa:g} phi", phi, t, "phi", len(flagged), flagged.min() if len(flagged) else np.inf)
    check("debug_cv_values", f"{layout} p=10 kappa={kappa:g} v", v, t, "v", len(flagged), flagged.min() if len(flagged) else np.inf)
    gflag = t.ratio[(ginfo & 1) == 1]
    check("cv_groups_shapley", f"{layout} g=4 p=10 kappa={kappa:g} phi", gphi, t, "gphi", len(gflag),
          gflag.min() if len(gflag) else np.inf)
    last("cv_shapley", "debug_cv_values", "cv_groups_shapley")


# ---- h: the ridge path ---------------------------------------------------------------------------------------------------------
def test_ridge_path_at_kappa_1e6(engine):
    truths = C.path_truths()
    t0, K = truths[0], C.CV_K
    regs = C.path_regs(t0.X)
    engine.cv_load(t0.X, t0.y, t0.ids, K, 0.0)
    try:
        phi, phi_fold, r2_fold, info = engine.cv_path_shapley(regs)
    finally:
        engine.cv_free()
    for l, t in enumerate(truths):
        for f in range(K):
            tag = f"reg={regs[l]:.3g} fold {f} info={info[l, f]}"
            check("cv_path_shapley", f"{tag} phi_fold", phi_fold[l, f], t, ("phi_fold", f), info[l, f] & 1, t.ratio[f])
            check("cv_path_shapley", f"{tag} r2_fold", r2_fold[l, f], t, ("r2_fold", f), info[l, f] & 1, t.ratio[f])
        flagged = t.ratio[(info[l] & 1) == 1]
        check("cv_path_shapley", f"reg={regs[l]:.3g} phi", phi[l], t, "phi", len(flagged),
              flagged.min() if len(flagged) else np.inf)
    # the huge ridge: G is reg I to 1e-6, phi ~ 1e-6 of R^2 -- finite, unflagged, and within the absolute T0
    assert np.all(info[-1] == 0) and np.all(np.isfinite(phi[-1])) and np.all(np.isfinite(phi_fold[-1]))
    assert np.abs(truths[-1].want["phi"]).max() < 1e-4 and np.abs(phi[-1] - truths[-1].want["phi"]).max() <= T0["float64"]
    last("cv_path_shapley")


# ---- i: selection under near-ties ------------------------------------------------------------------------------------------
def check_selection(entry, kappa, t, v, masks, count, not_pd, ratio):
    """v, masks [p + 1][T], count [p + 1] of a (top) list against the table t.table: every valid rank's value through
    judge; its mask wherever the truth's margin to both neighbours exceeds 2 tol; a missing rank only where every
    candidate of that size is a legitimately excusable failed pivot."""
    p, T = 10, v.shape[1]
    e_plain = t.e_plain["v_all"]
    tol = C.tol_of(e_plain)
    rank = C.ranking(t.table, p, T)
    gaps = C.margins(rank, T)
    size = HG.bits_of(np.arange(1 << p), p).sum(axis=1)
    got, want, by_mask, by_value = [], [], [], 0
    for k in range(p + 1):
        full = min(T, comb(p, k))
        assert 0 <= count[k] <= full
        if count[k] < full:
            assert not_pd, f"{entry} kappa={kappa:g}: size {k} has {count[k]} of {full} ranks without NOT_PD"
            if count[k] == 0:
                worst = t.pivots[size == k].max() / threshold(p)
                assert worst < 100, f"{entry} kappa={kappa:g}: size {k} not found, a candidate's pivot {worst:.3g} x"
            continue                                  # ranks of a size that lost candidates are not the truth's ranks
        for r in range(full):
            got.append(v[k, r])
            want.append(float(rank[k][r][0]))
            if gaps[k, r] > 2 * tol:
                by_mask.append((k, r))
            else:
                by_value += 1
    name = f"{entry} p=10 kappa={kappa:g}"
    r = judge(name, np.array(got), np.array(want), e_plain, int(bool(not_pd)), float(ratio))
    keep(entry, name, r, e_plain)
    if r == r:
        for k, rk in by_mask:
            assert int(masks[k, rk]) == rank[k][rk][1], f"{name}: size {k} rank {rk}: mask {int(masks[k, rk]):#x}, " \
                                                         f"the truth's {rank[k][rk][1]:#x} by {gaps[k, rk]:.3e}"
        BY_MASK[(entry, kappa)] = (len(by_mask), by_value)
        print(f"ACCENUM {name}: {len(by_mask)} ranks compared by mask, {by_value} by value only (2 tol = {2 * tol:.3e})")
        if kappa <= 1e3:
            assert by_value == 0
    last(entry)


@pytest.mark.parametrize("kappa", KAPPAS)
def test_sweep_subsets_best_and_top(engine, kappa):
    t = C.selection_truth(kappa)
    engine.load_data(*t.data, 0.0)
    v, masks, found, info = engine.subsets_best()
    check_selection("subsets_best", kappa, t, v[:, None], masks[:, None], found.astype(int), info & 1, t.ratio)
    tv, tmasks, count, tinfo = engine.subsets_top(n_best=C.N_BEST)
    check_selection("subsets_top", kappa, t, tv, tmasks, count, tinfo & 1, t.ratio)


@pytest.mark.parametrize("kappa", KAPPAS)
def test_sweep_cv_best(engine, kappa):
    t = C.cv_truth(kappa)
    engine.cv_load(t.X, t.y, t.ids, C.CV_K, 0.0)
    try:
        v, masks, found, _, info = engine.cv_best()
    finally:
        engine.cv_free()
    flagged = t.ratio[(info & 1) == 1]
    check_selection("cv_best", kappa, t, v[:, None], masks[:, None], found.astype(int), len(flagged),
                    flagged.min() if len(flagged) else np.inf)


@pytest.fixture(scope="module", autouse=True)
def report():
    """After the module's tests, whichever of them ran: the numbers of DESIGN.md (Numerics) -- every entry point's worst
    r over all cases and over those whose tolerance is MG * e_plain and not the floor T0, and how selection was
    compared.  Nothing is asserted here: judge has held every case."""
    yield
    for entry in sorted(WORST):
        r, name = WORST[entry]
        print(f"ACCENUM worst {entry}: r = {r:.2f} ({name}){'  ABOVE THE DOCUMENTED MARGIN OF 2' if r > 2 else ''}")
        r, name = GOVERNED.get(entry, (float("nan"), "no case above the floor"))
        print(f"ACCENUM worst above the floor {entry}: r = {r:.2f} ({name})")
    for (entry, kappa), (n_mask, n_value) in sorted(BY_MASK.items()):
        print(f"ACCENUM selection {entry} kappa={kappa:g}: {n_mask} by mask, {n_value} by value only")
