"""The ridge path of the K-fold CV attribution on the MI355X (lsspa_cv_path_shapley, lsspa_cv_path_groups_shapley;
the path kernels of csrc/k_cv.hip): every row bit for bit against ls_spa_cv with that ridge value, whatever the block,
the order and the length of the path; isolation from the loaded folds; the long-double truth; credit moving between
collinear columns as tests/cv_ref.py says it does; failed pivots named by ridge value and fold; the C-level refusals."""
import ctypes as C
import functools
import warnings

import numpy as np
import pytest

import cv_ref as R
import hp_ref
from ls_spa import CVGroupPathResults, CVPathResults, ls_spa_cv, ls_spa_cv_path
from ls_spa import _native as N
from test_cv_path_host import GPU_BLOCKS, GPU_COLUMN_CASES, GPU_GROUP_CASES, GPU_REGS, gpu_group_labels

pytestmark = pytest.mark.gpu

NOT_PD = 1
ERR_ARG, ERR_STATE = 1, 3


@functools.lru_cache(maxsize=None)
def data(p, K, n):
    X, y = R.data(p, n, seed=100 * p + K)
    ids = R.fold_ids(n, K, seed=7)
    for a in (X, y, ids):
        a.setflags(write=False)
    return X, y, ids


_want = {}


def want_rows(engine, p, K, n, labels=None):
    """reg -> ls_spa_cv(X, y, reg=reg) on the kept engine, for the ridge values of GPU_REGS: computed once a case."""
    key = (p, K, n, None if labels is None else tuple(labels))
    if key not in _want:
        X, y, ids = data(p, K, n)
        _want[key] = {r: ls_spa_cv(X, y, r, ids, groups=labels, _engine=engine) for r in set(GPU_REGS)}
    return _want[key]


def assert_rows(got, regs, want, grouped=False):
    """row l of the engine's path output against ls_spa_cv's result for regs[l], bit for bit"""
    for l, r in enumerate(regs):
        ref = want[r]
        np.testing.assert_array_equal(got[0][l], ref.attribution)
        np.testing.assert_array_equal(got[1][l], ref.fold_attribution)
        np.testing.assert_array_equal(got[2][l], ref.fold_r_squared)
        if grouped:
            np.testing.assert_array_equal(got[3][l], ref.fold_baseline_r_squared)
        assert (got[-1][l] == 0).all()


# ---- 1. bitwise rows ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p, K", GPU_COLUMN_CASES)
def test_rows_have_the_bits_of_ls_spa_cv(engine, p, K):
    n = 120
    X, y, ids = data(p, K, n)
    want = want_rows(engine, p, K, n)
    assert len(set(GPU_REGS)) == 4 and len(GPU_REGS) == 5            # a repeated value among them
    engine.cv_load(X, y, ids, K, 0.7)                                # the load's own reg plays no part
    try:
        for block in GPU_BLOCKS:
            assert_rows(engine.cv_path_shapley(GPU_REGS, block), GPU_REGS, want)
            plan = engine.debug_cv_path_plan(p, K, len(GPU_REGS), block)
            assert engine.cv_timing()["launches"] == plan["launches"]
        assert_rows(engine.cv_path_shapley(GPU_REGS[::-1], 2), GPU_REGS[::-1], want)
        for r in (0.0, 10.0):                                        # L = 1
            assert_rows(engine.cv_path_shapley([r]), [r], want)
    finally:
        engine.cv_free()


@pytest.mark.parametrize("p, K, reps, cuts", [(20, 5, 10, 1), (24, 5, 4, 1), (27, 2, 1, 2)])
def test_rows_where_the_launches_are_cut_differently(engine, p, K, reps, cuts):
    """The sizes at which the path's launches differ from the one-value call's.  p = 20: a unit has two steps and ten
    problems share a launch where the call's five do.  p = 24: a launch holds four problems, so the call runs folds
    0 .. 3 together and fold 4 alone -- by the one-problem instantiation of the kernel --, the path 4 + 4 + 2: fold 4 of
    the first value and folds 0 and 1 of the second run beside other neighbours, by the other instantiation.  p = 27: a
    problem alone takes two launches (the cut of a unit's steps shows in the bits) and no two share one."""
    n, regs = 300, [0.1, 1e-3]
    X, y, ids = data(p, K, n)
    plan = engine.debug_cv_path_plan(p, K, len(regs))
    assert plan["reps"] == reps and -(-plan["per"] // plan["steps"]) == cuts and plan["blocks"] == 1
    want = {r: ls_spa_cv(X, y, r, ids, _engine=engine) for r in regs}
    engine.cv_load(X, y, ids, K, 0.0)
    try:
        assert_rows(engine.cv_path_shapley(regs), regs, want)
        assert engine.cv_timing()["launches"] == plan["launches"] == -(-len(regs) * K // reps) * cuts
    finally:
        engine.cv_free()


@pytest.mark.parametrize("case", [0, 1], ids=["g3-p7-baseline2", "g6-p40"])
def test_group_rows_have_the_bits_of_ls_spa_cv(engine, case):
    labels, K = GPU_GROUP_CASES[case]
    p, n = len(labels), 200
    assert (p, int(labels.max()) + 1, int((labels < 0).sum())) in [(7, 3, 2), (40, 6, 0)]
    X, y, ids = data(p, K, n)
    want = want_rows(engine, p, K, n, labels)
    cols = want_rows(engine, p, K, n) if p <= 32 else None
    engine.cv_groups_load(X, y, ids, K, 0.7)
    try:
        for block in GPU_BLOCKS:
            assert_rows(engine.cv_path_groups_shapley(labels, GPU_REGS, block), GPU_REGS, want, grouped=True)
            plan = engine.debug_cv_path_groups_plan(labels, K, len(GPU_REGS), block)
            assert engine.cv_timing()["launches"] == plan["launches"]
        assert_rows(engine.cv_path_groups_shapley(labels, GPU_REGS[::-1], 2), GPU_REGS[::-1], want, grouped=True)
        assert_rows(engine.cv_path_groups_shapley(labels, [1e-3]), [1e-3], want, grouped=True)
        if p <= 32:                                                  # after a grouped load of p <= 32 both families work
            assert_rows(engine.cv_path_shapley(GPU_REGS, 3), GPU_REGS, cols)
        else:
            with pytest.raises(N.LSSPANativeError, match="at most p = 32 features"):
                engine.cv_path_shapley(GPU_REGS)
            assert_rows(engine.cv_path_groups_shapley(labels, [0.1]), [0.1], want, grouped=True)
    finally:
        engine.cv_free()


def test_group_rows_over_several_units_one_problem_a_launch(engine):
    """tests/cv_groups_ref.py's layout of 18 groups over 64 columns: 8192 units of four steps, a launch's bound filled by
    one problem, so that no two problems share a launch."""
    import cv_groups_ref as GR
    labels, K, n, regs = GR.multi_labels(), GR.MULTI_K, GR.MULTI_N, [0.1, 1e-3]
    X, y = R.data(len(labels), n, seed=GR.MULTI_SEED)
    ids = R.fold_ids(n, K, seed=GR.FOLD_SEED)
    plan = engine.debug_cv_path_groups_plan(labels, K, len(regs))
    assert plan["units"] == 8192 and plan["per"] == 4 and plan["reps"] == 1
    want = {r: ls_spa_cv(X, y, r, ids, groups=labels, _engine=engine) for r in regs}
    engine.cv_groups_load(X, y, ids, K, 0.0)
    try:
        assert_rows(engine.cv_path_groups_shapley(labels, regs), regs, want, grouped=True)
        assert engine.cv_timing()["launches"] == plan["launches"] == len(regs) * K * -(-plan["per"] // plan["steps"])
    finally:
        engine.cv_free()


def test_public_call_and_determinism():
    p, K, n = 7, 3, 120
    X, y, ids = data(p, K, n)
    regs = [10.0, 0.0, 0.1]
    res = ls_spa_cv_path(X, y, regs, K, seed=7)
    again = ls_spa_cv_path(X, y, regs, ids)
    assert isinstance(res, CVPathResults)
    np.testing.assert_array_equal(res.fold_ids, ids)
    for l, r in enumerate(regs):
        one = ls_spa_cv(X, y, r, K, seed=7)
        np.testing.assert_array_equal(res.attribution[l], one.attribution)
        np.testing.assert_array_equal(res.fold_attribution[l], one.fold_attribution)
        np.testing.assert_array_equal(res.fold_r_squared[l], one.fold_r_squared)
        np.testing.assert_array_equal(res.theta[l], one.theta)
        assert res.r_squared[l] == one.r_squared
    for a, b in zip((res.attribution, res.fold_attribution, res.fold_r_squared, res.theta),
                    (again.attribution, again.fold_attribution, again.fold_r_squared, again.theta)):
        np.testing.assert_array_equal(a, b)                          # two calls agree bitwise
    assert res.best_index == int(np.argmax(res.r_squared)) and res.within_one_se[res.best_index]
    labels = gpu_group_labels(3, 7, 2)
    grp = ls_spa_cv_path(X, y, regs, K, seed=7, groups=labels)
    assert isinstance(grp, CVGroupPathResults)
    for l, r in enumerate(regs):
        one = ls_spa_cv(X, y, r, K, seed=7, groups=labels)
        np.testing.assert_array_equal(grp.attribution[l], one.attribution)
        np.testing.assert_array_equal(grp.fold_baseline_r_squared[l], one.fold_baseline_r_squared)
        assert grp.r_squared[l] == one.r_squared and grp.baseline_r_squared[l] == one.baseline_r_squared


# ---- 2. isolation ------------------------------------------------------------------------------------------------------
def test_the_loaded_folds_are_not_touched(engine):
    p, K, n = 7, 3, 120
    X, y, ids = data(p, K, n)
    labels = gpu_group_labels(3, 7, 2)
    engine.cv_load(X, y, ids, K, 0.25)
    try:
        own = engine.cv_shapley()
        best = engine.cv_best()
        probs = [engine.cv_get_problem(f) for f in range(K)]
        path = engine.cv_path_shapley([5.0, 0.0, 0.25])
        best_after = engine.cv_best()                                # a path call between two cv_best calls
        engine.cv_path_groups_shapley(labels, [3.0, 0.0])
        own_after = engine.cv_shapley()
        grp = engine.cv_groups_shapley(labels)
        for a, b in zip(own + best, own_after + best_after):
            np.testing.assert_array_equal(a, b)
        for f in range(K):
            for a, b in zip(probs[f], engine.cv_get_problem(f)):
                np.testing.assert_array_equal(a, b)
        for a, b in zip(own[:3], path[:3]):                          # the load's own reg, as a row of a path
            np.testing.assert_array_equal(a, b[2])
        assert np.abs(path[0][0] - own[0]).max() > 1e-6              # the other rows are other problems
        grp_row = engine.cv_path_groups_shapley(labels, [0.25])
        for a, b in zip(grp, grp_row):
            np.testing.assert_array_equal(a, b[0])
    finally:
        engine.cv_free()


# ---- 3. the truth ------------------------------------------------------------------------------------------------------
def test_attribution_against_the_long_double_truth(engine):
    """p = 7, K = 3, reg = 0.1: per fold problem the brute-force Shapley values of tests/hp_ref.py in long double (trained
    on the other folds, tested on the fold), rescaled from the fold's ||y_f||^2 to the pooled ||y||^2, and their sum; the
    tolerance is tests/test_gpu_cv.py's for one ridge value."""
    p, K, n, reg = 7, 3, 120, 0.1
    X, y, ids = data(p, K, n)
    yl = np.asarray(y, dtype=np.longdouble)
    fold = []
    for f in range(K):
        te = ids == f
        pr = hp_ref.Problem(X[~te], X[te], y[~te], y[te], reg)
        fold.append(pr.shapley(raw=True) * (yl[te] @ yl[te]) / (yl @ yl))
    truth = np.asarray(sum(fold), dtype=np.float64)
    engine.cv_load(X, y, ids, K, 0.0)
    try:
        phi, phi_fold, r2_fold, info = engine.cv_path_shapley([3.0, reg])
    finally:
        engine.cv_free()
    print("max |phi - truth|", np.abs(phi[1] - truth).max())
    assert (info == 0).all()
    np.testing.assert_allclose(phi[1], truth, rtol=0, atol=1e-11)
    np.testing.assert_allclose(phi_fold[1], np.asarray(fold, dtype=np.float64), rtol=0, atol=1e-11)
    v, vf = R.cv_values(X, y, ids, K, reg)
    np.testing.assert_allclose(r2_fold[1], vf[-1].astype(np.float64), rtol=0, atol=1e-11)
    assert abs(phi[1].sum() - float(v[-1])) < 1e-11


# ---- 4. credit moves between collinear columns -------------------------------------------------------------------------
def test_collinear_columns_share_the_credit_as_the_ridge_grows(engine):
    """Columns 0 and 1 are nearly the same column and y depends on column 0: the unpenalised fit credits them unequally,
    and the ridge pulls their attributions together.  What "together" means is read from tests/cv_ref.py, not written
    down here.  Tolerance: the smallest eigenvalue of G_f is about 0.2^2 / 2 against a largest of about 2, a condition
    number of 1e2, so fp64 keeps the attribution to about 1e2 eps ~ 1e-14; 1e-11 is tests/test_gpu_cv.py's bound."""
    p, K, n = 6, 3, 150
    rng = np.random.default_rng(17)
    X = rng.standard_normal((n, p))
    X[:, 1] = X[:, 0] + 0.2 * rng.standard_normal(n)
    y = 2.0 * X[:, 0] + 0.5 * X[:, 3] + 0.3 * rng.standard_normal(n)
    ids = R.fold_ids(n, K, seed=3)
    regs = [1e-3, 1e-2, 0.1, 1.0, 10.0]
    truth = np.array([R.shapley(R.cv_values(X, y, ids, K, r)[0], p).astype(np.float64) for r in regs])
    want_gap = np.abs(truth[:, 0] - truth[:, 1])
    print("truth's |phi_0 - phi_1| along the path", want_gap)
    assert (np.diff(want_gap) < -1e-6).all()                         # the fixture does what it is meant to do
    engine.cv_load(X, y, ids, K, 0.0)
    try:
        phi, _, _, info = engine.cv_path_shapley(regs)
    finally:
        engine.cv_free()
    assert (info == 0).all()
    gap = np.abs(phi[:, 0] - phi[:, 1])
    np.testing.assert_allclose(phi, truth, rtol=0, atol=1e-11)
    np.testing.assert_allclose(gap, want_gap, rtol=0, atol=2e-11)
    assert (np.diff(gap) < 0).all()


# ---- 5. failed pivots --------------------------------------------------------------------------------------------------
def test_failed_pivot_names_the_ridge_value_and_the_fold(engine):
    p, K, n = 8, 3, 120
    X, y = R.data(p, n, seed=800)
    ids = (np.arange(n) % K).astype(np.int32)
    X = X.copy()
    X[ids != 1, 7] = 0.0                 # column 7 is constant zero in the training complement of fold 1
    regs = [0.1, 0.0, 0.1]
    engine.cv_load(X, y, ids, K, 0.0)
    try:
        phi, phi_fold, r2_fold, info = engine.cv_path_shapley(regs)
        again = engine.cv_path_shapley(regs)
    finally:
        engine.cv_free()
    assert info[1, 1] & NOT_PD and info[1, 0] == 0 and info[1, 2] == 0 and (info[[0, 2]] == 0).all()
    assert np.isfinite(phi[[0, 2]]).all() and np.isfinite(phi_fold[[0, 2]]).all() and np.isfinite(r2_fold[[0, 2]]).all()
    assert np.isfinite(phi_fold[1, [0, 2]]).all()
    for a, b in zip((phi[[0, 2]], phi_fold[[0, 2]], r2_fold, info), (again[0][[0, 2]], again[1][[0, 2]], again[2], again[3])):
        np.testing.assert_array_equal(a, b)
    truth = R.shapley(R.cv_values(X, y, ids, K, 0.1)[0], p).astype(np.float64)
    np.testing.assert_allclose(phi[0], truth, rtol=0, atol=1e-11)
    np.testing.assert_array_equal(phi[0], phi[2])
    with pytest.warns(RuntimeWarning, match=r"ridge value 0 \(regs\[1\]\): fold\(s\) 1;") as rec:
        res = ls_spa_cv_path(X, y, regs, ids, _engine=engine)
    assert "regs[0]" not in str(rec[0].message) and "regs[2]" not in str(rec[0].message)
    np.testing.assert_array_equal(res.attribution[[0, 2]], phi[[0, 2]])
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ls_spa_cv_path(X, y, [0.1, 1.0], ids, _engine=engine)


# ---- 6. the C-level refusals -------------------------------------------------------------------------------------------
def test_c_level_refusals_leave_the_folds_usable(engine):
    p, K, n = 5, 2, 120
    X, y, ids = data(p, K, n)
    lib, h = engine._lib, engine._h
    L = 3
    regs = np.array([0.0, 0.1, 1.0])
    phi, fold, r2, info = np.empty((L, p)), np.empty((L, K, p)), np.empty((L, K)), np.zeros((L, K), dtype=np.int32)
    base = np.empty((L, K))
    labels = np.array([-1, 0, 0, 1, 1], dtype=np.int32)
    null_d, null_i = C.POINTER(C.c_double)(), C.POINTER(C.c_int32)()

    def cols(regs=regs, L=L, block=0, phi_=None, regs_ptr=None):
        return lib.lsspa_cv_path_shapley(h, N.dptr(regs) if regs_ptr is None else regs_ptr, L, block,
                                         N.dptr(phi) if phi_ is None else phi_, N.dptr(fold), N.dptr(r2), N.iptr(info))

    def grps(regs=regs, L=L, block=0, lab=labels, g=2, base_=None):
        return lib.lsspa_cv_path_groups_shapley(h, N.iptr(lab), g, N.dptr(regs), L, block, N.dptr(phi), N.dptr(fold),
                                                N.dptr(r2), N.dptr(base) if base_ is None else base_, N.iptr(info))

    engine.cv_free()
    assert cols() == ERR_STATE and grps() == ERR_STATE               # nothing loaded
    engine.cv_load(X, y, ids, K, 0.5)
    try:
        own = engine.cv_shapley()
        for call in (cols, grps):
            assert call(L=0) == ERR_ARG and call(L=257) == ERR_ARG and call(L=-1) == ERR_ARG
            assert call(block=-1) == ERR_ARG
            for bad in (-1e-300, np.nan, np.inf, -np.inf):
                assert call(regs=np.array([0.0, 0.1, bad])) == ERR_ARG
                assert b"regs[2]" in lib.lsspa_last_error(h)
        assert cols(phi_=null_d) == ERR_ARG and cols(regs_ptr=null_d) == ERR_ARG and grps(base_=null_d) == ERR_ARG
        assert grps(lab=np.array([-1, 0, 0, 2, 2], dtype=np.int32), g=3) == ERR_ARG      # a gap in the numbering
        assert grps(g=33) == ERR_ARG
        assert lib.lsspa_cv_path_shapley(None, N.dptr(regs), L, 0, N.dptr(phi), N.dptr(fold), N.dptr(r2),
                                         N.iptr(info)) == ERR_ARG
        assert cols() == 0 and grps() == 0                           # the folds are still usable ...
        for a, b in zip(own, engine.cv_shapley()):                   # ... and still the load's
            np.testing.assert_array_equal(a, b)
    finally:
        engine.cv_free()
    wide = gpu_group_labels(6, 40, 0)
    Xw, yw, idw = data(40, 2, 200)
    engine.cv_groups_load(Xw, yw, idw, 2, 0.0)
    try:
        wphi, wfold = np.empty((L, 40)), np.empty((L, 2, 40))
        rc = lib.lsspa_cv_path_shapley(h, N.dptr(regs), L, 0, N.dptr(wphi), N.dptr(wfold), N.dptr(r2), N.iptr(info))
        assert rc == ERR_STATE                                       # the column call after a load of 40 columns
        got = engine.cv_path_groups_shapley(wide, [0.1])
        assert (got[-1] == 0).all()
    finally:
        engine.cv_free()
