"""tests/hp_games.py has to earn its trust before tests/test_gpu_accuracy_enum.py leans on it, and the case table of
tests/accuracy_enum_cases.py has to be one that cannot hide a failure.

1. Every helper against the existing fp64 oracle of the same game, on well-conditioned data at p <= 8, to 1e-12.
2. Against mpmath.  The helpers run in either arithmetic of hp_ref: at 50 digits they agree with hp_ref.Problem(ar=MP())
   to 1e-17 relative (the formulas, weights and index maps); the long-double run of the same code -- the truth the GPU
   tests use -- is then held to hp_ref's own rule against the 50-digit values, max(e_plain / 256, 1e-17): no
   long-double evaluation can be 1e-17 relative at kappa(G) = 1e12, its unit round-off being 5.4e-20.
3. The case table, from the truth alone: (a) no NOT_PD excuse is possible at kappa <= 1e4 -- every problem, fold and
   replicate has its true smallest relative pivot >= 100 x the engine's threshold 16 p eps; (b) at kappa <= 1e3 the
   truth's winner of every size (and every rank of the top lists) is clear of its neighbours by more than twice the
   case's tolerance, so the GPU test asserts the winning masks themselves; (c) every case's pivot / threshold is
   printed, to read the GPU log against."""
import time

import numpy as np
import pytest

import accuracy_enum_cases as C
import boot_ref
import cv_ref
import hp_games as HG
import hp_ref
import owen_ref
import perm_ref
from test_groups_host import group_shapley, group_values, labels_of
from test_multi_groups_host import multi_group_oracle, multi_group_values
from test_multi_host import multi_data, multi_gram_problem, multi_oracle_batched, multi_subset_values, with_responses
from test_subsets_host import data, exact_shapley, gram_problem, subset_values

TOL = dict(rtol=0, atol=1e-12)
LABELS8 = labels_of([2, 1, 3], 2, seed=8)


# ---- 1. against the fp64 oracles -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("reg", [0.0, 0.05])
def test_many_responses_against_the_multi_oracles(reg):
    p, m = 8, 5
    D = multi_data(p, m, seed=3)
    prob = multi_gram_problem(*D, reg)
    ref = HG.MultiProblem(*D, reg=reg)
    masks = np.arange(1 << p, dtype=np.uint64)
    np.testing.assert_allclose(ref.values(masks).astype(np.float64), multi_subset_values(*prob, masks), **TOL)
    np.testing.assert_allclose(ref.shapley(), multi_oracle_batched(*D, reg=reg), **TOL)
    gm = np.arange(8, dtype=np.uint64)
    np.testing.assert_allclose(ref.group_values(gm, LABELS8).astype(np.float64),
                               multi_group_values(*prob, LABELS8, gm), **TOL)
    np.testing.assert_allclose(ref.shapley(LABELS8), multi_group_oracle(*D, LABELS8, reg=reg), **TOL)
    np.testing.assert_allclose(ref.shapley().sum(axis=1), ref.total(), **TOL)
    np.testing.assert_allclose(ref.shapley(LABELS8).sum(axis=1), ref.total(LABELS8), **TOL)
    assert 0 < ref.min_pivot <= 1


def test_one_factorisation_serves_every_response_and_is_hp_refs():
    """Column r of the table is hp_ref.Problem's value on response r alone, to long double's rounding, and the pivots
    kept are hp_ref's."""
    p, m = 7, 3
    D = multi_data(p, m, seed=5)
    ref = HG.MultiProblem(*D)
    masks = np.arange(1 << p, dtype=np.uint64)
    v = ref.values(masks)
    for r in range(m):
        one = hp_ref.Problem(D[0], D[1], D[2][:, r], D[3][:, r])
        want = np.array([one.mask_value(k) for k in masks], dtype=np.longdouble)
        assert float(np.abs(v[:, r] - want).max()) < 1e-17
        assert ref.min_pivot == pytest.approx(one.min_pivot, rel=1e-15)
    np.testing.assert_array_equal(ref.shapley()[0], HG.MultiProblem(D[0], D[1], D[2][:, 0], D[3][:, 0]).shapley()[0])


@pytest.mark.parametrize("sizes, nb", [([3, 2, 2], 1), ([4, 1, 2], 0), ([8], 0), ([1] * 6, 2)])
def test_owen_against_owen_ref(sizes, nb):
    labels = labels_of(sizes, nb, seed=sum(sizes))
    d = data(len(labels), seed=len(labels))
    ref = hp_ref.Problem(*d)
    got = HG.owen(ref, labels)
    np.testing.assert_allclose(got, owen_ref.owen_values(*gram_problem(*d), labels), **TOL)
    np.testing.assert_array_equal(got[labels == -1], 0.0)
    phi = ref.shapley(labels)
    for k in range(len(sizes)):
        assert abs(got[labels == k].sum() - phi[k]) < 1e-14
    assert 0 < ref.min_pivot <= 1


def test_fold_problems_against_cv_ref():
    p, n, K = 8, 70, 3
    X, y = cv_ref.data(p, n, seed=1)
    ids = cv_ref.fold_ids(n, K, seed=2)
    v, vf = cv_ref.cv_values(X, y, ids, K, 0.1)
    refs = HG.RowsProblem.of_folds(X, y, ids, K, 0.1)
    tabs = np.stack([r.all_values()[:, 0] for r in refs], axis=1)
    np.testing.assert_allclose(tabs.astype(np.float64), vf.astype(np.float64), **TOL)
    np.testing.assert_allclose(tabs.sum(axis=1).astype(np.float64), v.astype(np.float64), **TOL)
    phi = sum(r.shapley(raw=True) for r in refs)
    np.testing.assert_allclose(phi.astype(np.float64), cv_ref.shapley(v, p).astype(np.float64), **TOL)
    for f, (r, prob) in enumerate(zip(refs, HG.plain_fold_problems(X, y, ids, K, 0.1))):
        for a, b in zip((r.G, r.g, r.H, r.h, r.yy), prob):
            np.testing.assert_allclose(np.asarray(a, dtype=np.float64), b, rtol=1e-13, atol=0)
        assert float(r.mask_value(37)) == pytest.approx(float(vf[37, f]), abs=1e-15)
        assert float(r.group_value(5, LABELS8)) == pytest.approx(float(r.group_values([5], LABELS8)[0, 0]), abs=1e-17)
        np.testing.assert_allclose(r.shapley(LABELS8), group_shapley(*prob, LABELS8), **TOL)
        # a fold's pivots are its own: those of its training complement alone
        alone = hp_ref.Problem(X[ids != f], X[ids == f], y[ids != f], y[ids == f], reg=0.1)
        alone.shapley()
        assert r.min_pivot == pytest.approx(alone.min_pivot, rel=1e-12)


@pytest.mark.parametrize("r", [0, 3])
def test_weighted_rows_against_boot_ref(r):
    """The counts of tests/boot_ref.py as weights give the problem of the explicitly resampled rows."""
    p, seed = 8, 11
    Xa, Xe, ya, ye = d = data(p, seed=4)
    ia, ie = boot_ref.indices(seed, r, 0, len(ya)), boot_ref.indices(seed, r, 1, len(ye))
    Za, Ze = np.column_stack([Xa, ya]), np.column_stack([Xe, ye])
    wa, we = boot_ref.counts(seed, r, 0, len(ya)), boot_ref.counts(seed, r, 1, len(ye))
    assert (wa == 0).any() and wa.max() > 1
    ref = HG.RowsProblem(Za, wa, Ze, we, reg=0.02)
    drawn = (Xa[ia], Xe[ie], ya[ia], ye[ie])
    np.testing.assert_allclose(ref.shapley(), exact_shapley(*gram_problem(*drawn, reg=0.02)), **TOL)
    np.testing.assert_allclose(ref.shapley(LABELS8), group_shapley(*gram_problem(*drawn, reg=0.02), LABELS8), **TOL)
    rows = hp_ref.Problem(*drawn, reg=0.02)
    np.testing.assert_allclose(ref.shapley(), rows.shapley(), rtol=0, atol=1e-15)
    assert ref.min_pivot == pytest.approx(rows.min_pivot, rel=1e-12)
    assert float(ref.mask_value(201)) == pytest.approx(float(rows.mask_value(201)), abs=1e-15)
    plain = HG.plain_rows_problem(Za, wa, Ze, we, 0.02)
    for a, b in zip(plain, gram_problem(*drawn, reg=0.02)):
        np.testing.assert_allclose(a, b, rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(subset_values(*plain, np.array([255], dtype=np.uint64))[0], float(ref.mask_value(255)),
                               **TOL)


@pytest.mark.parametrize("grouped", [False, True])
def test_permuted_responses_against_perm_ref(grouped):
    p, R, seed = 8, 3, 9
    d = data(p, seed=6)
    labels = LABELS8 if grouped else None
    eng = perm_ref.PermOracleEngine()
    eng.perm_load(*d, 0.0)
    want, _, _, _ = eng.perm_run(R, seed, labels)
    Ya = perm_ref.permuted_responses(d[2], seed, range(R), 0)
    Ye = perm_ref.permuted_responses(d[3], seed, range(R), 1)
    np.testing.assert_allclose(HG.MultiProblem(d[0], d[1], Ya, Ye).shapley(labels), want, **TOL)
    np.testing.assert_allclose(HG.MultiProblem(*d).shapley(labels)[0], eng.perm_observed(labels)[0], **TOL)


# ---- 2. against mpmath -----------------------------------------------------------------------------------------------------
def test_against_mpmath_at_50_digits():
    mpmath = pytest.importorskip("mpmath", reason="mpmath does not import")
    del mpmath
    p, m, kappa = 4, 3, 1e6
    mp = hp_ref.MP(50)
    d = hp_ref.gen(p, 4 * p + 50, 3 * p + 40, kappa, seed=4)
    D = with_responses(*d, m, 4)
    labels = np.array([0, 1, -1, 0])
    olab = np.array([0, 0, 1, 0])
    masks, gmasks = np.arange(1 << p, dtype=np.uint64), np.arange(4, dtype=np.uint64)
    Za, Ze = np.column_stack([d[0], d[2]]), np.column_stack([d[1], d[3]])
    wa, we = C.boot_weights(d[0], 1)[3], C.boot_weights(d[1], 2)[3]
    got = {}
    for ar in (mp, hp_ref.LD):
        multi = HG.MultiProblem(*D, ar=ar)
        rows = HG.RowsProblem(Za, wa, Ze, we, ar=ar)
        got[ar.name] = dict(values=multi.values(masks), group_values=multi.group_values(gmasks, labels),
                            phi=multi.shapley(raw=True), group_phi=multi.shapley(labels, raw=True),
                            owen=HG.owen(hp_ref.Problem(*d, ar=ar), olab, raw=True)[None, :],
                            rows_phi=rows.shapley(raw=True)[None, :], rows_value=rows.values(masks),
                            pivot=multi.min_pivot)
    # the 50-digit run against hp_ref.Problem at 50 digits, one response at a time: 1e-17 relative
    rel = lambda a, b: abs(float((a - b) / b)) if b != 0 else abs(float(a))
    exact = got["mpmath"]
    for r in range(m):
        one = hp_ref.Problem(D[0], D[1], D[2][:, r], D[3][:, r], ar=mp)
        for k in masks:
            assert rel(exact["values"][int(k), r], one.mask_value(k)) < 1e-17
        for k in gmasks:
            assert rel(exact["group_values"][int(k), r], one.group_value(k, labels)) < 1e-17
        for a, b in zip(exact["phi"][r], one.shapley(raw=True)):
            assert rel(a, b) < 1e-17
        for a, b in zip(exact["group_phi"][r], one.shapley(labels, raw=True)):
            assert rel(a, b) < 1e-17
    # Owen at 50 digits: labels of singletons give the Shapley value, and a group's columns sum to its phi
    one = hp_ref.Problem(*d, ar=mp)
    for a, b in zip(HG.owen(hp_ref.Problem(*d, ar=mp), np.arange(p), raw=True), one.shapley(raw=True)):
        assert rel(a, b) < 1e-17
    gphi = one.shapley(olab, raw=True)
    assert rel(exact["owen"][0][olab == 0].sum(), gphi[0]) < 1e-17 and rel(exact["owen"][0][2], gphi[1]) < 1e-17
    # the weighted rows at 50 digits: integer weights are repeated rows
    rep_a, rep_e = np.repeat(np.arange(len(Za)), wa.astype(int)), np.repeat(np.arange(len(Ze)), we.astype(int))
    drawn = hp_ref.Problem(d[0][rep_a], d[1][rep_e], d[2][rep_a], d[3][rep_e], ar=mp)
    for a, b in zip(exact["rows_phi"][0], drawn.shapley(raw=True)):
        assert rel(a, b) < 1e-17
    # long double against 50 digits, by hp_ref's rule
    prob = multi_gram_problem(*D)
    plain = dict(values=multi_subset_values(*prob, masks), group_values=multi_group_values(*prob, labels, gmasks),
                 phi=multi_oracle_batched(*D), group_phi=multi_group_oracle(*D, labels),
                 owen=owen_ref.owen_values(*gram_problem(*d), olab)[None, :],
                 rows_phi=exact_shapley(*HG.plain_rows_problem(Za, wa, Ze, we))[None, :],
                 rows_value=subset_values(*HG.plain_rows_problem(Za, wa, Ze, we), masks)[:, None])
    for key, ref64 in plain.items():
        want, ld = exact[key], got["longdouble"][key]
        e_ld = max(abs(float(mp.exact(a) - b)) for a, b in zip(np.ravel(ld), np.ravel(want)))
        e_plain = float(np.abs(ref64 - mp.to_float(want)).max())
        print(f"MP {key}: long double {e_ld:.2e}, plain fp64 {e_plain:.2e}")
        assert e_ld <= max(e_plain / 256, 1e-17)
    assert got["longdouble"]["pivot"] == pytest.approx(exact["pivot"], rel=1e-6)


# ---- 3. the case table -----------------------------------------------------------------------------------------------------
def test_the_case_table_cannot_hide_a_failure():
    t0 = time.perf_counter()
    for kappa in C.KAPPAS:
        for name, t in C.all_truths(kappa):
            ratios = t.ratios()
            print(f"CASE {name} kappa={kappa:g}: true pivot / threshold = "
                  + " ".join(f"{x:.3g}" for x in ratios) + f"; worst e_plain {max(t.e_plain.values()):.2e}")
            assert np.all(np.isfinite(ratios)) and np.all(ratios > 0)
            assert all(np.all(np.isfinite(w)) for w in t.want.values())
            if kappa <= 1e4:                                                     # (a)
                assert ratios.min() >= 100, f"{name} kappa={kappa:g}: an excuse would be possible"
    seconds = time.perf_counter() - t0
    print(f"CASE host seconds of all truths: {seconds:.1f}")
    assert seconds < 120


@pytest.mark.parametrize("kappa", [k for k in C.KAPPAS if k <= 1e3])
def test_selection_cases_have_clear_winners(kappa):
    """(b): every size's winner, and every rank of the top lists, is clear of its neighbours by more than 2 tol."""
    for name, t in C.selection_cases(kappa):
        tol = C.tol_of(t.e_plain["v_all"])
        gaps = C.margins(C.ranking(t.table, 10, C.N_BEST), C.N_BEST)
        print(f"CASE selection {name} kappa={kappa:g}: smallest margin {np.nanmin(gaps):.3e}, 2 tol {2 * tol:.3e}")
        assert np.nanmin(gaps) > 2 * tol
        assert t.pivots.min() / C.threshold(10) >= 100


def test_ranking_and_margins_on_a_hand_made_table():
    v = np.array([0.0, 0.5, 0.7, 0.9], dtype=np.longdouble)            # p = 2: {}, {0}, {1}, {0, 1}
    rank = C.ranking(v, 2, 3)
    assert [[m for _, m in row] for row in rank] == [[0], [2, 1], [3]]
    gaps = C.margins(rank, 3)
    assert gaps[1, 0] == pytest.approx(0.2) and gaps[1, 1] == pytest.approx(0.2) and np.isinf(gaps[0, 0])
    assert np.isnan(gaps[0, 1]) and np.isnan(gaps[1, 2])
    tie = C.ranking(np.array([0.0, 0.5, 0.5, 0.9], dtype=np.longdouble), 2, 1)
    assert [m for _, m in tie[1]] == [1, 2]                              # on equal values the smaller mask


def test_the_shapes_are_what_the_table_says():
    """What needs no engine: the responses fill one chunk and one more, the folds and weights are the stated ones."""
    from ls_spa._engine import HipEngine
    assert C.MULTI_RB == HipEngine.MULTI_RB and C.M_RESP == C.MULTI_RB + 1
    ids = C.cv_folds(90, 10)
    assert [(ids == f).sum() for f in range(3)] == [12, 45, 33]
    w = C.boot_weights(C.data_of(10, 1e3)[0], 1)
    assert w.shape == (4, 90) and (w[0] == 1).all() and w[1].sum() == 90 and w[2].sum() == 90
    assert (w[3] == 0).sum() == 30 and w[3].max() == 7 and set(np.unique(w[3])) == set(range(8))
    lop = C.lopsided_folds(C.LOPSIDED_N, 10, C.LOPSIDED_SEED)
    assert [(lop == f).sum() for f in range(3)] == [C.LOPSIDED_N - 10, 5, 5]


def test_one_replicate_and_one_fold_are_markedly_worse_than_their_siblings():
    """What lets the GPU tests tell one info word from another: the hand-made replicate is several times nearer the
    threshold than the others and alone inside the excusable band at the top kappa; fold 0 of the lopsided layout is
    far under the threshold at kappa >= 1e6 (it must be flagged) while its siblings are far above (they must not be)."""
    top = C.boot_truth(C.KAPPAS[-1]).ratio
    assert top[3] < 100 <= top[:3].min() and top[3] < top[:3].min() / 4
    for kappa in C.KAPPAS:
        r = C.cv_truth(kappa, 0.0, "lopsided").ratio
        print(f"CASE cv lopsided kappa={kappa:g}: fold pivots / threshold {r[0]:.3g} {r[1]:.3g} {r[2]:.3g}")
        assert r[0] < r[1:].min() / 50
        if kappa >= 1e6:
            assert r[0] < 0.05 and r[1:].min() >= 100
    assert len(C.LABELS_OWEN) == 17 and len(C.LABELS_G10) == 24 and len(C.LABELS_G12) == 40 and len(C.LABELS_P10) == 10
