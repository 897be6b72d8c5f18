"""The running mean and covariance and the device error estimator against a long-double truth, on chosen lift vectors.

Every case injects a seeded matrix as a launched batch (lsspa_debug_lift_inject; the problem is an identity Gram matrix of
the case's dimension), collects it in stated chunks through a stated form, reads the statistics -- and, where the
estimator runs, every check and the sums D and s -- and asserts  err <= bound  against tests/hp_stats.py: the truth in
long double, the bound counted from the kernels' roundings (derived there, no fitted constant).  The cases, their forms,
shapes and input families are hp_stats.STATS_CASES / EST_CASES; tests/test_hp_stats_host.py has vetted each of them on
the CPU: a plain fp64 restatement of the route stays inside the bound, three mutations of it leave it by more than 100 x.

Printed per case (SACC ...): the worst err / bound of every asserted quantity and the relative error of the variances;
DESIGN.md, Numerics, has the table measured on the MI355X."""
import numpy as np
import pytest

import hp_stats as S
from ls_spa._engine import HipEngine, debug_stats_slices
from ls_spa._native import LSSPANativeError

pytestmark = pytest.mark.gpu

STATS = [(name, p, plan, fam) for name, p, plan, fams in S.STATS_CASES for fam in fams]
EST = [(name, p, how, counts, stride, fam) for name, p, how, counts, stride, fams in S.EST_CASES for fam in fams]
ID0 = 3       # sample i of a case has id ID0 + stride * i


def run_plan(L, plan, est=None):
    """One engine, one injected batch, the plan's steps front to back.  est: None or (how, seed, stride, Xi for 'thin').
    Returns (n, mean, cov), {chunk: (feat, tot, mean, n)}, (D, s) or None."""
    N, p = L.shape
    eng = HipEngine(0)
    try:
        eng.load_reduced(np.eye(p), np.ones(p) / p, 1.0, 1.0, H=np.eye(p), h=np.ones(p) / p)
        how, seed, stride, xi = est if est else (None, 0, 1, None)
        if how == "thin":
            eng.history_enable(N)
        elif how:
            eng.error_running_enable(seed)
        t = eng.debug_inject_lifts(L)
        i, n, c, slots = 0, 0, 0, {}
        for st in plan:
            if st[0] in ("acc1", "acc2"):
                eng.collect_batch(t, accumulate=1 if st[0] == "acc1" else 2, first=i, count=st[1])
                i += st[1]
                if st[0] == "acc2":
                    n = i
                    if how in ("check", "draws", "group", "group0"):
                        eng.error_advance(ID0 + stride * (i - st[1]), stride)
                    if how == "check":
                        eng.error_check_enqueue(n, c)
                        slots[c] = c
                    elif how == "draws":
                        eng.error_running_draws(n)
                        eng.error_quantiles_enqueue(c)
                        slots[c] = c
                    c += 1
            elif st[0] == "merge":
                eng.merge()
                n = i
            elif st[0] == "chunks":
                eng.collect_chunks(t, i, st[1], st[2], accumulate=2)
                i += st[1] * st[2]
                n = i
            elif st[0] == "group":
                counts = np.array(st[1])
                first = i + np.concatenate([[0], np.cumsum(counts)[:-1]])
                after = np.where(counts > 0, i + np.cumsum(counts), 0)
                ks = c + np.arange(len(counts))
                eng.group_collect(t, first, counts, ID0 + stride * first, stride, after, ks)
                slots.update({int(k): int(k) for k, cnt in zip(ks, counts) if cnt > 0})
                i += int(counts.sum())
                n, c = i, c + len(counts)
        assert i == N
        stats = eng.stats()
        checks = {k: eng.error_result(sl, wait=True) for k, sl in slots.items()}
        state = eng.error_state() if how and how != "thin" else None
        if how == "thin":
            eng.error_draws(xi, N)
            feat, tot = eng.error_quantiles()
            checks = {0: (feat, tot, stats[1], stats[0])}
        return stats, checks, state
    finally:
        eng.close()


def judge_stats(tag, L, ref, stats):
    """n exact; mean and covariance within the bound; the covariance bitwise symmetric, its diagonal >= -bound."""
    n, mean, cov = stats
    assert n == ref.n
    r_mean, r_cov = S.ratio(mean - ref.mean, ref.Em), S.ratio(cov - ref.cov, ref.Ecov)
    var = np.diag(ref.cov)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel_var = float(np.nanmax(np.where(var > 0, np.abs(np.diag(cov) - var) / var, 0.0)))
    print(f"SACC {tag}: n {n} err/bound mean {r_mean:.3g} cov {r_cov:.3g} | rel. variance error {rel_var:.3g} "
          f"min diag/bound {float(np.min(np.diag(cov) / np.maximum(np.diag(ref.Ecov), 1e-300))):.3g}")
    assert r_mean <= 1.0, f"{tag}: mean off by {r_mean:.3g} bounds"
    assert r_cov <= 1.0, f"{tag}: covariance off by {r_cov:.3g} bounds"
    np.testing.assert_array_equal(cov, cov.T)
    assert np.all(np.diag(cov) >= -np.diag(ref.Ecov)), f"{tag}: a variance below -bound"
    return r_mean, r_cov


def judge_family(tag, fam, name, p, L, plan, ref, stats, checks, rerun):
    """What a family asserts beyond the bound."""
    n, mean, cov = stats
    if fam == "liftlike":          # rows sum to a constant: the covariance's rows sum to ~0
        rows, want = np.asarray(cov, dtype=S.LD).sum(1), ref.cov.sum(1)
        assert S.ratio(rows - want, ref.Ecov.sum(1)) <= 1.0, f"{tag}: row sums of the covariance"
        assert np.all(np.abs(rows) <= ref.Ecov.sum(1) + np.abs(want))
    if fam == "degenerate":
        assert mean[0] == 0.0 and not cov[0].any() and not cov[:, 0].any(), f"{tag}: zero column"
        for k, (feat, *_rest) in checks.items():
            assert feat[0] == 0.0, f"{tag}: quantile of the zero column, check {k}"
        if p > 1:                   # constant column: round-off of c^2, not of sigma^2 -- the bound says how much
            assert abs(cov[1, 1]) <= ref.Ecov[1, 1] + abs(ref.cov[1, 1])
        if p > 3:                   # identical columns, different tiles: equal within the bounds
            assert abs(cov[2, 2] - cov[2, 3]) <= ref.Ecov[2, 2] + ref.Ecov[2, 3]
            assert abs(cov[3, 3] - cov[2, 3]) <= ref.Ecov[3, 3] + ref.Ecov[2, 3]
        if p > 5:
            assert abs(cov[4, 4] + cov[4, 5]) <= ref.Ecov[4, 4] + ref.Ecov[4, 5]
    if fam == "scaled":             # powers of two commute with every rounding: the unscaled run, scaled, bit for bit
        k = S.scaling_exponents(p, S.case_seed(name, fam))
        sc = np.exp2(k)
        np.testing.assert_array_equal(L / sc, S.family("gauss", len(L), p, S.case_seed(name, fam)))
        (n0, mean0, cov0), checks0, _ = rerun(L / sc)
        assert n0 == n
        np.testing.assert_array_equal(mean, mean0 * sc)
        np.testing.assert_array_equal(cov, cov0 * np.outer(sc, sc))
        for c in checks:
            np.testing.assert_array_equal(checks[c][0], checks0[c][0] * sc)


@pytest.mark.parametrize("name,p,plan,fam", STATS, ids=[f"{c[0]}-{c[3]}" for c in STATS])
def test_statistics_within_the_bound(name, p, plan, fam):
    for st in plan:                 # the sliced cases sit on the edges they were chosen for
        if st[0] in ("acc1", "acc2") and (st[1], p) in S.SLICE_EDGES:
            assert debug_stats_slices(st[1], p) == (S.SLICE_EDGES[(st[1], p)], False)
    groups = S.plan_groups(plan)
    L = S.family(fam, sum(groups), p, S.case_seed(name, fam))
    assert L.nbytes < 5e6
    ref = S.Reference(L, groups)
    stats, _, _ = run_plan(L, plan)
    tag = f"{name} {fam}"
    judge_stats(tag, L, ref, stats)
    judge_family(tag, fam, name, p, L, plan, ref, stats, {}, lambda M: run_plan(M, plan))


@pytest.mark.parametrize("name,p,how,counts,stride,fam", EST, ids=[f"{c[0]}-{c[5]}" for c in EST])
def test_estimator_within_the_bound(engine, name, p, how, counts, stride, fam):
    plan, chunks, cg = S.est_layout(how, counts)
    groups = S.plan_groups(plan)
    N = sum(groups)
    seed = S.case_seed(name, fam)
    L = S.est_family(fam, N, p, seed)
    # the normals as the device makes them are exact inputs (their own accuracy: test_running_error_estimator)
    Xi = np.random.default_rng(seed).standard_normal((S.ND, N)) if how == "thin" else engine.error_xi(seed, ID0, stride, N)
    ref = S.Reference(L, groups)
    est = S.EstReference(L, Xi, chunks, ref, cg)
    stats, checks, state = run_plan(L, plan, (how, seed, stride, Xi))
    tag = f"{name} {fam}"
    judge_stats(tag, L, ref, stats)
    assert sorted(checks) == sorted(est.checks)
    worst = [0.0, 0.0, 0.0]
    for c, (feat, tot, mean, n) in checks.items():
        t = est.checks[c]
        assert n == t["n"], f"{tag}: check {c} read n = {n}"
        r = (S.ratio(feat - t["feat"], t["Efeat"]), S.ratio(tot - t["tot"], t["Etot"]), S.ratio(mean - t["mean"], t["Em"]))
        worst = [max(a, b) for a, b in zip(worst, r)]
        assert r[0] <= 1.0, f"{tag}: feature quantiles of check {c} off by {r[0]:.3g} bounds"
        assert r[1] <= 1.0, f"{tag}: overall quantile of check {c} off by {r[1]:.3g} bounds"
        assert r[2] <= 1.0, f"{tag}: snapshot mean of check {c} off by {r[2]:.3g} bounds"
    rD = rs = 0.0
    if state is not None:
        rD, rs = S.ratio(state[0] - est.D, est.ED), S.ratio(state[1] - est.s, est.Es)
        assert rD <= 1.0 and rs <= 1.0, f"{tag}: D off by {rD:.3g}, s by {rs:.3g} bounds"
    print(f"SACC {tag}: err/bound feature quantiles {worst[0]:.3g} overall {worst[1]:.3g} snapshot means {worst[2]:.3g} "
          f"D {rD:.3g} s {rs:.3g}")
    judge_family(tag, fam, name, p, L, plan, ref, stats, checks, lambda M: run_plan(M, plan, (how, seed, stride, Xi)))


@pytest.mark.parametrize("p", [12, 130])
@pytest.mark.parametrize("n_small", [972, 973])
def test_quantile_interpolation_to_the_bit(p, n_small):
    """numpy's _lerp is evaluated from b's side when t >= 0.5 (quantile_body), and no err <= bound assertion can see which
    side a kernel takes: the two differ by one rounding.  Here every |draw| of a feature is one of two values more than a
    factor two apart (integer lift vectors with an exact mean, integer normals of a few values through the thin form:
    core = Xi L - rowsum mean is exact, a draw is one rounding that NumPy reproduces), 972 of the smaller: the quantile
    sits between them, and it must be one of the values the b-side form can give (hp_stats.lerp_candidates: with or
    without fused multiply-adds) -- in about one column in ten none of those is a value the a-side form gives
    (host test; one such column is enough).  973 of
    the smaller: equal neighbours, the quantile is that value in every form.  Ties throughout: 1024 values, two sizes.
    If the unchanged kernel fails here after a compiler update, suspect first that the compiler changed contraction: the
    accepted set is the b-side form with the multiply-add fused or not, as hipcc emits it today, and nothing else."""
    L, Xi = S.lerp_inputs(p, 5 + p, n_small)
    eng = HipEngine(0)
    try:
        eng.load_reduced(np.eye(p), np.ones(p) / p, 1.0, 1.0, H=np.eye(p), h=np.ones(p) / p)
        eng.history_enable(S.LERP_N)
        eng.collect_batch(eng.debug_inject_lifts(L), accumulate=2)
        n, mean, _ = eng.stats()
        eng.error_draws(Xi, S.LERP_N)
        import torch
        eng.synchronize()
        draws = torch.as_tensor(eng.draws_buffer(), device="cuda:0").cpu().numpy().reshape(S.ND, -1)[:, :p]
        feat, _ = eng.error_quantiles()
    finally:
        eng.close()
    assert n == S.LERP_N
    np.testing.assert_array_equal(mean, L.mean(0))
    x = (Xi @ L - np.outer(Xi.sum(1), mean)) * (1.0 / np.sqrt(S.LERP_N * (S.LERP_N - 1.0)))
    np.testing.assert_array_equal(draws, x)                  # the draws themselves, bit for bit
    v = np.sort(np.abs(x), axis=0)
    apart = 0
    for c in range(p):
        b_side, a_side = S.lerp_candidates(v[971, c], v[972, c])
        assert feat[c] in b_side, f"column {c}: {feat[c]!r} is not numpy's _lerp of {v[971, c]!r}, {v[972, c]!r}: {sorted(b_side)}"
        apart += not (b_side & a_side)
    assert apart >= 1 if n_small == 972 else apart == 0


def test_inject_refusals():
    """lsspa_debug_lift_inject refuses with LSSPA_ERR_STATE (3) and a text: no problem, two lanes, a player map, a batch
    in flight; after the batch is taken the lane is free again."""
    import ctypes
    from ls_spa import _native as N
    state = r"status 3\): .*"
    eng = HipEngine(0)
    try:
        z, t = np.zeros((2, 4)), ctypes.c_int32()
        assert eng._lib.lsspa_debug_lift_inject(eng._h, N.dptr(z), 2, ctypes.byref(t)) == 3
        assert b"no problem" in eng._lib.lsspa_last_error(eng._h)
        eng.load_reduced(np.eye(4), np.ones(4), 1.0, 1.0, H=np.eye(4), h=np.ones(4))
        t = eng.debug_inject_lifts(np.arange(12.0).reshape(3, 4))
        with pytest.raises(LSSPANativeError, match=state + "still to be collected"):
            eng.debug_inject_lifts(z)
        np.testing.assert_array_equal(eng.collect_batch(t, want_lifts=True, accumulate=2), np.arange(12.0).reshape(3, 4))
        eng.set_lanes(2)
        with pytest.raises(LSSPANativeError, match=state + "one-lane"):
            eng.debug_inject_lifts(z)
        eng.set_lanes(1)
        eng.set_players([0, 0, 1, 1])
        with pytest.raises(LSSPANativeError, match=state + "player map"):
            eng.debug_inject_lifts(z)
        eng.clear_players()
        eng.discard_batch(eng.debug_inject_lifts(z))
    finally:
        eng.close()
