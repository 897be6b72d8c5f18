"""tests/hp_stats.py has to earn its trust before tests/test_gpu_stats_accuracy.py leans on it, on the CPU: its long-double
truth against mpmath, a plain fp64 restatement of the engine's route inside the rounding-count bound on every case the GPU
tests run (the bound is not too tight), and every such case moved by more than 100 bounds by each of three mutations of
that restatement (the case is not blind)."""
import numpy as np
import pytest

import hp_stats as S
import philox_ref

STATS = [(name, p, plan, fam) for name, p, plan, fams in S.STATS_CASES for fam in fams]
EST = [(name, p, how, counts, stride, fam) for name, p, how, counts, stride, fams in S.EST_CASES for fam in fams]


def test_truth_against_mpmath():
    """p = 3, n = 11, three chunks: mean, covariance, draws and both quantiles of the long-double truth against 50 digits."""
    import mpmath
    mpmath.mp.dps = 50
    rng = np.random.default_rng(11)
    L = rng.standard_normal((11, 3))
    Xi = rng.standard_normal((S.ND, 11))
    ref = S.Reference(L, [4, 1, 6])
    est = S.EstReference(L, Xi, [4, 1, 6], ref, [None, None, 2])
    mp = lambda a: [[mpmath.mpf(float(v)) for v in row] for row in np.atleast_2d(a)]      # noqa: E731
    Lm, Xm = mp(L), mp(Xi)
    mean = [sum(Lm[s][a] for s in range(11)) / 11 for a in range(3)]
    cov = [[sum((Lm[s][a] - mean[a]) * (Lm[s][b] - mean[b]) for s in range(11)) / 11 for b in range(3)] for a in range(3)]
    scale = 1 / mpmath.sqrt(mpmath.mpf(110))
    x = [[sum(Xm[d][s] * (Lm[s][a] - mean[a]) for s in range(11)) * scale for a in range(3)] for d in range(S.ND)]

    def q95(v):
        v = sorted(v)
        pos = mpmath.mpf(0.95 * (len(v) - 1))        # numpy's (and the kernel's) fp64 position
        lo = int(mpmath.floor(pos))
        return v[lo] + (v[lo + 1] - v[lo]) * (pos - lo)

    def close(got, want, scale_of):
        # long double carries 64 bits; the data are of size 1 and n = 11: 16 x 2^-60 leaves a few dozen roundings' room
        assert abs(mpmath.mpf(float(got)) + mpmath.mpf(float(got - np.longdouble(float(got)))) - want) <= scale_of * 2.0 ** -60

    for a in range(3):
        close(ref.mean[a], mean[a], 16.0)
        close(est.checks[2]["feat"][a], q95([abs(x[d][a]) for d in range(S.ND)]), 16.0)
        for b in range(3):
            close(ref.cov[a][b], cov[a][b], 16.0)
            close(ref.chan_cov[a][b], cov[a][b], 16.0)
    close(est.checks[2]["tot"], q95([mpmath.sqrt(sum(v * v for v in row)) for row in x]), 16.0)
    for d in (0, 517, 1023):
        for a in range(3):
            close(est.checks[2]["x"][d, a], x[d][a], 16.0)
    x64 = np.asarray(est.checks[2]["x"], dtype=np.float64)
    np.testing.assert_allclose(S.quantile95(np.abs(x64)), np.quantile(np.abs(x64), 0.95, axis=0), rtol=4e-16, atol=0)


def test_slice_edges_follow_the_librarys_own_rule():
    """The sliced cases sit on the edges they were chosen for (a last slice of one sample, trailing empty slices) under
    the rule the library itself applies (lsspa_debug_stats_slices: stats_batch_slices and the samples per slice)."""
    from ls_spa._engine import debug_stats_slices as slices
    for (n, p), want in S.SLICE_EDGES.items():
        assert slices(n, p) == (want, False), (n, p, slices(n, p))
    used = {(st[1], p) for _, p, plan, _ in S.STATS_CASES for st in plan if st[0] in ("acc1", "acc2")}
    assert set(S.SLICE_EDGES) <= used
    # one slice: the small forms' range and, beyond p = 128, up to 64 samples (17 and 1 in the batch_p* cases); their
    # 100-sample chunks are two slices already (64 + 36), not one
    assert slices(512, 128) == ([512], True) and slices(513, 128) == ([64] * 8 + [1], False)
    assert slices(64, 129) == ([64], False) and slices(17, 257) == ([17], False)
    assert slices(100, 129) == ([64, 36], False) and slices(100, 257) == ([64, 36], False)
    for name, p, plan, _ in S.STATS_CASES:          # every case takes the form its name says
        small = {slices(st[1], p)[1] for st in plan if st[0] in ("acc1", "acc2", "chunks")}
        assert small == {name.startswith(("small_", "multi_"))}, (name, small)


def test_lerp_case_tells_the_two_forms_apart():
    """The bitwise quantile case (test_gpu_stats_accuracy.py) is not blind: in some columns (about one in ten) no value the a-side form of
    the interpolation can give is one the b-side form can give; between equal neighbours all forms give the neighbour."""
    for p in (12, 130):
        L, Xi = S.lerp_inputs(p, 5 + p)
        mean = L.mean(0)
        np.testing.assert_array_equal(mean * S.LERP_N, L.sum(0))
        x = np.abs((Xi @ L - np.outer(Xi.sum(1), mean)) * (1.0 / np.sqrt(S.LERP_N * (S.LERP_N - 1.0))))
        x.sort(axis=0)
        assert np.all(x[971] == x[0]) and np.all(x[972] == x[-1]) and np.all(x[972] > 2 * x[971])
        apart = sum(not (b & a) for b, a in (S.lerp_candidates(x[971, c], x[972, c]) for c in range(p)))
        print(f"HOST lerp p={p}: the two forms are apart in {apart} of {p} columns")
        assert apart >= 1           # one such column is enough for the a-side form to fail the GPU test
    b, a = S.lerp_candidates(0.3, 0.3)
    assert b == a == {0.3}


def test_every_form_of_the_issue_has_a_case():
    names = " ".join(n for n, *_ in S.STATS_CASES + S.EST_CASES)
    for form in ("small_merge", "small_fused", "multi", "batch", "sliced", "merge2", "est_check", "est_draws", "est_group",
                 "est_thin"):
        assert form in names
    counts = {st[1] for n, _, plan, _ in S.STATS_CASES if n.startswith("small_") for st in plan if st[0] != "merge"}
    assert {1, 3, 15, 16, 17, 63, 64, 65, 511, 512} <= counts


@pytest.mark.parametrize("name,p,plan,fam", STATS, ids=[f"{c[0]}-{c[3]}" for c in STATS])
def test_plain_route_is_inside_the_bound_and_mutations_are_outside(name, p, plan, fam):
    groups = S.plan_groups(plan)
    L = S.family(fam, sum(groups), p, S.case_seed(name, fam))
    ref = S.Reference(L, groups)
    assert S.ratio(ref.chan_cov - ref.cov, ref.Ecov) <= 1e-3        # the Chan route in exact arithmetic IS the covariance
    n, mean, cov, snaps = S.plain_stats(L, groups)
    assert n == ref.n
    r_mean, r_cov = S.ratio(mean - ref.mean, ref.Em), S.ratio(cov - ref.cov, ref.Ecov)
    r_snap = max(S.ratio(m - t[1], t[2]) for (_, m), t in zip(snaps, ref.snaps))
    print(f"HOST {name} {fam}: plain err/bound mean {r_mean:.3g} cov {r_cov:.3g} snapshots {r_snap:.3g}")
    assert max(r_mean, r_cov, r_snap) <= 1.0
    for mut in S.MUTATIONS:
        _, m2, c2, _ = S.plain_stats(L, groups, mutate=mut)
        moved = max(S.ratio(m2 - ref.mean, ref.Em), S.ratio(c2 - ref.cov, ref.Ecov))
        print(f"HOST {name} {fam}: mutation {mut} moves a quantity by {moved:.3g} bounds")
        assert moved > 100.0, f"{name} {fam} is blind to '{mut}'"


@pytest.mark.parametrize("name,p,how,counts,stride,fam", EST, ids=[f"{c[0]}-{c[5]}" for c in EST])
def test_plain_estimator_is_inside_the_bound(name, p, how, counts, stride, fam):
    plan, chunks, cg = S.est_layout(how, counts)
    groups = S.plan_groups(plan)
    N = sum(groups)
    seed = S.case_seed(name, fam)
    L = S.est_family(fam, N, p, seed)
    Xi = philox_ref.normals(seed, 3 + stride * np.arange(N))
    ref = S.Reference(L, groups)
    est = S.EstReference(L, Xi, chunks, ref, cg)
    n, mean, cov, snaps = S.plain_stats(L, groups)
    assert max(S.ratio(mean - ref.mean, ref.Em), S.ratio(cov - ref.cov, ref.Ecov)) <= 1.0
    D, s, checks = S.plain_estimator(L, Xi, chunks, snaps, cg)
    rD, rs = S.ratio(D - est.D, est.ED), S.ratio(s - est.s, est.Es)
    worst = 0.0
    for c, (feat, tot) in checks.items():
        t = est.checks[c]
        worst = max(worst, S.ratio(feat - t["feat"], t["Efeat"]), S.ratio(tot - t["tot"], t["Etot"]))
    print(f"HOST {name} {fam}: plain err/bound D {rD:.3g} s {rs:.3g} quantiles {worst:.3g}")
    assert len(checks) == sum(g is not None for g in cg) > 0
    assert max(rD, rs, worst) <= 1.0
    if fam.startswith("ties"):
        # sensitivity of the statistics does not apply (one or two non-zero samples): these cases are about the draws of a
        # nearly empty history, the sort and the quantile
        return
    for mut in S.MUTATIONS:
        _, m2, c2, _ = S.plain_stats(L, groups, mutate=mut)
        assert max(S.ratio(m2 - ref.mean, ref.Em), S.ratio(c2 - ref.cov, ref.Ecov)) > 100.0, f"{name} {fam} blind to {mut}"
