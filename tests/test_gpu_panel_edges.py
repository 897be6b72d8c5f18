"""The per-ordering general path (gather -> chol_diag2 -> chol_panel2 with X tiles and fused lift scan -> strip2 -> lift)
against the long-double truth at every panel, live-row and dispatch edge, and its independence of batch composition and
of what the workspace held before.  The cases are tests/panel_cases.py; tests/test_panel_plan_host.py proves on the CPU,
with the library's own launch rule, that they reach every class.

    a. lifts of every case against hp_ref (long double from the fp64 inputs on), judged like tests/test_gpu_accuracy.py:
       tol = max(T0, MG * e_plain) with its T0 and MG, e_plain the error of NumPy / LAPACK at the same precision; in fp64
       also the 1e-11 absolute of test_lift_batch_vs_oracle; info() == 0; after full_fit() every sample's lifts sum to
       R^2 within the engine's own check; the profile shows the general kernels, launch for launch as the plan says
    b. the factors (lsspa_debug_factor) L, z = row p of L, L_t and V against the long-double factors, tolerances of
       test_cholesky_factor (fp32: the 1e-4 of the largest entry of test_vt_tiles_agree_with_the_strip_kernel), and the
       identity padding of the rows beyond p + 1, exactly
    c. the lift row of an ordering does not depend on the batch it is run in: bit-equal alone, in a grouped batch and in
       an ungrouped one (the tile map changes where a workgroup runs, not what it adds)
    d. ... nor on what the workspace held: bit-equal on a fresh engine and after other shapes, precisions and modes
       (the padding that the p_live skipping relies on is rewritten by the gather, not inherited)

Host time: the long-double truth of every case took 170 s on a slow host (measured; the long-double Gram matrices
alone 10 s a shape at p = 511, an ordering 1.2 s), 110 s without the p >= 495 shapes -- 19 s on the MI355X machine's CPU.  So the cases with p >= 495 (ORACLE_FROM_P) take the
fp64 QR oracle (tests/oracle_engine.py) as the truth of their lifts, and for their factors the long-double factorisation
of the fp64 Gram matrices (the Gram step is pinned by tests/test_gpu_gram_exact.py); every other case has the long-double
truth from the inputs on, computed once per shape (p, n, m) and shared by the precisions, flags and batch sizes of that
shape.  The p >= 495 cases are marked slow."""
import time

import numpy as np
import pytest

import hp_ref
import panel_cases as PC
from ls_spa._engine import HipEngine, debug_panel_plan
from oracle_engine import OracleEngine
from test_gpu_accuracy import judge, threshold          # judge brings its T0 and MG

pytestmark = pytest.mark.gpu

_TRUTH = {}
_FACTORS = {}
HOST_SECONDS = {"truth": 0.0}
WORST = {}          # (class, dtype) -> worst r; ("factor", dtype) -> worst |L - truth|


ORACLE_FROM_P = 495


class GramProblem(hp_ref.Problem):
    """hp_ref.Problem from the fp64 Gram matrices (p >= ORACLE_FROM_P, factors only): long double from there on."""

    def __init__(self, d):
        self.ar = hp_ref.LD
        G, g, H, h, yy = hp_ref.plain_gram(*d)
        self.G, self.g, self.H, self.h, self.yy = (hp_ref.LD.conv(a) for a in (G, g, H, h, np.float64(yy)))
        self.p, self.m, self.tri = len(g), len(d[3]), True
        self.min_pivot = self.min_pivot_test = float("inf")
        self._lift_cache = {}


def truth_of(p, n, m):
    """(data, long-double problem) of a shape, made once."""
    key = (p, n, m)
    if key not in _TRUTH:
        t = time.perf_counter()
        d = PC.data_of(p, n, m)
        _TRUTH[key] = (d, hp_ref.Problem(*d) if p < ORACLE_FROM_P else GramProblem(d))
        HOST_SECONDS["truth"] += time.perf_counter() - t
    return _TRUTH[key]


def truth_lifts(p, d, ref, orders, anti):
    t = time.perf_counter()
    if p < ORACLE_FROM_P:
        want = ref.lifts(orders, anti)
    else:
        key = ("oracle", p, len(d[3]))
        if key not in _TRUTH:
            _TRUTH[key] = OracleEngine()
            _TRUTH[key].load_data(*d, 0.0)
        o = _TRUTH[key]
        want = o.collect_batch(o.launch_batch(orders, anti), want_lifts=True, accumulate=False)
    HOST_SECONDS["truth"] += time.perf_counter() - t
    return want


@pytest.fixture(scope="module")
def eng():
    e = HipEngine(0)
    yield e
    e.close()


def _param(c):
    return pytest.param(c, id=c.name, marks=[pytest.mark.slow] if c.p >= 495 else [])


# ---- a. lifts against the long-double truth ----------------------------------------------------------------------------
@pytest.mark.parametrize("case", [_param(c) for c in PC.CASES])
def test_lifts_against_the_long_double_truth(eng, case):
    c = case
    tri = PC.is_tri(c)
    d, ref = truth_of(c.p, c.n, c.m)
    orders = PC.orderings_of(c.p, c.B)
    want = truth_lifts(c.p, d, ref, orders, c.anti)
    e_plain = float(np.abs(hp_ref.plain_lifts(*d, 0.0, orders, c.anti, np.dtype(c.dtype).type) - want).max())
    ratio = min(ref.min_pivot, ref.min_pivot_test) / threshold(c.p, c.dtype)
    plan = debug_panel_plan(c.p, PC.n_ord_of(c), tri, c.flags)

    eng.set_flags(c.flags)
    eng.set_precision(c.dtype)
    try:
        eng.load_data(*d, 0.0)
        assert eng.tri == tri
        eng.profile(True)
        eng.profile_reset()
        got = eng.run_batch(orders, c.anti, want_lifts=True, accumulate=False)
        used = eng.profile_read()
        eng.profile(False)
        info = eng.info()
        theta, r2, fit_info = eng.full_fit()          # from here on every batch's sums are checked
        again = eng.run_batch(orders, c.anti, want_lifts=True, accumulate=False)
        info_sum = eng.info()
    finally:
        eng.profile(False)
        eng.set_flags(0)
        eng.set_precision("float64")

    r = judge(f"PANEL {c.name}", got, want, e_plain, 0, ratio, c.dtype)
    err = float(np.abs(got - want).max())
    print(f"PANEL {c.name} class {c.cls}: err {err:.3e} e_plain {e_plain:.3e} r {r:.2f} "
          f"sum dev {np.abs(again.sum(axis=1) - r2).max():.3e}")
    key = (c.cls, "tri" if tri else "rect", c.dtype)
    WORST[key] = max(WORST.get(key, 0.0), r)
    assert info == 0 and fit_info == 0, (info, fit_info)
    if c.dtype == PC.F64:
        assert err <= 1e-11, f"{c.name}: |got - truth| = {err:.3e}"
    # the general kernels ran, launch for launch as planned, and the fused small-p kernel did not
    n_run = used["gather"][1]
    vt = tri and not c.flags & 128
    assert n_run >= 1 and used["small_p"][1] == 0, used
    assert used["chol_diag"][1] == n_run and used["lift"][1] == n_run, used
    assert used["chol_panel"][1] == n_run * len(plan["launches"]), (used, plan)
    assert used["strip"][1] == (0 if vt else n_run), used
    # the sums: the engine's own check did not fire, and they are within its tolerance of R^2
    assert info_sum & 12 == 0 and info_sum == 0, info_sum
    np.testing.assert_array_equal(again, got)
    tol = (1e-9 if c.dtype == PC.F64 else 1e-4) * max(1.0, abs(r2))
    assert np.abs(again.sum(axis=1) - r2).max() <= tol


# ---- b. factors against the truth --------------------------------------------------------------------------------------
def factor_truth(p, which):
    """Long-double L, z, L_t, yt, V = L^-1 L_t of the identity (which = 0) or a seeded ordering of the tri shape of p."""
    key = (p, which)
    if key not in _FACTORS:
        d, ref = truth_of(p, PC.n_of(p), PC.tri_m(p))
        t = time.perf_counter()
        o = np.arange(p) if which == 0 else np.random.default_rng(1000 + p).permutation(p)
        L, z, _ = ref._chol_aug(ref.G[np.ix_(o, o)], ref.g[o])
        Lt, yt, _ = ref._chol_aug(ref.H[np.ix_(o, o)], ref.h[o])
        V = ref._forward(L, Lt)
        _FACTORS[key] = (o.astype(np.int32),) + tuple(np.asarray(a, dtype=np.float64) for a in (L, z, Lt, yt, V))
        HOST_SECONDS["truth"] += time.perf_counter() - t
    return _FACTORS[key]


@pytest.mark.parametrize("dtype", [PC.F64, PC.F32])
@pytest.mark.parametrize("p", [pytest.param(p, marks=[pytest.mark.slow] if p >= 495 else []) for p in PC.FACTOR_P])
def test_factors_against_the_long_double_truth(eng, p, dtype):
    """fp64: the tolerances of test_cholesky_factor.  fp32: 1e-4 of the largest entry of the matrix compared, the bound
    test_vt_tiles_agree_with_the_strip_kernel holds V to (the Gram matrices are rounded to fp32 first: 6e-8 relative,
    times the condition of the factorisation, some 1e3 for H with m = p + 50 test rows).  Padding: the rows beyond the
    carried row are the identity's, bit for bit, in both factors -- the gather writes them, the factorisation keeps
    them, and the p_live skipping relies on it."""
    d, _ = truth_of(p, PC.n_of(p), PC.tri_m(p))
    f64 = dtype == PC.F64
    eng.set_precision(dtype)
    worst = 0.0
    try:
        eng.load_data(*d, 0.0)
        for which in (0, 1):
            o, Lw, zw, Ltw, ytw, Vw = factor_truth(p, which)
            for flags in (1024, 1024 | 128):
                eng.set_flags(flags)
                L, Lt, V = eng.debug_factor(o)
                assert eng.info() == 0
                name = f"PANEL factor p={p} {dtype} flags={flags} perm={which}"
                errs = [float(np.abs(a - b).max()) for a, b in ((np.tril(L[:p, :p]), Lw), (L[p, :p], zw),
                                                                (np.tril(Lt[:p, :p]), Ltw), (Lt[p, :p], ytw),
                                                                (V[:p, :p], Vw))]
                print(f"{name}: |L - truth| {errs[0]:.3e} z {errs[1]:.3e} L_t {errs[2]:.3e} yt {errs[3]:.3e} "
                      f"V {errs[4]:.3e}")
                worst = max(worst, errs[0], errs[2])
                if f64:
                    np.testing.assert_allclose(np.tril(L[:p, :p]), Lw, rtol=1e-11, atol=1e-12, err_msg=name)
                    np.testing.assert_allclose(L[p, :p], zw, rtol=1e-10, atol=1e-12, err_msg=name)
                    np.testing.assert_allclose(np.tril(Lt[:p, :p]), Ltw, rtol=1e-11, atol=1e-11, err_msg=name)
                    np.testing.assert_allclose(Lt[p, :p], ytw, rtol=1e-10, atol=1e-11, err_msg=name)
                    np.testing.assert_allclose(V[:p, :p], Vw, rtol=1e-10, atol=1e-10, err_msg=name)
                else:
                    for a, b in ((np.tril(L[:p, :p]), Lw), (L[p, :p], zw), (np.tril(Lt[:p, :p]), Ltw),
                                 (Lt[p, :p], ytw), (V[:p, :p], Vw)):
                        np.testing.assert_allclose(a, b, rtol=0, atol=1e-4 * np.abs(b).max(), err_msg=name)
                # padding: rows beyond the carried row p
                p_pad = L.shape[0]
                assert p_pad == (p + 1 + 127) // 128 * 128 and Lt.shape == L.shape
                for F in (L, Lt):
                    pad = F[p + 1:, :]
                    np.testing.assert_array_equal(np.tril(pad, k=p + 1), np.eye(p_pad)[p + 1:, :], err_msg=name)
    finally:
        eng.set_flags(0)
        eng.set_precision("float64")
    key = ("factor", dtype)
    WORST[key] = max(WORST.get(key, 0.0), worst)


# ---- c. composition does not change a bit --------------------------------------------------------------------------------
def _lifts(e, orders):
    return e.run_batch(np.ascontiguousarray(orders), False, want_lifts=True, accumulate=False)


@pytest.mark.parametrize("dtype", [PC.F64, PC.F32])
@pytest.mark.parametrize("p", PC.COMPOSITION_P)
@pytest.mark.parametrize("mode", ["tri", "rect"])
def test_composition_does_not_change_a_bit(eng, mode, p, dtype):
    """Non-antithetical batches.  tri: every ordering alone (2 matrices) against its row in batches of 4 (8 matrices:
    the grouped map wherever a launch has more than one L tile), 12 (24, grouped) and 5 (10, ungrouped).  rect: alone
    against batches of 8 (grouped) and 9.  And a call repeated gives the same bits.  No summation in these kernels is
    shared between matrices or ordered by workgroup id, so nothing but equality is right."""
    tri = mode == "tri"
    m = PC.tri_m(p) if tri else PC.RECT_M
    d = PC.data_of(p, PC.n_of(p), m)
    sizes = (4, 12, 5) if tri else (8, 9)
    orders = PC.orderings_of(p, max(sizes))
    for B in sizes:      # what this test is about has to be what the library does
        grouped = any(ln["grouped"] for ln in debug_panel_plan(p, B, tri)["launches"])
        assert grouped == (B in (4, 12, 8)), (B, grouped)
    assert not any(ln["grouped"] for ln in debug_panel_plan(p, 1, tri)["launches"])
    eng.set_precision(dtype)
    try:
        eng.load_data(*d, 0.0)
        assert eng.tri == tri
        alone = np.concatenate([_lifts(eng, orders[k:k + 1]) for k in range(len(orders))])
        assert np.all(np.isfinite(alone))
        for B in sizes:
            got = _lifts(eng, orders[:B])
            np.testing.assert_array_equal(got, alone[:B], err_msg=f"batch of {B} against the orderings alone")
            np.testing.assert_array_equal(_lifts(eng, orders[:B]), got, err_msg=f"batch of {B} repeated")
        # a batch that starts elsewhere in the sequence: every ordering sits in another slot
        got = _lifts(eng, orders[3:3 + sizes[0]])
        np.testing.assert_array_equal(got, alone[3:3 + sizes[0]])
        assert eng.info() == 0
    finally:
        eng.set_precision("float64")


# ---- d. workspace history does not change a bit ------------------------------------------------------------------------
def _fresh(p, m, dtype, B=4, anti=True):
    e = HipEngine(0)
    try:
        return _visit(e, p, m, dtype, B, anti)
    finally:
        e.close()


def _visit(e, p, m, dtype, B=4, anti=True):
    e.set_precision(dtype)
    e.load_data(*PC.data_of(p, PC.n_of(p), m), 0.0)
    out = e.run_batch(PC.orderings_of(p, B), anti, want_lifts=True, accumulate=False)
    assert e.info() == 0 and np.all(np.isfinite(out))
    return out


def test_workspace_history_does_not_change_a_bit():
    """One engine: p = 511 fp64, then p = 257 fp64, fp32 and fp64 again -- each p = 257 result has the bits a fresh engine
    gives.  The work matrices of p = 257 (p_pad = 384, p_live = 272) lie in memory the p = 511 ones (p_pad = 512) filled;
    the gather rewrites every row up to its 64-column block edge and the kernels read nothing beyond."""
    want64, want32 = _fresh(257, PC.tri_m(257), PC.F64), _fresh(257, PC.tri_m(257), PC.F32)
    assert not np.array_equal(want64, want32)
    e = HipEngine(0)
    try:
        _visit(e, 511, PC.tri_m(511), PC.F64)
        np.testing.assert_array_equal(_visit(e, 257, PC.tri_m(257), PC.F64), want64)
        np.testing.assert_array_equal(_visit(e, 257, PC.tri_m(257), PC.F32), want32)
        np.testing.assert_array_equal(_visit(e, 257, PC.tri_m(257), PC.F64), want64)
    finally:
        e.close()


@pytest.mark.parametrize("dtype", [PC.F64, PC.F32])
def test_workspace_history_across_modes(dtype):
    """rect after tri (the strip kernel's V in the memory that held V^T), and tri after rect at a smaller p_pad."""
    rect_want = _fresh(300, PC.RECT_M, dtype)
    tri_want = _fresh(257, PC.tri_m(257), dtype)
    e = HipEngine(0)
    try:
        _visit(e, 385, PC.tri_m(385), dtype)
        np.testing.assert_array_equal(_visit(e, 300, PC.RECT_M, dtype), rect_want)
        _visit(e, 385, PC.RECT_M, dtype, B=8, anti=False)
        np.testing.assert_array_equal(_visit(e, 257, PC.tri_m(257), dtype), tri_want)
    finally:
        e.close()


def test_report():
    """Not a check: the worst r per class and the host time of the truth, for DESIGN.md (Numerics)."""
    for key in sorted(WORST):
        print("PANEL worst", *key, f"{WORST[key]:.3e}")
    print(f"PANEL host seconds of the long-double truth: {HOST_SECONDS['truth']:.1f}")
