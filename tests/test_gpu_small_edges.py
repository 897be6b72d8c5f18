"""The one-response fused per-ordering kernels (csrc/k_small.hip: small_reg_kernel<NB>, NB = 1 .. 7, a matrix in one wave's
registers; small_p_kernel, both matrices in LDS, at nb = 8 or under developer flag 16384) against the long-double truth
at every block count and edge of the augmented row, and what they promise bit for bit.  The cases are
tests/small_cases.py; tests/test_small_cases_host.py proves on the CPU that they reach every class and that no truth case
may be flagged NOT_PD.

    a. lifts of every shape x kappa x form, single orderings and antithetical pairs, against hp_ref (long double from
       the fp64 inputs on), judged like tests/test_gpu_accuracy.py: tol = max(T0, MG * e_plain) with its T0 and MG; at
       kappa = 1 also the 1e-11 absolute of test_lift_batch_vs_oracle; info() == 0; the profile shows the fused kernel
       and no gather; after full_fit() the same batch has the same bits, the sum check stays quiet and every row sums to
       R^2 within the 1e-9 max(1, |R^2|) of tests/test_gpu_panel_edges.py
    b. the sum check itself: sum_deviation() is max_k |sum(lifts[k]) - R^2| of the lifts the call returns, within the
       bound of two sums of p terms taken in different orders, 2 p u sum|lift| (u = 2^-53); at kappa = 1e4 the deviation
       is orders of magnitude above that bound, so a check that did not run (deviation 0) fails it
    c. bits: an ordering's row does not depend on its batch, its slot, the call or the lane; an antithetical pair is
       0.5 a + 0.5 b of its two orderings run singly; flag 16384 selects another kernel up to p = 111 and the same from 112
    d. NOT_PD wherever the pivot fails -- every block row, the last position, either matrix alone -- and not for a near
       copy whose true pivot is between 1e3 and 1e4 x the threshold; what a failed ordering leaves behind is not read
    e. workspace history: p = 127 (the LDS form's 144 KB), then p = 17 and 47 under both forms, then p = 127 again, each
       with the bits of a fresh engine

What was measured on the MI355X -- the table test_report prints, the near copy's r, the time -- is in DESIGN.md, Numerics."""
import time

import numpy as np
import pytest

import hp_ref
import small_cases as SC
from ls_spa._engine import HipEngine
from test_gpu_accuracy import judge, shape, threshold          # judge brings its T0 and MG

pytestmark = pytest.mark.gpu

T_START = time.perf_counter()
_TRUTH = {}
_FRESH = {}
WORST = {}          # (form, nb) -> (worst r, error, case)
SUMS = {"dev": 0.0}
U = 2.0 ** -53


@pytest.fixture(scope="module")
def eng():
    e = HipEngine(0)
    yield e
    e.close()


def truth_of(p, kappa, reg):
    """Data, orderings, the long-double lifts and e_plain of both batch kinds, and the true pivot ratio: made once per
    (p, kappa, reg) and shared by the forms."""
    key = (p, kappa, reg)
    if key not in _TRUTH:
        d, orders = SC.data_of(p, kappa), SC.orderings_of(p, kappa)
        ref = hp_ref.Problem(*d, reg)
        want = {anti: ref.lifts(orders, anti) for anti in (False, True)}
        e_plain = {anti: float(np.abs(hp_ref.plain_lifts(*d, reg, orders, anti) - want[anti]).max())
                   for anti in (False, True)}
        ratio = min(ref.min_pivot, ref.min_pivot_test) / threshold(p)
        _TRUTH[key] = (d, orders, want, e_plain, ratio)
    return _TRUTH[key]


def _run(e, orders, anti=False):
    return e.run_batch(np.ascontiguousarray(orders), anti, want_lifts=True, accumulate=False)


def _note(c, r, err):
    key = (c.form, c.nb)
    if not r <= WORST.get(key, (-1.0,))[0]:
        WORST[key] = (r, err, c.name)


# ---- a. lifts against the long-double truth ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [pytest.param(c, id=c.name) for c in SC.CASES])
def test_lifts_against_the_long_double_truth(eng, case):
    c = case
    assert (c.n, c.m) == shape(c.p)
    d, orders, want, e_plain, ratio = truth_of(c.p, c.kappa, c.reg)
    got, again, info, info_sum = {}, {}, {}, {}
    eng.set_flags(c.flags)
    try:
        eng.load_data(*d, c.reg)
        assert eng.tri
        eng.profile(True)
        eng.profile_reset()
        for anti in (False, True):
            got[anti] = _run(eng, orders, anti)
            info[anti] = eng.info()
        used = eng.profile_read()
        eng.profile(False)
        theta, r2, fit_info = eng.full_fit()          # from here on every batch's sums are checked
        for anti in (False, True):
            again[anti] = _run(eng, orders, anti)
            info_sum[anti] = eng.info()
        dev = eng.sum_deviation()
    finally:
        eng.profile(False)
        eng.set_flags(0)

    for anti in (False, True):
        name = f"SMALL {c.name} {c.form} nb={c.nb} anti={int(anti)}"
        r = judge(name, got[anti], want[anti], e_plain[anti], info[anti] & 1, ratio)
        err = float(np.abs(got[anti] - want[anti]).max())
        _note(c, r, err)
        assert info[anti] == 0 and fit_info == 0, (name, info[anti], fit_info)
        if c.kappa == 1.0:
            assert err <= 1e-11, f"{name}: |got - truth| = {err:.3e}"
        # the sums: the engine's own check did not fire, and they are within its tolerance of R^2
        assert info_sum[anti] & 12 == 0 and info_sum[anti] == 0, (name, info_sum[anti])
        np.testing.assert_array_equal(again[anti], got[anti], err_msg=name)
        sum_dev = float(np.abs(again[anti].sum(axis=1) - r2).max())
        print(f"{name}: sum dev {sum_dev:.3e} (engine {dev:.3e})")
        SUMS["dev"] = max(SUMS["dev"], sum_dev)
        assert sum_dev <= 1e-9 * max(1.0, abs(r2)), name
    # the fused kernel ran and the general path did not
    assert used["small_p"][1] >= 1 and used["gather"][1] == 0 and used["chol_panel"][1] == 0, used


# ---- b. the sum check --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, SC.FLAG_LDS])
@pytest.mark.parametrize("p", SC.BITS_P)
@pytest.mark.parametrize("kappa", SC.KAPPAS)
def test_sum_deviation_is_that_of_the_returned_lifts(eng, p, flags, kappa):
    """Register form: the wave that holds the p lifts sums them (two a lane, then a butterfly) and keeps the largest
    |sum - R^2| of the batch; LDS form and p >= 112: sum_check_kernel of csrc/k_lift.hip does, from memory.  NumPy adds
    the same p numbers in another order: each sum is within (p - 1) u sum|lift| of the exact one, the subtraction of R^2
    is exact (the sum is within a factor of two of it), so the two deviations differ by at most 2 p u sum|lift|.
    At kappa = 1 the deviation itself is of the size of that bound, and a check that never ran (deviation 0: the
    tolerance not armed, sum_check_kernel not launched, the atomicMax lost) would pass; at kappa = 1e4 the Gram route's
    own error puts every row's sum some 1e-11 from R^2, far above the bound, and it cannot."""
    d = SC.data_of(p, kappa)
    orders = SC.bit_orderings(p, 24)
    eng.set_flags(flags)
    try:
        eng.load_data(*d, 0.0)
        theta, r2, fit_info = eng.full_fit()
        assert fit_info == 0
        eng.reset_stats()                         # the deviation is the largest since the last reset
        assert eng.sum_deviation() == 0.0
        lifts = _run(eng, orders, False)
        dev, info = eng.sum_deviation(), eng.info()
    finally:
        eng.set_flags(0)
    mine = np.abs(lifts.sum(axis=1) - r2)
    bound = float((2 * p * U * np.abs(lifts).sum(axis=1)).max())
    print(f"SMALL sum check p={p} kappa={kappa:g} flags={flags}: engine {dev:.3e} numpy {mine.max():.3e} "
          f"bound {bound:.3e}")
    assert info == 0
    assert abs(dev - mine.max()) <= bound
    if kappa > 1.0:       # the case has to tell a check that ran from one that did not
        assert mine.max() > 2 * bound and dev > 0.0, (mine.max(), bound, dev)


# ---- c. bits -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, SC.FLAG_LDS])
@pytest.mark.parametrize("p", SC.BITS_P)
def test_an_orderings_row_does_not_depend_on_batch_slot_or_call(eng, p, flags):
    """A workgroup owns its ordering from the gather to the lifts and writes nothing another reads; the only shared
    destination is a pair's row, zeroed first, to which two halves are added -- and a + b = b + a."""
    d = SC.data_of(p, 1.0)
    seq = SC.bit_orderings(p, 29)
    eng.set_flags(flags)
    try:
        eng.load_data(*d, 0.0)
        alone = np.concatenate([_run(eng, seq[k:k + 1]) for k in range(len(seq))])
        assert np.all(np.isfinite(alone))
        batch = _run(eng, seq[:24])
        np.testing.assert_array_equal(batch, alone[:24], err_msg="batch of 24 against the orderings alone")
        np.testing.assert_array_equal(_run(eng, seq[:24]), batch, err_msg="the call repeated")
        np.testing.assert_array_equal(_run(eng, seq[5:29]), alone[5:29], err_msg="a batch that starts at another offset")
        np.testing.assert_array_equal(_run(eng, seq[:1]), alone[:1], err_msg="a grid of one, repeated")
        # pairs: the reversed ordering is the forward row read backwards by the kernel; run singly it is a row of its own
        back = _run(eng, seq[:24, ::-1])
        pair = _run(eng, seq[:24], True)
        np.testing.assert_array_equal(pair, 0.5 * batch + 0.5 * back, err_msg="pair against 0.5 a + 0.5 b")
        np.testing.assert_array_equal(_run(eng, seq[5:6], True), pair[5:6], err_msg="a pair alone")
        assert eng.info() == 0
    finally:
        eng.set_flags(0)


def test_the_flag_selects_another_kernel_up_to_p_111_and_the_same_from_112(eng):
    differs = []
    for p in SC.BITS_P:
        d = SC.data_of(p, 1.0)
        orders = SC.bit_orderings(p, 24)
        out = {}
        try:
            for flags in (0, SC.FLAG_LDS):
                eng.set_flags(flags)
                eng.load_data(*d, 0.0)
                out[flags] = _run(eng, orders, True)
                assert eng.info() == 0
        finally:
            eng.set_flags(0)
        if p <= SC.REG_MAX_P:
            np.testing.assert_allclose(out[0], out[SC.FLAG_LDS], rtol=0, atol=1e-12)      # test_fused_small_p_kernel's
            differs.append(not np.array_equal(out[0], out[SC.FLAG_LDS]))
        else:
            np.testing.assert_array_equal(out[0], out[SC.FLAG_LDS], err_msg=f"p = {p}: one kernel under both flags")
    print("SMALL forms differ in bits at p <= 111:", differs)
    assert any(differs)


@pytest.mark.parametrize("flags", [0, SC.FLAG_LDS])
@pytest.mark.parametrize("p", SC.BITS_P)
def test_two_batches_in_flight_on_two_lanes(eng, p, flags):
    d = SC.data_of(p, 1.0)
    seq = SC.bit_orderings(p, 24)
    eng.set_flags(flags)
    try:
        eng.load_data(*d, 0.0)
        want = {anti: _run(eng, seq, anti) for anti in (False, True)}
        eng.set_lanes(2)
        for anti in (False, True):
            t1 = eng.launch_batch(seq[:12], anti)
            t2 = eng.launch_batch(seq[12:], anti)
            a = eng.collect_batch(t1, want_lifts=True, accumulate=False)
            b = eng.collect_batch(t2, want_lifts=True, accumulate=False)
            np.testing.assert_array_equal(np.concatenate([a, b]), want[anti], err_msg=f"anti = {anti}")
        assert eng.info() == 0
    finally:
        eng.set_lanes(1)
        eng.set_flags(0)


# ---- d. NOT_PD where the pivot fails ---------------------------------------------------------------------------------------
def fresh_lifts(p, flags, kappa=1.0, B=8, anti=True):
    """What a new engine gives for the well-conditioned data of p: made once per key."""
    key = (p, flags, kappa, B, anti)
    if key not in _FRESH:
        e = HipEngine(0)
        try:
            _FRESH[key] = _visit(e, p, flags, kappa, B, anti)
        finally:
            e.close()
    return _FRESH[key]


def _visit(e, p, flags, kappa=1.0, B=8, anti=True):
    e.set_flags(flags)
    try:
        e.load_data(*SC.data_of(p, kappa), 0.0)
        out = _run(e, SC.bit_orderings(p, B), anti)
        assert e.info() == 0 and np.all(np.isfinite(out))
    finally:
        e.set_flags(0)
    return out


@pytest.mark.parametrize("where", SC.DUP_WHERE)
@pytest.mark.parametrize("p, flags", SC.NOT_PD_RUNS, ids=[f"p{p}_f{f}" for p, f in SC.NOT_PD_RUNS])
def test_duplicate_column_is_flagged_at_every_position(eng, p, flags, where):
    """Column dup an exact copy of column 3, the first copy at position 0, the second at b: the pivot at b is zero up to
    round-off in G, in H or in both.  As a pair the reverse has the copies at p - 1 - b and p - 1.  Afterwards the same
    engine gives, for well-conditioned data, the bits of a fresh engine: the NaNs a failed ordering leaves in LDS and in
    the lift buffer are rewritten before anything reads them."""
    want = fresh_lifts(p, flags)
    d = SC.dup_data(p, where)
    eng.set_flags(flags)
    try:
        eng.load_data(*d, 0.0)
        for b, o in zip(SC.dup_positions(p), SC.dup_orderings(p)):
            for anti in (False, True):
                eng.reset_stats()                 # the info word is sticky
                assert eng.info() == 0
                with np.errstate(all="ignore"):
                    _run(eng, o[None, :], anti)
                assert eng.info() & 1, f"copy at position {b}, anti = {anti}: not flagged"
    finally:
        eng.set_flags(0)
    np.testing.assert_array_equal(_visit(eng, p, flags), want)


@pytest.mark.parametrize("p, flags", SC.NOT_PD_RUNS, ids=[f"p{p}_f{f}" for p, f in SC.NOT_PD_RUNS])
def test_a_near_copy_is_not_flagged(eng, p, flags):
    """x_dup = x_src + t noise with the true smallest pivot 1e3 .. 1e4 x the threshold (tests/test_small_cases_host.py): no
    NOT_PD, and the lifts within the rule of (a)."""
    d = SC.near_data(p)
    orders = SC.dup_orderings(p)
    ref = hp_ref.Problem(*d)
    eng.set_flags(flags)
    try:
        eng.load_data(*d, 0.0)
        for anti in (False, True):
            got = _run(eng, orders, anti)
            info = eng.info()
            want = ref.lifts(orders, anti)
            e_plain = float(np.abs(hp_ref.plain_lifts(*d, 0.0, orders, anti) - want).max())
            ratio = min(ref.min_pivot, ref.min_pivot_test) / threshold(p)
            assert 1e3 <= ratio <= 1e4, ratio
            assert info & 1 == 0, f"near copy flagged NOT_PD at a true pivot {ratio:.3g} x the threshold"
            r = judge(f"SMALL near copy p={p} flags={flags} anti={int(anti)}", got, want, e_plain, info & 1, ratio)
            key = (f"near copy, {SC.form_of(p, flags)}", SC.nb_of(p))       # a row of its own in test_report
            if not r <= WORST.get(key, (-1.0,))[0]:
                WORST[key] = (r, float(np.abs(got - want).max()), f"p{p}_f{flags}")
            assert info == 0
    finally:
        eng.set_flags(0)


# ---- e. workspace history --------------------------------------------------------------------------------------------------
def test_workspace_history_does_not_change_a_bit():
    """One engine: p = 127 fills the LDS form's 144 KB; p = 17 (nb = 2) and p = 47 (nb = 3) then run under both forms in
    LDS that holds the larger problem's matrices, p = 127 again in LDS that holds theirs.  Every block a kernel reads it
    has written in the same launch (the gather writes the identity padding too), so each result has the bits a fresh
    engine gives."""
    visits = [(127, 0), (17, 0), (17, SC.FLAG_LDS), (47, 0), (47, SC.FLAG_LDS), (127, 0)]
    want = {v: fresh_lifts(*v) for v in set(visits)}
    assert not np.array_equal(want[(47, 0)], want[(47, SC.FLAG_LDS)])
    e = HipEngine(0)
    try:
        for v in visits:
            np.testing.assert_array_equal(_visit(e, *v), want[v], err_msg=f"p = {v[0]}, flags = {v[1]}")
    finally:
        e.close()


def test_report():
    """Not a check: the worst r per (form, nb) of (a) and of the near copy of (d), the largest sum deviation and the wall
    time, for DESIGN.md (Numerics)."""
    for key in sorted(WORST):
        r, err, name = WORST[key]
        print(f"SMALL worst {key[0]} nb={key[1]}: r {r:.2f} err {err:.3e} at {name}")
    print(f"SMALL largest |sum - R^2| after a full fit: {SUMS['dev']:.3e}")
    print(f"SMALL seconds since the module was imported: {time.perf_counter() - T_START:.1f}")
