"""The lifecycle every public entry point of the driver wraps round its GPU work, on a recording test double: whose
engine it is (kept, made for the call, the caller's), what is bound, loaded, fitted, reset, closed and released, in which
order, after success and after an exception; what the info bits turn into; which frame a warning is attributed to;
which phases ``_timings`` names; how the estimator, look-ahead and lane defaults are resolved.  No GPU.

Apart from ``test_option_function``, which calls the function the defaults were pulled into, nothing here knows how the
driver is organised: the tests drive the public functions and read the double's log."""
import threading
import warnings

import numpy as np
import pytest

from ls_spa import (LSSPANativeError, _driver, ls_spa, ls_spa_groups, ls_spa_interactions,
                    ls_spa_interactions_sampled)
from test_group_interactions_host import GroupInteractionsOracleEngine
from test_groups_host import labels_of
from test_pairs_host import PairsOracleEngine
from test_subsets_host import data

P = 10
DATA = data(P, seed=90)
LABELS = labels_of([3, 3, 3], 1, seed=4)      # g = 3 and one baseline column
NOT_PD = ("a permuted Gram matrix was not numerically positive definite; the attribution of collinear features is not "
          "meaningful (the reference's is not either)")
REPEAT = "engine fault in the fused lift scan (info bits 8): the run is repeated with the lift kernel of its own"
SUM_FAULT = ("a sample's lifts did not sum to the R^2 of the full model (info bits 8): the lift vectors of this run are "
             "not valid (engine fault)")
SCAN_FAULT = ("the fused lift scan gave up waiting for a row of its panel (info bits 4): the lift vectors of this run "
              "are not valid (engine fault)")


class Boom(Exception):
    pass


class RecordingEngine(PairsOracleEngine, GroupInteractionsOracleEngine):
    """Every double of the host tests in one (sampling with a player map, pair tables, both enumerations), with the
    methods only a call on an engine of its own needs; each call of a recorded method is a (name, args, kwargs) entry
    of ``log``.  fail: the method that raises ``boom``; fit_info: full_fit's info; collected: what info_collected
    returns, call by call (then 0)."""
    RECORDED = ("set_precision", "set_lanes", "set_flags", "history_enable", "load_data", "load_data_sharded",
                "full_fit", "set_players", "clear_players", "pairs_enable", "pairs_batch", "pairs_get", "run_batch",
                "launch_batch", "subsets_shapley", "groups_shapley", "subsets_interactions", "groups_interactions",
                "info_collected", "reduce_timing", "close")

    def __init__(self, log, fail=None, fit_info=0, collected=()):
        super().__init__()
        self.log, self.fail, self.boom = log, fail, Boom("injected")
        self.fit_info, self.collected = fit_info, list(collected)
        for name in self.RECORDED:
            if hasattr(self, name):
                setattr(self, name, self._recorded(name, getattr(self, name)))

    def _recorded(self, name, method):
        def call(*args, **kwargs):
            self.log.append((name, args, kwargs))
            if name == self.fail:
                raise self.boom
            return method(*args, **kwargs)
        return call

    def set_precision(self, name):
        self.precision = name

    def set_flags(self, flags):
        self.flags = flags

    def full_fit(self):
        theta, r_squared, _ = super().full_fit()
        return theta, r_squared, self.fit_info

    def info_collected(self):
        return self.collected.pop(0) if self.collected else 0

    def close(self):
        self.closed = True


class TimedRecordingEngine(RecordingEngine):
    def reduce_timing(self):
        return {"pin": 0.0, "h2d_gram": 1e-4, "unpin": 0.0, "finalize": 1e-5}


class Comm(_driver._Comm):
    """A world of one that can be bound and closed."""

    def __init__(self, log):
        self.log = log

    def bind(self, engine):
        self.log.append(("comm.bind", (engine,), {}))

    def close(self):
        self.log.append(("comm.close", (), {}))


class Source:
    """An ordering source whose close is seen."""

    def __init__(self, source, log):
        self._source, self._log = source, log

    def __getattr__(self, name):
        return getattr(self._source, name)

    def close(self):
        self._log.append(("source.close", (), {}))
        if hasattr(self._source, "close"):
            self._source.close()


# name -> (the call, the method that is its first batch of GPU work, takes comm=, sets a player map, uses pair tables,
# has an ordering source).  The calls are made from this file: a warning for the caller names it.
ENTRIES = {
    "ls_spa": (lambda **kw: ls_spa(*DATA, method="random", max_samples=32, batch_size=16, **kw),
               "run_batch", True, False, False, True),
    "subsets": (lambda **kw: ls_spa(*DATA, method="subsets", **kw),
                "subsets_shapley", True, False, False, False),
    "interactions": (lambda **kw: ls_spa_interactions(*DATA, groups=LABELS, **kw),
                     "groups_interactions", True, False, False, False),
    "groups": (lambda **kw: ls_spa_groups(*DATA, LABELS, method="random", max_samples=32, batch_size=16, **kw),
               "run_batch", False, True, False, True),
    "pairs": (lambda **kw: ls_spa_interactions_sampled(*DATA, groups=LABELS, max_samples=16, batch_size=8, **kw),
              "pairs_batch", False, True, True, True),
}
ALL = sorted(ENTRIES)
WITH_COMM = [n for n in ALL if ENTRIES[n][2]]


def names(log):
    return [entry[0] for entry in log]


def at(log, name, *args):
    """Positions in the log of the calls of `name` (with exactly these positional arguments, if any are given)."""
    return [k for k, entry in enumerate(log) if entry[0] == name and (not args or entry[1] == args)]


@pytest.fixture
def stage(monkeypatch):
    """log, and own(engine, kept): the next engine the driver acquires is this one, with a held lock if it is a kept
    one.  prepare_sampling is the driver's, recorded, its source wrapped; without own() acquiring an engine fails."""
    log = []
    real_prepare = _driver.prepare_sampling

    def prepare(*args, **kwargs):
        log.append(("prepare_sampling", args, kwargs))
        out = list(real_prepare(*args, **kwargs))
        out[1] = Source(out[1], log)
        return tuple(out)

    def nobody(device):
        raise AssertionError("an engine was acquired")

    def own(engine, kept=True):
        lock = None
        if kept:
            lock = threading.Lock()
            lock.acquire()

        def acquire(device):
            log.append(("_acquire_engine", (device,), {}))
            return engine, lock
        monkeypatch.setattr(_driver, "_acquire_engine", acquire)
        return lock

    monkeypatch.setattr(_driver, "prepare_sampling", prepare)
    monkeypatch.setattr(_driver, "_acquire_engine", nobody)
    return log, own


def check_cleanups(log, name, done):
    """After success: the player map cleared and the pair tables given back, after the work; after a failure: neither.
    The ordering source is closed either way."""
    _, work, _, players, pairs, source = ENTRIES[name]
    if source:
        assert at(log, "source.close")
    last_work = max(at(log, work), default=-1)
    if done:
        if players:
            assert len(at(log, "clear_players")) == 1 and at(log, "clear_players")[0] > last_work
        if pairs:
            assert len(at(log, "pairs_enable", False)) == 1 and at(log, "pairs_enable", False)[0] > last_work
    else:
        assert not at(log, "clear_players") and not at(log, "pairs_enable", False)
    return last_work


# ---- 1. whose engine it is -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_kept_engine_after_success(stage, name):
    log, own = stage
    lock = own(RecordingEngine(log))
    ENTRIES[name][0]()
    assert not at(log, "close")
    last_work = check_cleanups(log, name, done=True)
    assert len(at(log, "set_flags", 0)) == 1 and len(at(log, "history_enable", 0)) == 1
    reset = at(log, "set_flags", 0)[0]
    assert last_work < reset < at(log, "history_enable", 0)[0]
    assert all(k < reset for k in at(log, "clear_players") + at(log, "pairs_enable", False))
    assert not lock.locked()


@pytest.mark.parametrize("where", ["full_fit", "work"])
@pytest.mark.parametrize("name", ALL)
def test_kept_engine_after_an_exception(stage, name, where):
    log, own = stage
    engine = RecordingEngine(log, fail=ENTRIES[name][1] if where == "work" else "full_fit")
    lock = own(engine)
    with pytest.raises(Boom) as caught:
        ENTRIES[name][0]()
    assert caught.value is engine.boom
    assert names(log)[-1] == "close" and len(at(log, "close")) == 1      # not trusted with another call
    assert not at(log, "set_flags", 0) and not at(log, "history_enable", 0)
    check_cleanups(log, name, done=False)
    assert not lock.locked()


@pytest.mark.parametrize("kept", [True, False])
@pytest.mark.parametrize("name", ["groups", "pairs"])
def test_owned_engine_whose_cleanup_raises_is_closed(stage, name, kept):
    """The body succeeded, clearing the player map did not: the engine may still carry it, so no later call gets it."""
    log, own = stage
    engine = RecordingEngine(log, fail="clear_players")
    lock = own(engine, kept=kept)
    with pytest.raises(Boom) as caught:
        ENTRIES[name][0]()
    assert caught.value is engine.boom
    assert names(log)[-1] == "close" and len(at(log, "close")) == 1
    assert at(log, "source.close") and not at(log, "set_flags", 0) and not at(log, "history_enable", 0)
    assert lock is None or not lock.locked()


@pytest.mark.parametrize("name", ALL)
def test_engine_made_for_the_call_is_closed(stage, name):
    log, own = stage
    own(RecordingEngine(log), kept=False)
    ENTRIES[name][0]()
    assert names(log)[-1] == "close" and len(at(log, "close")) == 1
    assert not at(log, "set_flags") and not at(log, "history_enable")
    check_cleanups(log, name, done=True)


@pytest.mark.parametrize("name", ALL)
def test_callers_engine_is_neither_closed_nor_reset(stage, name):
    log, _ = stage
    ENTRIES[name][0](_engine=RecordingEngine(log))      # (acquiring one fails)
    assert not at(log, "close") and not at(log, "set_flags") and not at(log, "history_enable")
    check_cleanups(log, name, done=True)


@pytest.mark.parametrize("name", ALL)
def test_callers_engine_after_an_exception(stage, name):
    log, _ = stage
    engine = RecordingEngine(log, fail=ENTRIES[name][1])
    with pytest.raises(Boom) as caught:
        ENTRIES[name][0](_engine=engine)
    assert caught.value is engine.boom
    assert not at(log, "close") and not at(log, "set_flags") and not at(log, "history_enable")
    check_cleanups(log, name, done=False)


@pytest.mark.parametrize("name", ["ls_spa", "groups", "pairs"])
def test_acquiring_fails(stage, name):
    log, _ = stage      # the ordering source exists by then: it is closed
    with pytest.raises(AssertionError, match="an engine was acquired"):
        ENTRIES[name][0]()
    assert names(log) == ["prepare_sampling", "source.close"]


# ---- 2. the communicator ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kept", [True, False])
@pytest.mark.parametrize("name", WITH_COMM)
def test_communicator_of_an_owned_engine(stage, name, kept):
    log, own = stage
    engine = RecordingEngine(log)
    own(engine, kept=kept)
    ENTRIES[name][0](comm=Comm(log))
    assert len(at(log, "comm.bind")) == 1 and log[at(log, "comm.bind")[0]][1] == (engine,)
    assert at(log, "_acquire_engine")[0] < at(log, "comm.bind")[0] < at(log, "load_data")[0]
    assert len(at(log, "comm.close")) == 1
    assert at(log, "comm.close")[0] < (at(log, "set_flags", 0) if kept else at(log, "close"))[0]
    assert at(log, "comm.close")[0] > max(at(log, ENTRIES[name][1]))


@pytest.mark.parametrize("name", WITH_COMM)
def test_communicator_of_an_owned_engine_is_closed_after_an_exception(stage, name):
    log, own = stage
    own(RecordingEngine(log, fail=ENTRIES[name][1]))
    with pytest.raises(Boom):
        ENTRIES[name][0](comm=Comm(log))
    assert len(at(log, "comm.close")) == 1 and at(log, "comm.close")[0] < at(log, "close")[0]


@pytest.mark.parametrize("name", WITH_COMM)
def test_communicator_of_the_callers_engine_stays_open(stage, name):
    log, _ = stage
    ENTRIES[name][0](comm=Comm(log), _engine=RecordingEngine(log))
    assert len(at(log, "comm.bind")) == 1 and at(log, "comm.bind")[0] < at(log, "load_data")[0]
    assert not at(log, "comm.close")


def test_entry_points_without_a_communicator(stage):
    log, _ = stage
    engine = RecordingEngine(log)
    with pytest.raises(TypeError):
        ENTRIES["pairs"][0](comm=Comm(log), _engine=engine)
    for kw in (dict(comm=Comm(log)), dict(checkpoint="state.npz"), dict(row_sharded=True)):
        with pytest.raises(ValueError, match="ls_spa_groups does not take " + next(iter(kw))):
            ENTRIES["groups"][0](_engine=engine, **kw)
    assert log == []


@pytest.mark.parametrize("name", WITH_COMM)
@pytest.mark.parametrize("row_sharded, shard_test", [(True, True), ("train", False)])
def test_row_sharded_load(stage, name, row_sharded, shard_test):
    log, _ = stage
    comm = Comm(log)
    ENTRIES[name][0](row_sharded=row_sharded, comm=comm, _engine=RecordingEngine(log))
    (_, args, kwargs), = [log[k] for k in at(log, "load_data_sharded")]
    assert args[5] is comm and kwargs == {"shard_test": shard_test} and not at(log, "load_data")
    assert at(log, "load_data_sharded")[0] < at(log, "full_fit")[0]
    log.clear()
    ENTRIES[name][0](row_sharded=row_sharded, _engine=RecordingEngine(log))      # a world of one by default
    assert type(log[at(log, "load_data_sharded")[0]][1][5]) is _driver._Comm


# ---- 3. the info bits ------------------------------------------------------------------------------------------------
def caught_by(name, **kw):
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        result = ENTRIES[name][0](**kw)
    return result, [w for w in seen if issubclass(w.category, RuntimeWarning)]


@pytest.mark.parametrize("name", ALL)
def test_singular_full_fit_warns_and_takes_the_minimum_norm_fit(stage, monkeypatch, name):
    log, _ = stage
    theta = np.arange(float(P))
    monkeypatch.setattr(_driver, "_singular_fit", lambda engine, X_test, y_test: (theta, 0.25))
    result, seen = caught_by(name, _engine=RecordingEngine(log, fit_info=1))
    assert [str(w.message) for w in seen] == [NOT_PD]
    # the caller's frame -- for ls_spa_groups that of its own call of ls_spa, as ever
    assert seen[0].filename == (_driver.__file__ if name == "groups" else __file__)
    assert result.theta is theta and result.r_squared == 0.25


@pytest.mark.parametrize("name", ["ls_spa", "groups", "pairs"])
def test_singular_batch_warns_and_keeps_the_full_fit(stage, name):
    log, _ = stage
    plain = ENTRIES[name][0](_engine=RecordingEngine(log))
    for bits in (1, 9):      # with bit 1 the sum check's bit is no fault
        result, seen = caught_by(name, _engine=RecordingEngine(log, collected=[bits]))
        assert [str(w.message) for w in seen] == [NOT_PD]
        assert seen[0].filename == (_driver.__file__ if name == "groups" else __file__)
        np.testing.assert_array_equal(result.theta, plain.theta)
        assert not at(log, "set_flags")


@pytest.mark.parametrize("name", ["subsets", "interactions"])
def test_singular_subset_warns(stage, name):
    log, _ = stage
    engine = RecordingEngine(log)
    engine._info = 1
    _, seen = caught_by(name, _engine=engine)
    assert [str(w.message) for w in seen] == [NOT_PD] and seen[0].filename == __file__


@pytest.mark.parametrize("name", ["groups", "pairs"])
@pytest.mark.parametrize("bits, text", [pytest.param(8, SUM_FAULT, id="sum"), pytest.param(4, SCAN_FAULT, id="scan")])
def test_fault_bits_raise(stage, name, bits, text):
    log, own = stage
    lock = own(RecordingEngine(log, collected=[bits, bits]))
    with pytest.raises(LSSPANativeError) as caught, warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ENTRIES[name][0]()
    assert str(caught.value) == text
    assert names(log)[-1] == "close" and not lock.locked()
    check_cleanups(log, name, done=False)


def test_fault_with_orderings_of_the_caller_raises_at_once(stage):
    log, _ = stage
    perms = [np.random.default_rng(k).permutation(P) for k in range(8)]
    with pytest.raises(LSSPANativeError) as caught:
        ls_spa(*DATA, perms=perms, _engine=RecordingEngine(log, collected=[8]))
    assert str(caught.value) == SUM_FAULT and not at(log, "set_flags")


def test_fault_with_a_seeded_source_is_repeated_once(stage):
    log, _ = stage
    plain = ENTRIES["ls_spa"][0](_engine=RecordingEngine(log))
    log.clear()
    result, seen = caught_by("ls_spa", _engine=RecordingEngine(log, collected=[8, 0]))
    assert [str(w.message) for w in seen] == [REPEAT] and seen[0].filename == __file__
    assert [log[k][1] for k in at(log, "set_flags")] == [(512,)]
    first, second = at(log, "prepare_sampling")
    flagged = at(log, "set_flags", 512)[0]
    runs = at(log, "run_batch")
    assert len(at(log, "info_collected")) == 2 and len(at(log, "full_fit")) == len(at(log, "load_data")) == 1
    assert [k < flagged for k in runs] == [True] * (len(runs) // 2) + [False] * (len(runs) // 2)
    assert any(flagged < k < second for k in at(log, "source.close"))      # the first source, before the second is made
    assert at(log, "source.close")[-1] > runs[-1]
    np.testing.assert_array_equal(result.attribution, plain.attribution)      # the same orderings again
    # twice: the run is lost
    with pytest.raises(LSSPANativeError) as caught, warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ENTRIES["ls_spa"][0](_engine=RecordingEngine(log, collected=[8, 8]))
    assert str(caught.value) == SUM_FAULT


# ---- 4. order ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ls_spa", "groups", "pairs"])
def test_order_of_a_sampling_call(stage, name):
    log, own = stage
    own(RecordingEngine(log))
    ENTRIES[name][0](precision="float32")
    work = ENTRIES[name][1]
    order = [at(log, step)[0] for step in ("prepare_sampling", "_acquire_engine", "set_precision", "load_data",
                                           "full_fit")]
    if ENTRIES[name][3]:
        order.append(at(log, "set_players")[0])
        assert len(at(log, "set_players")) == 1
    if ENTRIES[name][4]:
        order.append(at(log, "pairs_enable", True)[0])
    order.append(at(log, work)[0])
    assert order == sorted(order)
    assert log[at(log, "set_precision")[0]][1] == ("float32",)


@pytest.mark.parametrize("name", ["subsets", "interactions"])
def test_enumerations_run_in_float64_and_build_no_sampler(stage, name):
    log, own = stage
    engine = RecordingEngine(log)
    engine.precision = "float32"      # what an earlier call left on a kept engine
    own(engine)
    ENTRIES[name][0]()
    assert [log[k][1] for k in at(log, "set_precision")] == [("float64",)]
    order = [at(log, step)[0] for step in ("_acquire_engine", "set_precision", "load_data", "full_fit",
                                           ENTRIES[name][1])]
    assert order == sorted(order) and not at(log, "prepare_sampling")


def test_value_errors_come_before_any_engine_work(stage):
    log, _ = stage
    engine = RecordingEngine(log)
    bad_y = (DATA[0], DATA[1], DATA[2][:, None], DATA[3])
    for call in (lambda: ls_spa(*bad_y, _engine=engine), lambda: ls_spa_interactions(*bad_y, _engine=engine),
                 lambda: ls_spa_groups(*bad_y, LABELS, method="random", _engine=engine),
                 lambda: ls_spa_interactions_sampled(*bad_y, _engine=engine)):
        with pytest.raises(ValueError, match="y_train and y_test must be one-dimensional"):
            call()
    with pytest.raises(ValueError, match="error_estimator must be None, 'reference', 'lowrank' or 'device'"):
        ls_spa(*DATA, error_estimator="exact", _engine=engine)
    with pytest.raises(ValueError, match="method must be one of"):
        ls_spa(*DATA, method="sobol", _engine=engine)
    with pytest.raises(ValueError, match="exact path only"):
        ls_spa(*DATA, groups=LABELS, _engine=engine)
    with pytest.raises(ValueError, match="no attribution history"):
        ls_spa(*DATA, method="subsets", return_history=True, _engine=engine)
    with pytest.raises(ValueError, match="gap in its numbering"):
        ls_spa_interactions(*DATA, groups=[0, 0, 0, 2, 2, 2, 3, 3, 3, -1], _engine=engine)
    with pytest.raises(ValueError, match="batch_size and max_samples must be positive"):
        ls_spa_interactions_sampled(*DATA, batch_size=0, _engine=engine)
    assert [n for n in names(log) if n not in ("prepare_sampling", "source.close")] == []


# ---- 5. _timings -------------------------------------------------------------------------------------------------------
PHASES = {"sampler_start", "engine_create", "setup", "final_fit", "teardown", "sampler", "estimator", "sampling"}
SPLIT = {"reduction_pin", "reduction_copy_gram", "reduction_unpin", "reduction_finalize", "reduction_host"}


@pytest.mark.parametrize("owned", [True, False])
@pytest.mark.parametrize("name", ["ls_spa", "groups"])
def test_timing_keys(stage, name, owned):
    log, own = stage
    for engine, reduction in ((RecordingEngine(log), {"reduction_h2d_gram"}), (TimedRecordingEngine(log), SPLIT)):
        tm = {}
        if owned:
            own(engine)
            ENTRIES[name][0](_timings=tm)
        else:
            ENTRIES[name][0](_timings=tm, _engine=engine)
        assert set(tm) == PHASES | reduction
        assert all(isinstance(v, float) and v >= 0 for k, v in tm.items() if k != "reduction_host")


# ---- 6. estimator, look-ahead and lanes when nobody names them ----------------------------------------------------------
ORDERINGS = "orderings"      # stands for perms= of the right width
OPTIONS = [
    # method, perms, p, what the caller names -> estimator, look-ahead, lanes
    (None, None, 10, {}, ("reference", 1, 1)),
    ("random", None, 10, {}, ("reference", 1, 1)),
    ("exact", None, 10, {}, ("reference", 1, 1)),
    ("argsort", None, 10, {}, ("device", "auto", 1)),
    ("permutohedron", None, 10, {}, ("device", "auto", 1)),
    ("argsort", None, 127, {}, ("device", "auto", 1)),
    ("argsort", None, 128, {}, ("device", "auto", 2)),
    ("permutohedron", None, 128, {}, ("device", "auto", 2)),
    ("random", None, 128, {}, ("reference", 1, 1)),
    (None, None, 128, {}, ("reference", 1, 1)),
    (None, ORDERINGS, 128, {}, ("reference", 1, 1)),
    (None, ORDERINGS, 10, {"error_estimator": "device"}, ("device", 1, 1)),
    ("random", None, 10, {"error_estimator": "device"}, ("device", 1, 1)),
    ("argsort", None, 128, {"error_estimator": "reference"}, ("reference", 1, 2)),
    ("argsort", None, 10, {"error_estimator": "lowrank"}, ("lowrank", 1, 1)),
    ("argsort", None, 10, {"error_estimator": "reference", "lookahead": "auto"}, ("reference", "auto", 1)),
    ("argsort", None, 10, {"lookahead": 4}, ("device", 4, 1)),
    ("random", None, 10, {"lookahead": 3, "lanes": 2}, ("reference", 3, 2)),
    ("argsort", None, 128, {"lanes": 1}, ("device", "auto", 1)),
    ("argsort", None, 10, {"lanes": 2}, ("device", "auto", 2)),
    ("argsort", None, 10, {"error_estimator": "exact"}, "error_estimator must be None, 'reference', 'lowrank' or 'device'"),
    ("argsort", None, 10, {"lookahead": 0}, "lookahead must be >= 1 or 'auto'"),
    ("random", None, 10, {"lookahead": -2}, "lookahead must be >= 1 or 'auto'"),
    ("argsort", None, 128, {"lanes": 3}, "lanes must be 1, 2 or 'auto'"),
    ("random", None, 10, {"lanes": 0}, "lanes must be 1, 2 or 'auto'"),
]
_wide = {}


@pytest.mark.parametrize("method, perms, p, given, want", OPTIONS)
def test_options_as_the_sampling_loop_and_the_engine_get_them(monkeypatch, method, perms, p, given, want):
    got = {}

    def prepare(dim, **kwargs):
        return None, object(), kwargs["batch_size"], kwargs["antithetical"], kwargs["max_samples"], False

    def run(engine, dim, **kwargs):
        got.update(kwargs)
        return np.zeros(dim), np.zeros(dim), 0.0, np.zeros(0), None, 0

    monkeypatch.setattr(_driver, "prepare_sampling", prepare)
    monkeypatch.setattr(_driver, "run_estimator", run)
    if p not in _wide:
        _wide[p] = data(p, n=p + 20, m=p + 10, seed=p)
    engine = RecordingEngine([])
    call = lambda: ls_spa(*_wide[p], method=method, perms=None if perms is None else [np.arange(p)], _engine=engine,
                          **given)
    if isinstance(want, str):
        with pytest.raises(ValueError, match=want):
            call()
        assert not at(engine.log, "run_batch")
    else:
        call()
        assert (got["error_estimator"], got["lookahead"], engine.lanes) == want


@pytest.mark.parametrize("method, perms, p, given, want", OPTIONS)
def test_option_function(method, perms, p, given, want):
    args = (method, None if perms is None else [np.arange(p)], p)
    if isinstance(want, str):
        with pytest.raises(ValueError, match=want):
            _driver._sampling_options(*args, **given)
    else:
        assert _driver._sampling_options(*args, **given) == want
