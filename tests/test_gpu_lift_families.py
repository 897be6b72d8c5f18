"""The lifecycle the three sampled families share (lsspa_multi_lift_*, lsspa_cv_lift_*, lsspa_boot_lift_* of
include/lsspa.h): each keeps a player map, orderings and statistics of its own, and the host code that sets a map, checks
and stages orderings and keeps the running statistics is one path for all three.  What a merge of three copies can
break is checked here at the smallest shape that has every part: p = 5 columns with labels [-1, 0, 0, 1, 2] (a baseline,
a two-column group, g = 3), N = M = 24 rows, m = 3 responses, K = 2 folds, 6 samples, 3 replicates, antithetical pairs.

Everything is compared bitwise -- with fresh contexts that run the same calls, never with a reference -- or as text."""
import contextlib
import re

import numpy as np
import pytest

from ls_spa import _native as N
from ls_spa._engine import HipEngine

pytestmark = pytest.mark.gpu

P, M_RESP, ROWS, K, SAMPLES, REPS, BOOT_SEED = 5, 3, 24, 2, 6, 3, 7
LABELS = np.array([-1, 0, 0, 1, 2], dtype=np.int32)
G = 3
FAMILIES = ("multi", "cv", "boot")


def _data():
    rng = np.random.default_rng(20)
    Xa, Xe = rng.standard_normal((ROWS, P)), rng.standard_normal((ROWS, P))
    W = rng.standard_normal((P, M_RESP))
    Ya, Ye = Xa @ W + rng.standard_normal((ROWS, M_RESP)), Xe @ W + rng.standard_normal((ROWS, M_RESP))
    return Xa, Xe, Ya, Ye


DATA = _data()
FOLD_IDS = (np.arange(ROWS) % K).astype(np.int32)


def orderings(d, seed=3, count=SAMPLES):
    rng = np.random.default_rng(seed + d)
    return np.array([rng.permutation(d) for _ in range(count)], dtype=np.int32)


@contextlib.contextmanager
def fresh():
    eng = HipEngine(0)
    try:
        yield eng
    finally:
        eng.close()


def load(eng, fam):
    Xa, Xe, Ya, Ye = DATA
    if fam == "multi":
        eng.multi_lift_load(Xa, Xe, Ya, Ye, 0.0)
    elif fam == "cv":
        eng.cv_lift_load(Xa, Ya[:, 0], FOLD_IDS, K, 0.0)
    else:
        eng.boot_lift_load(Xa, Xe, Ya[:, 0], Ye[:, 0], 0.0)


def set_map(eng, fam, on):
    if on:
        getattr(eng, f"{fam}_lift_set_players")(LABELS)
    else:
        getattr(eng, f"{fam}_lift_clear_players")()


def run(eng, fam, perms):
    """One run of a family over perms, everything it returns as a flat list of arrays."""
    if fam == "multi":
        lifts = eng.multi_lift_batch(perms, True, want_lifts=True)
        n, mean, m2 = eng.multi_lift_get()
        return [lifts, mean, m2, np.array([n, eng.multi_lift_info()])]
    if fam == "cv":
        fold, tot = eng.cv_lift_batch(perms, True, want_lifts=True)
        n, mean, m2 = eng.cv_lift_get()
        return [fold, tot, mean, m2, np.array([n]), eng.cv_lift_info()]
    eng.boot_lift_set_orderings(perms, True)
    out = list(eng.boot_lift_run(REPS, BOOT_SEED, want_samples=True))
    point = eng.boot_lift_point(want_samples=True)
    return out + [np.asarray(a) for a in point]


def same(got, want, what):
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert a.shape == b.shape and a.tobytes() == b.tobytes(), f"{what}: array {k} differs"


NO_ORDERINGS = "no orderings set (lsspa_boot_lift_set_orderings comes first)"


def starts_over(eng, fam):
    """Right after a map is set or cleared: n = 0 (multi, CV); the orderings are gone (bootstrap)."""
    if fam == "boot":
        with pytest.raises(N.LSSPANativeError, match=re.escape(NO_ORDERINGS)):
            eng.boot_lift_run(REPS, BOOT_SEED)
    else:
        assert getattr(eng, f"{fam}_lift_get")()[0] == 0


@pytest.mark.parametrize("fam", FAMILIES)
def test_map_clear_map_is_three_fresh_contexts(fam):
    steps = [(True, orderings(G)), (False, orderings(P)), (True, orderings(G))]
    with fresh() as eng:
        load(eng, fam)
        got = []
        for on, perms in steps:
            set_map(eng, fam, on)
            starts_over(eng, fam)
            got.append(run(eng, fam, perms))
        getattr(eng, f"{fam}_lift_free")()
    for k, (on, perms) in enumerate(steps):
        with fresh() as eng:
            load(eng, fam)
            if on:
                set_map(eng, fam, True)
            same(got[k], run(eng, fam, perms), f"{fam}, step {k}")
            getattr(eng, f"{fam}_lift_free")()
    same(got[0], got[2], f"{fam}: the map set again")


def test_families_in_one_context_do_not_see_each_other():
    perms, again = orderings(G), orderings(G, seed=11)
    alone = {}
    for fam in FAMILIES:
        with fresh() as eng:
            load(eng, fam)
            set_map(eng, fam, True)
            first = run(eng, fam, perms)
            if fam != "boot":
                getattr(eng, f"{fam}_lift_reset")()
            alone[fam] = (first, run(eng, fam, again))
            getattr(eng, f"{fam}_lift_free")()
    with fresh() as eng:
        for fam in FAMILIES:             # loads, then maps, interleaved
            load(eng, fam)
        for fam in reversed(FAMILIES):
            set_map(eng, fam, True)
        half = SAMPLES // 2
        # the first run in pieces, another family's call between any two of one family's
        eng.multi_lift_batch(perms[:half], True)
        eng.cv_lift_batch(perms[:half], True)
        eng.boot_lift_set_orderings(perms, True)
        eng.multi_lift_reset()
        eng.cv_lift_reset()
        got = {"boot": run(eng, "boot", perms)}
        got["multi"] = run(eng, "multi", perms)
        eng.boot_lift_point()
        got["cv"] = run(eng, "cv", perms)
        for fam in FAMILIES:
            same(got[fam], alone[fam][0], f"{fam} beside the others")
        eng.multi_lift_free()            # one leaves, the others go on
        eng.cv_lift_reset()
        same(run(eng, "cv", again), alone["cv"][1], "cv after multi_lift_free")
        same(run(eng, "boot", again), alone["boot"][1], "boot after multi_lift_free")
        eng.cv_lift_free()
        same(run(eng, "boot", again), alone["boot"][1], "boot after cv_lift_free")
        eng.boot_lift_free()


NULL_LABELS = "lsspa: lsspa_{}_lift_set_players: labels is NULL (clear the map with labels = NULL, g = 0)"
NOT_A_PERMUTATION = {
    False: "lsspa: {}: a row of perms is not a permutation of 0 .. p-1",
    True: "lsspa: {}: a row of perms is not a permutation of 0 .. g-1 (a player map is set: the orderings are "
          "orderings of the groups)",
}
ENTRY = {"multi": "lsspa_multi_lift_batch", "cv": "lsspa_cv_lift_batch", "boot": "lsspa_boot_lift_set_orderings"}
NO_ROWS = {
    ("multi", False): "lsspa: lsspa_multi_lift_batch: perms is NULL, B < 1 or B p >= 2^31",
    ("multi", True): "lsspa: lsspa_multi_lift_batch: perms is NULL, B < 1 or 2 B p >= 2^31",
    ("cv", False): "lsspa: lsspa_cv_lift_batch: perms is NULL, B < 1 or 2 B p >= 2^31",
    ("cv", True): "lsspa: lsspa_cv_lift_batch: perms is NULL, B < 1 or 2 B p >= 2^31",
    ("boot", False): "lsspa: lsspa_boot_lift_set_orderings: perms is NULL, n_samples < 1 or 2 n_samples p >= 2^31",
    ("boot", True): "lsspa: lsspa_boot_lift_set_orderings: perms is NULL, n_samples < 1 or 2 n_samples p >= 2^31",
}


def give(eng, fam, perms):
    if fam == "boot":
        eng.boot_lift_set_orderings(perms, True)
    else:
        getattr(eng, f"{fam}_lift_batch")(perms, True)


@pytest.mark.parametrize("with_map", [False, True])
@pytest.mark.parametrize("fam", FAMILIES)
def test_refusal_texts(engine, fam, with_map):
    d = G if with_map else P
    try:
        load(engine, fam)
        if with_map:
            set_map(engine, fam, True)
        texts = []
        for call in (lambda: engine._check(getattr(engine._lib, f"lsspa_{fam}_lift_set_players")(engine._h, None, 2)),
                     lambda: give(engine, fam, np.array([list(range(d - 1)) + [d - 2]], dtype=np.int32)),
                     lambda: give(engine, fam, np.zeros((0, d), dtype=np.int32))):
            with pytest.raises(ValueError) as err:
                call()
            texts.append(str(err.value))
        assert texts == [NULL_LABELS.format(fam), NOT_A_PERMUTATION[with_map].format(ENTRY[fam]), NO_ROWS[fam, with_map]]
        # a refused call changes nothing: the family still runs, with the map it had
        run(engine, fam, orderings(d))
    finally:
        getattr(engine, f"{fam}_lift_free")()
