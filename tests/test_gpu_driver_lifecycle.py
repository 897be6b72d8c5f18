"""The kept engine handed round every public entry point: whatever a call sets on it -- a player map, pair tables, a
flag, a lane count, a precision -- the next call, of any kind, finds an engine that computes what a fresh one does."""
import numpy as np
import pytest

import ls_spa as package
from ls_spa import ls_spa, ls_spa_groups, ls_spa_interactions, ls_spa_interactions_sampled
from test_subsets_host import data

pytestmark = pytest.mark.gpu

P, GROUPS = 12, np.arange(12) // 3      # four groups of three columns
FIELDS = ("attribution", "theta", "interactions", "counts")


def test_kept_engine_gives_every_entry_point_a_fresh_engines_result():
    d = data(P, n=300, m=200, seed=12)
    calls = {
        "ls_spa": lambda: ls_spa(*d, method="argsort", max_samples=512, batch_size=128),
        "subsets": lambda: ls_spa(*d, method="subsets"),
        "interactions": lambda: ls_spa_interactions(*d, groups=GROUPS),
        "groups": lambda: ls_spa_groups(*d, GROUPS, method="argsort", max_samples=512, batch_size=128),
        "pairs": lambda: ls_spa_interactions_sampled(*d, max_samples=64, batch_size=32, precision="float32"),
    }
    package.release()
    fresh = {}
    for name, call in calls.items():
        package.release()
        fresh[name] = call()
    package.release()
    orders = (("ls_spa", "subsets", "interactions", "groups", "pairs"),
              ("subsets", "interactions", "pairs", "groups", "ls_spa"))      # fp32 pair tables and a player map, then ls_spa
    try:
        for order in orders:
            for name in order:
                got = calls[name]()
                for field in FIELDS:
                    if hasattr(fresh[name], field):
                        assert np.array_equal(getattr(got, field), getattr(fresh[name], field)), (order, name, field)
    finally:
        package.release()
