"""NumPy restatement of the permutation test's permutations (csrc/host_perms.cpp: perm_indices) and a NumPy double of
the engine's perm_* methods.

TESTS ONLY.  pi for (seed, replicate r, side s in {0 train, 1 test}, n): Fisher-Yates on a[i] = i, for t = n - 1 down to
1 swap a[t] and a[j], j = (uint64(word) * (t + 1)) >> 32, word = word t % 4 of Philox4x32-10 with key = the 64-bit seed and
counter = (t / 4, 2 + s, r low, r high); then y_pi[i] = y[a[i]].
"""
import numpy as np

from oracle_engine import OracleEngine
from philox_ref import philox4x32_10
from test_multi_groups_host import multi_group_oracle
from test_multi_host import multi_gram_problem, multi_oracle_batched


def indices(seed, r, side, n):
    """a [n] (uint32): the permutation of (seed, r, side, n)."""
    seed, r = int(seed) & (2 ** 64 - 1), int(r) & (2 ** 64 - 1)
    a = np.arange(n, dtype=np.uint32)
    if n < 2:
        return a
    ctr = np.zeros(((n + 3) // 4, 4), dtype=np.uint64)
    ctr[:, 0] = np.arange((n + 3) // 4, dtype=np.uint64)
    ctr[:, 1] = 2 + side
    ctr[:, 2] = r & 0xFFFFFFFF
    ctr[:, 3] = r >> 32
    words = philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32)).reshape(-1)      # word t % 4 of counter t / 4 is words[t]
    for t in range(n - 1, 0, -1):
        j = (int(words[t]) * (t + 1)) >> 32
        a[t], a[j] = a[j], a[t]
    return a


def permuted_responses(y, seed, replicates, side):
    """Y [n][len(replicates)]: column k is y permuted by the permutation of replicate replicates[k]."""
    y = np.asarray(y, dtype=np.float64)
    return np.stack([y[indices(seed, r, side, len(y))] for r in replicates], axis=1)


class PermOracleEngine(OracleEngine):
    """What ls_spa_permutation_test asks of an engine, computed by the oracles of the multi-response tests on the
    explicitly permuted responses."""

    def __init__(self, info=0, fail_in=None):
        super().__init__()
        self.calls, self._info, self._fail_in = [], info, fail_in

    def _step(self, name):
        self.calls.append(name)
        if self._fail_in == name:
            raise RuntimeError(f"planted failure in {name}")

    def perm_load(self, Xa, Xe, ya, ye, reg):
        self._step("load")
        self._pd = tuple(np.asarray(a, dtype=np.float64) for a in (Xa, Xe, ya, ye))
        self._preg = reg

    def _phi(self, Ya, Ye, labels):
        Xa, Xe = self._pd[:2]
        if labels is None:
            return multi_oracle_batched(Xa, Xe, Ya, Ye, reg=self._preg)
        return multi_group_oracle(Xa, Xe, Ya, Ye, np.asarray(labels), reg=self._preg)

    def perm_observed(self, labels=None):
        self._step("observed")
        return self._phi(self._pd[2][:, None], self._pd[3][:, None], labels)[0], self._info

    def perm_run(self, R, seed, labels=None, first=0, sides=3, block=0):
        self._step("run")
        Xa, Xe, ya, ye = self._pd
        reps = range(first, first + R)
        Ya = permuted_responses(ya, seed, reps, 0) if sides & 1 else np.repeat(ya[:, None], R, axis=1)
        Ye = permuted_responses(ye, seed, reps, 1) if sides & 2 else np.repeat(ye[:, None], R, axis=1)
        _, g, _, h, _ = multi_gram_problem(Xa, Xe, Ya, Ye, self._preg)
        return self._phi(Ya, Ye, labels), g, h, self._info

    def perm_gram(self):
        Xa, Xe, ya, ye = self._pd
        G, g, H, h, yy = multi_gram_problem(Xa, Xe, ya[:, None], ye[:, None], self._preg)
        return G, g[0], H, h[0], float(yy[0])

    def perm_free(self):
        self.calls.append("free")


# The X^T y[pi] cases of tests/test_gpu_permutation_test.py: (N, M, p, groups g or 0, R, block).  Kept here so that the
# CPU test of the plan (tests/test_permutation_host.py) can prove which edges they reach.  With g the columns are cut
# into g groups round-robin (the gathered pass does not know about groups; they keep the enumeration of p = 32 .. 64
# columns cheap).  Between them: n in {1, 3, 4, 5, 63, 64, 65} and 255 / 256 / 257 (a slice is 256 rows at these sizes),
# p in {1, 15, 16, 17, 32} and {33, 48, 64}, R in {1, 15, 16, 17, 63, 65}, M < p.
XTY_CASES = [
    (1, 3, 1, 0, 1, 0),
    (4, 5, 15, 0, 15, 0),
    (63, 64, 16, 0, 16, 0),
    (65, 255, 17, 0, 17, 8),
    (256, 257, 32, 3, 63, 0),
    (257, 512, 5, 0, 65, 0),
    (513, 40, 32, 4, 65, 16),
    (64, 65, 33, 3, 17, 0),
    (300, 20, 48, 4, 16, 0),
    (257, 70, 64, 5, 15, 8),
]


def case_labels(p, g):
    return None if not g else (np.arange(p) % g).astype(np.int32)
