"""NumPy restatement of the sampled pairwise interaction index (include/lsspa.h, lsspa_pairs_*; csrc/k_pairs.hip):
the expansion of a sample into three orderings, the d - 1 second differences of a sample from its three lift vectors,
and the per-pair (count, mean, M2) tables -- Welford over a batch in sample order, one Chan merge into the table.
Vetted against the definition of I_ab in tests/test_pairs_host.py.  TESTS ONLY -- the product never imports this."""
from math import factorial

import numpy as np


def expand(perms):
    """(B, d) orderings -> (3 B, d): row 3 s is perms[s], row 3 s + 1 perms[s] with positions (0,1), (2,3), .. swapped,
    row 3 s + 2 with positions (1,2), (3,4), .. swapped."""
    perms = np.asarray(perms)
    B, d = perms.shape
    out = np.repeat(perms, 3, axis=0)
    for first, row in ((0, 1), (1, 2)):
        k = np.arange(first, d - 1, 2)
        out[row::3, k], out[row::3, k + 1] = perms[:, k + 1], perms[:, k]
    return out


def deltas(lifts3, perm):
    """Delta_k, k = 0 .. d-2, of one sample: lifts3 (3, d) are the lift vectors (indexed by player) of expand's three
    rows of `perm`.  With b = perm[k + 1]: Delta_k = lifts3[0][b] - lifts3[1 + (k & 1)][b], the second difference
    v(S+a+b) - v(S+a) - v(S+b) + v(S) of a = perm[k], b and S = perm[:k]."""
    perm = np.asarray(perm)
    k = np.arange(len(perm) - 1)
    b = perm[1:]
    return lifts3[0][b] - lifts3[1 + (k & 1), b]


class PairTables:
    """count (int64), mean, m2 [d][d], symmetric with a zero diagonal, the sum of all lift vectors and the sample count:
    the state lsspa_pairs_get returns."""

    def __init__(self, d):
        self.d, self.n = d, 0
        self.count = np.zeros((d, d), dtype=np.int64)
        self.mean, self.m2 = np.zeros((d, d)), np.zeros((d, d))
        self.phi_sum = np.zeros(d)
        self.max_abs = np.zeros((d, d))      # largest |Delta| a pair has seen (the tests' rounding bounds)

    def add_batch(self, lifts, perms):
        """lifts (3 B, d), perms (B, d): per pair Welford's update over the batch's hits in sample order, then Chan's
        merge of the batch into the table."""
        lifts, perms = np.asarray(lifts, dtype=np.float64), np.asarray(perms)
        B, d = perms.shape
        assert lifts.shape == (3 * B, d) and d == self.d
        batch = {}
        for s in range(B):
            x = deltas(lifts[3 * s:3 * s + 3], perms[s])
            lo, hi = np.minimum(perms[s, :-1], perms[s, 1:]), np.maximum(perms[s, :-1], perms[s, 1:])
            for a, b, v in zip(lo.tolist(), hi.tolist(), x.tolist()):
                c, m, q = batch.get((a, b), (0, 0.0, 0.0))
                c += 1
                dl = v - m
                m += dl / c
                q += dl * (v - m)
                batch[(a, b)] = (c, m, q)
                self.max_abs[a, b] = self.max_abs[b, a] = max(self.max_abs[a, b], abs(v))
        for (a, b), (c, m, q) in batch.items():
            n0 = int(self.count[a, b])
            if n0 == 0:
                n, mean, m2 = c, m, q
            else:
                n = n0 + c
                dl = m - self.mean[a, b]
                mean = self.mean[a, b] + dl * (c / n)
                m2 = self.m2[a, b] + q + dl * dl * (n0 * c / n)
            for i, j in ((a, b), (b, a)):
                self.count[i, j], self.mean[i, j], self.m2[i, j] = n, mean, m2
        for r in lifts:          # rows in order, as the device adds them
            self.phi_sum += r
        self.n += B
        return self

    @property
    def phi(self):
        return self.phi_sum / (3 * self.n)


def game_lifts(v, rows):
    """Lift vectors (len(rows), d), indexed by player, of orderings `rows` (n, d) in the game v [2^d] (v[mask], bit j =
    player j): lift[row[k]] = v(row[:k + 1]) - v(row[:k])."""
    rows = np.asarray(rows)
    n, d = rows.shape
    out = np.empty((n, d))
    mask = np.zeros(n, dtype=np.int64)
    for k in range(d):
        nxt = mask | (1 << rows[:, k])
        out[np.arange(n), rows[:, k]] = v[nxt] - v[mask]
        mask = nxt
    return out


def interaction_index(v, d):
    """I_ab = sum over S without a and b of |S|! (d - 2 - |S|)! / (d - 1)! (v(S+a+b) - v(S+a) - v(S+b) + v(S)), the
    definition, from the table v [2^d]; symmetric, zero diagonal."""
    masks = np.arange(1 << d, dtype=np.int64)
    size = np.array([bin(m).count("1") for m in masks])
    w = np.array([factorial(s) * factorial(d - 2 - s) / factorial(d - 1) for s in range(d - 1)])
    out = np.zeros((d, d))
    for a in range(d):
        for b in range(a + 1, d):
            S = masks[(masks & ((1 << a) | (1 << b))) == 0]
            dd = v[S | (1 << a) | (1 << b)] - v[S | (1 << a)] - v[S | (1 << b)] + v[S]
            out[a, b] = out[b, a] = np.sum(w[size[S]] * dd)
    return out
