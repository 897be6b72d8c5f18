"""NumPy restatement of the bootstrap's row draws (include/lsspa.h, lsspa_boot_run; csrc/k_boot.hip: boot_counts_kernel).

TESTS ONLY.  Draw t = 0 .. n-1 of replicate r on side s (0 train, 1 test) picks row (word * n) >> 32, where word is output
word t % 4 of Philox4x32-10 (tests/philox_ref.py) with key = the 64-bit seed and counter = (t / 4, s, r low, r high)."""
import numpy as np

from philox_ref import philox4x32_10


def indices(seed, r, side, n):
    """The n rows drawn, in draw order (int64)."""
    calls = (n + 3) // 4
    ctr = np.zeros((calls, 4), dtype=np.uint64)
    ctr[:, 0] = np.arange(calls, dtype=np.uint64)
    ctr[:, 1] = side
    ctr[:, 2] = int(r) & 0xFFFFFFFF
    ctr[:, 3] = (int(r) >> 32) & 0xFFFFFFFF
    seed = int(seed) & (2 ** 64 - 1)
    words = philox4x32_10(ctr, (seed & 0xFFFFFFFF, seed >> 32)).reshape(-1)[:n]      # < 2^32 each, n < 2^31: no overflow
    return ((words * np.uint64(n)) >> np.uint64(32)).astype(np.int64)


def counts(seed, r, side, n):
    """cnt [n] (uint32): how often each row is drawn."""
    out = np.zeros(n, dtype=np.uint32)
    np.add.at(out, indices(seed, r, side, n), 1)
    return out
