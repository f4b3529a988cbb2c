"""Host-only numpy restatement of k_rollout_gather (csrc/meshenv_rollout.h) and of DeviceRolloutBuffer.get: SB3 2.x's
``RolloutBuffer.swap_and_flatten`` + ``_get_samples`` over the histories ``collect_rollout`` leaves in [T][n] order, with the
kernel's rule for an index that is no row (the row is NaN in every field and nothing is read for it; the index is compared as
the 64-bit value it is, BEFORE it is narrowed: 2^32 + 3 is no row, not row 3.  tests/test_gpu_rollout_buffer.py enters the
branch with int32 and int64 permutations, ``narrowed_first`` is the wrong kernel it would tell).  Shared by
tests/test_rollout_buffer_cpu.py and tests/test_gpu_rollout_buffer.py; nothing here touches a device."""
from __future__ import annotations

import numpy as np

KEYS = ("obs", "buffer_actions", "value", "log_prob", "advantages", "returns")        # collect_rollout's names, the kernel's order
FIELDS = ("observations", "actions", "old_values", "old_log_prob", "advantages", "returns")   # SB3's RolloutBufferSamples
TAILS = ((18,), (3,), (), (), (), ())
SHAPES = ((1, 1), (3, 5), (7, 37), (32, 33))       # (T, n): rows 1, 15, 259, 1056: below and across a workgroup and a 1024-float chunk
BATCH_SIZES = (1, 4, 64, 100, None)


def rollout(T, n, seed=0):
    """A dict shaped like collect_rollout's (float32, [T][n] order); every element distinct within its field, so a row that
    lands anywhere but where it belongs shows."""
    rng = np.random.default_rng(seed + 1000 * T + n)
    out = {}
    for f, (k, tail) in enumerate(zip(KEYS, TAILS)):
        size = T * n * int(np.prod(tail, dtype=np.int64))
        x = (rng.permutation(size).astype(np.float32) + np.float32(0.25)) * np.float32(1 + f)
        out[k] = x.reshape((T, n) + tail)
    return out


def swap_and_flatten(arr):
    """stable_baselines3.common.buffers.BaseBuffer.swap_and_flatten: [T, n, ...] -> [n * T, ...], row i = env * T + t."""
    shape = arr.shape
    if len(shape) < 3:
        shape = (*shape, 1)
    return arr.swapaxes(0, 1).reshape(shape[0] * shape[1], *shape[2:])


def flat(out):
    """The six flattened fields under SB3's names; the four per-step scalars flattened to [rows] as _get_samples does."""
    res = {}
    for k, f, tail in zip(KEYS, FIELDS, TAILS):
        x = swap_and_flatten(np.asarray(out[k]))
        res[f] = np.ascontiguousarray(x if tail else x.reshape(-1))
    return res


def gather(out, perm):
    """What one launch writes: every row of every field in the order of ``perm`` (any integer dtype); an index outside
    [0, rows) gives a NaN row and reads nothing."""
    fl = flat(out)
    perm = np.asarray(perm).astype(np.int64)
    rows = fl["returns"].shape[0]
    assert perm.shape == (rows,)
    ok = (perm >= 0) & (perm < rows)
    safe = np.where(ok, perm, 0)
    res = {}
    for f, x in fl.items():
        y = x[safe].copy()
        y[~ok] = np.nan
        res[f] = y
    return res


def narrowed_first(perm):
    """The indices a kernel would see that cut an int64 index down to its low 32 bits (as a signed int32) before comparing it
    with the number of rows: the counter-example of the GPU test's int64 cases."""
    return np.asarray(perm).astype(np.int64).astype(np.uint64).astype(np.uint32).view(np.int32).astype(np.int64)


NOT_ROWS_32 = (-1, None, 2 ** 31 - 1)                                   # None stands for ``rows`` itself
NOT_ROWS_64 = NOT_ROWS_32 + (2 ** 32 + 3, -2 ** 32 + 5, 2 ** 63 - 1)  # the fourth and fifth alias rows 3 and 5 when narrowed first


def bounds(rows, batch_size):
    """SB3's ``while start_idx < rows`` loop: [(a, b)]; None is one minibatch of all rows, a shorter last one is kept."""
    b = rows if batch_size is None else batch_size
    return [(a, min(a + b, rows)) for a in range(0, rows, b)]


def get(out, perm, batch_size=None):
    """[dict of the six fields] per minibatch."""
    g = gather(out, perm)
    return [{f: x[a:b] for f, x in g.items()} for a, b in bounds(g["returns"].shape[0], batch_size)]
