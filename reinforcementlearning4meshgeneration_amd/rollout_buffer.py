"""The minibatches of SB3 2.x's ``RolloutBuffer.get`` on the GPU (include/meshenv_rollout.h, csrc/meshenv_rollout.h:
k_rollout_gather): per epoch of ``PPO.train`` / ``A2C.train``,

    indices = np.random.permutation(self.buffer_size * self.n_envs)
    ... swap_and_flatten of every field ...
    yield self._get_samples(indices[start_idx : start_idx + batch_size])

as ONE launch: every row of the six fields is written in permuted order into six buffers the object owns, and the minibatches
are contiguous slices of them.

    rb = DeviceRolloutBuffer(device=0)
    rb.load(out)                                  # out = venv.collect_rollout(policy, T, gamma=..., gae_lambda=...): references, no copy
    for epoch in range(n_epochs):
        for rollout_data in rb.get(batch_size):   # one k_rollout_gather launch, then views
            pg.backward(rollout_data, ...); fo.policy_step()

The flat row index is SB3's ``swap_and_flatten``: ``i = env * T + t``.  So ``perm=torch.from_numpy(np.random.permutation(rows))``
reproduces SB3's minibatches bit for bit; without a ``perm`` the object draws ``torch.randperm(rows)`` on the device.

THE VIEWS A ``get`` YIELDS ARE VALID UNTIL THE NEXT ``get``: it overwrites the same buffers.

The functions of this module that take no device (``check_rollout``, ``check_perm``, ``minibatch_bounds``) are the host half:
every refusal is made by them."""
from __future__ import annotations

import ctypes as C
from collections import namedtuple
from typing import List, Optional, Tuple

from . import _capi
from ._handle import Handle

OBS_DIM, ACT_DIM = _capi.OBS_DIM, _capi.ACT_DIM
MAX_ROWS = _capi.ROLLOUT_MAX_ROWS
# (key of collect_rollout's dict, trailing shape, field of RolloutBufferSamples), in meshenv_rollout_gather's order
FIELDS = (("obs", (OBS_DIM,), "observations"), ("buffer_actions", (ACT_DIM,), "actions"), ("value", (), "old_values"),
          ("log_prob", (), "old_log_prob"), ("advantages", (), "advantages"), ("returns", (), "returns"))

# SB3's stable_baselines3.common.type_aliases.RolloutBufferSamples: name, field order and shapes ([B, 18], [B, 3], [B] x 4)
RolloutBufferSamples = namedtuple("RolloutBufferSamples", [f for _, _, f in FIELDS])


def check_rollout(out, device=None) -> Tuple[int, int, list]:
    """(T, n, the six tensors in FIELDS' order) of a ``collect_rollout`` dict, or a ValueError that names what is wrong: a
    missing key, a dtype, a shape, a layout, a device (``device`` None: the device of ``obs``)."""
    import torch
    if not hasattr(out, "keys"):
        raise ValueError(f"load() takes the dict collect_rollout returns, got {type(out).__name__}")
    missing = [k for k, _, _ in FIELDS if k not in out]
    if missing:
        hint = " (advantages / returns exist only in a rollout collected with gamma=...)" if set(missing) & {"advantages", "returns"} else ""
        raise ValueError(f"the rollout has no {', '.join(repr(k) for k in missing)}{hint}")
    obs = out["obs"]
    if not torch.is_tensor(obs) or obs.dim() != 3 or obs.shape[2] != OBS_DIM or obs.shape[0] < 1 or obs.shape[1] < 1:
        raise ValueError(f"'obs' must be a [T, n, {OBS_DIM}] tensor with T, n >= 1, got {tuple(obs.shape) if torch.is_tensor(obs) else type(obs).__name__}")
    T, n = int(obs.shape[0]), int(obs.shape[1])
    if T * n > MAX_ROWS:
        raise ValueError(f"{T} x {n} = {T * n} rows; at most 2^24 - 16 = {MAX_ROWS}")
    device = obs.device if device is None else device
    tensors = []
    for key, tail, _ in FIELDS:
        x = out[key]
        if not torch.is_tensor(x):
            raise ValueError(f"{key!r} is a {type(x).__name__}, not a tensor")
        if x.dtype != torch.float32:
            raise ValueError(f"{key!r} is {str(x.dtype).replace('torch.', '')}, not float32")
        if tuple(x.shape) != (T, n) + tail:
            raise ValueError(f"{key!r} has shape {tuple(x.shape)}, not {(T, n) + tail} (T, n from 'obs')")
        if not x.is_contiguous():
            raise ValueError(f"{key!r} is not contiguous")
        if x.device != device:
            raise ValueError(f"{key!r} is on {x.device}, not on {device}")
        tensors.append(x)
    return T, n, tensors


def minibatch_bounds(rows: int, batch_size: Optional[int]) -> List[Tuple[int, int]]:
    """[(a, b)] of SB3's ``while start_idx < rows`` loop: ``batch_size`` None is one minibatch of all rows, and a last
    minibatch shorter than ``batch_size`` is kept."""
    if batch_size is None:
        batch_size = rows
    if isinstance(batch_size, bool) or not isinstance(batch_size, int) or batch_size < 1:
        raise ValueError(f"batch_size must be a positive int or None, got {batch_size!r}")
    return [(a, min(a + batch_size, rows)) for a in range(0, rows, batch_size)]


def check_perm(perm, rows: int, check: bool = False):
    """``perm`` as ``get`` takes it: an int32 or int64 tensor of ``rows`` indices, contiguous, on any device.  ``check``: every
    index lies in [0, rows) (reads the tensor: a synchronisation when it is on the GPU)."""
    import torch
    if not torch.is_tensor(perm):
        raise ValueError(f"perm must be an int32 or int64 tensor, got {type(perm).__name__}")
    if perm.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"perm is {str(perm.dtype).replace('torch.', '')}, not int32 or int64")
    if tuple(perm.shape) != (rows,):
        raise ValueError(f"perm has shape {tuple(perm.shape)}, not ({rows},): one index per row of the rollout")
    if not perm.is_contiguous():
        raise ValueError("perm is not contiguous")
    if check:
        bad = (perm < 0) | (perm >= rows)
        if bool(bad.any()):
            j = int(bad.nonzero()[0])
            raise ValueError(f"perm[{j}] = {int(perm[j])} is not a row of the rollout (0 <= index < {rows})")
    return perm


class DeviceRolloutBuffer(Handle):
    """load(out), then get(batch_size) per epoch: one launch on the current stream, no synchronisation."""
    PREFIX = "meshenv_rollout"

    def __init__(self, device: int = 0):
        super().__init__(device)
        self._in = None               # the six tensors of the loaded rollout (references)
        self._out = None              # the six output buffers, allocated at the first get for a given number of rows
        self.T = self.n_envs = 0
        self.launches = 0             # k_rollout_gather launches so far: one per get

    @property
    def rows(self) -> int:
        return self.T * self.n_envs

    def load(self, out) -> None:
        """Take the histories of ``venv.collect_rollout(policy, T, gamma=..., gae_lambda=...)``: obs [T, n, 18], buffer_actions
        [T, n, 3], value, log_prob, advantages, returns [T, n], float32 and contiguous on this device.  Nothing is copied:
        they are read by every ``get`` and must stay as they are until the last one."""
        self.T, self.n_envs, self._in = check_rollout(out, self.device)

    def get(self, batch_size: Optional[int] = None, perm=None, check: bool = False):
        """The minibatches of one epoch: an iterator of ``RolloutBufferSamples`` whose fields are contiguous views into
        buffers this object owns, VALID UNTIL THE NEXT ``get``.  The one launch is made by this call, before the first
        minibatch is taken.

        batch_size  None: one minibatch of all rows (A2C).  A last, shorter minibatch is yielded, as SB3 does.
        perm        None: ``torch.randperm(rows)`` on the device.  Else an int32 or int64 tensor of ``rows`` indices into SB3's
                    flat order ``i = env * T + t``, on the device (used as it is) or on the host (copied).
        check       test a caller's ``perm`` for indices outside [0, rows) first and raise ValueError: a synchronisation, so it
                    is off by default.  Unchecked, such an index is never dereferenced: its row is NaN in every field."""
        t = self._torch
        if self._in is None:
            raise ValueError("get() before load()")
        rows = self.rows
        bounds = minibatch_bounds(rows, batch_size)
        if perm is None:
            perm = t.randperm(rows, device=self.device)
        else:
            perm = check_perm(perm, rows, check)
            if perm.device != self.device:
                perm = perm.to(self.device)
        o = self._outputs()
        self._gather(perm, 0)
        return (RolloutBufferSamples(*[x[a:b] for x in o]) for a, b in bounds)

    def _outputs(self) -> list:
        """The six output buffers for the loaded rollout: allocated at the first use for a given number of rows."""
        t, rows = self._torch, self.rows
        if self._out is None or self._out[0].shape[0] != rows:
            self._out = [t.empty((rows,) + tail, dtype=t.float32, device=self.device) for _, tail, _ in FIELDS]
        return self._out

    def _gather(self, perm, variant: int) -> None:
        self._bind_stream()
        rc = self._L.meshenv_rollout_gather(self._h, self.T, self.n_envs, perm.data_ptr(), perm.element_size(), self._ptrs(self._in),
                                            self._ptrs(self._out), variant)
        self._check(rc, "meshenv_rollout_gather")
        self.launches += 1
