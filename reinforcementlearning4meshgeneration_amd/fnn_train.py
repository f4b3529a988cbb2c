"""Training the supervised element-extraction network of the reference on the GPU (include/meshenv_fnn_train.h,
csrc/meshenv_fnn_grad.h): the statement of general/EBRD.py's ``train_ch3`` (:272-320) that runs once per minibatch,

    action, logits = model(x)                                                    # Policy, x [B, 18]
    loss = CrossEntropyLoss(reduction='sum')(logits, cls) + MSELoss(reduction='sum')(action, y[:, 1:])
    optimizer.zero_grad(); loss.backward(); optimizer.step()

with ``y [B, 3] = (type, out0, out1)`` and ``cls = 2 type`` for ``type`` in {0, 0.5, 1} (``map_type_to_tensors``).
``FusedFNNTrain.backward`` is two launches and leaves the gradients in ``p.grad`` of the 14 LIVE parameters (views into one
flat buffer the object owns, OVERWRITTEN by every call); ``step()`` is the existing one-launch Adam of ``FusedOptimStep``;
``fit`` is the loop of ``train_ch3`` with nothing read back between entering and returning, and ends with one ``refresh()``
of the bound ``FusedFNN`` so that ``MeshVecEnv.mesh_with`` meshes with the trained weights (examples/fnn_training.py).

The samples are what ``MeshVecEnv.extract_samples(n_neighbor=3, n_radius=3)`` returns: 18 input columns and 3 output columns.

``FNNTrainSpec`` is the host half (the parameter tensors, the permutations and every refusal; no device needed)."""
from __future__ import annotations

import weakref
from typing import List

import numpy as np

from . import _capi
from ._handle import GradBuffer, Handle
from .fnn import LAYERS, SUPPORTED, live_parameters
from .optim_step import FusedOptimStep, OptimStepSpec
from .sb3_nets import check_device

OBS_DIM, OUT_DIM = _capi.OBS_DIM, 3
TYPES = (0.0, 0.5, 1.0)             # the rule types; the class of a row is 2 * type
OUTPUTS = ("loss", "classification_loss", "regression_loss", "hits")


def _is_tensor(a) -> bool:
    return hasattr(a, "detach") and hasattr(a, "data_ptr")


class FNNTrainSpec:
    """The module whose 14 parameters are trained and the ``torch.optim.Adam`` that steps exactly those."""

    def __init__(self, policy_module, optimizer):
        self.module = policy_module
        self.params = live_parameters(policy_module)      # ValueError for any other architecture
        import torch
        if type(optimizer) is not torch.optim.Adam:
            raise ValueError(f"the optimiser is {type(optimizer).__module__}.{type(optimizer).__name__}; train_ch3 steps a "
                             "torch.optim.Adam, and no other optimiser is supported here")
        self.optim = OptimStepSpec.on_policy(optimizer)   # ValueError for anything but a plain Adam
        stepped = [id(p) for p in optimizer.param_groups[0]["params"]]
        if sorted(stepped) != sorted(id(p) for p in self.params):
            raise ValueError(f"the optimiser steps {len(stepped)} tensors that are not exactly the 14 parameters of the module "
                             f"({SUPPORTED})")

    # ---------------------------------------------------------------- the flat gradient buffer
    @property
    def n_grad(self) -> int:
        """Floats in the gradient buffer: the 14 parameters in order, padded to a multiple of 64."""
        return (sum(int(p.numel()) for p in self.params) + 63) // 64 * 64

    def offsets(self):
        out, at = [], 0
        for p in self.params:
            out.append((p, at))
            at += int(p.numel())
        return out

    def check_device(self, device) -> None:
        check_device(self.params, device, "FusedFNNTrain")

    # ---------------------------------------------------------------- refusals of the data (numpy arrays or torch tensors)
    @staticmethod
    def check_shapes(x, y, rows=None):
        """(N, n): rows of the data set and of the minibatch."""
        if len(x.shape) != 2 or x.shape[1] != OBS_DIM or x.shape[0] == 0:
            raise ValueError(f"x must have shape (N, {OBS_DIM}), got {tuple(x.shape)}")
        N = int(x.shape[0])
        if tuple(y.shape) != (N, OUT_DIM):
            raise ValueError(f"y must have shape ({N}, {OUT_DIM}) = (type, out0, out1) per row of x, got {tuple(y.shape)}")
        if N > 2 ** 24:
            raise ValueError(f"at most 2^24 rows, got {N}")
        if rows is None:
            return N, N
        if len(rows.shape) != 1 or rows.shape[0] == 0:
            raise ValueError(f"rows must have shape (B,) with B > 0, got {tuple(rows.shape)}")
        if rows.shape[0] > 2 ** 24:
            raise ValueError(f"at most 2^24 rows in a minibatch, got {rows.shape[0]}")
        kind = str(rows.dtype).replace("torch.", "")
        if kind not in ("int32", "int64"):
            raise ValueError(f"rows must be int32 or int64 indices, got {kind}")
        return N, int(rows.shape[0])

    @staticmethod
    def check_labels(y) -> None:
        """Every y[:, 0] is 0, 0.5 or 1 (map_type_to_tensors has no class for anything else).  One pass; on a CUDA tensor one
        read-back of a flag."""
        t = y[:, 0]
        ok = (t == TYPES[0]) | (t == TYPES[1]) | (t == TYPES[2])
        if bool(ok.all()):
            return
        bad = ~ok
        i = int(bad.nonzero()[0][0]) if _is_tensor(bad) else int(np.flatnonzero(bad)[0])
        raise ValueError(f"y[{i}, 0] = {float(t[i])!r} is not a rule type: the labels are 0, 0.5 and 1")

    @staticmethod
    def check_rows(rows, N: int) -> None:
        """Every index lies in [0, N)."""
        lo, hi = int(rows.min()), int(rows.max())
        if lo < 0 or hi >= N:
            raise ValueError(f"rows holds {lo if lo < 0 else hi}, outside [0, {N})")

    # ---------------------------------------------------------------- the loop of train_ch3, host side
    @staticmethod
    def permutations(N: int, num_epochs: int, seed: int = 0) -> np.ndarray:
        """[num_epochs, N] int32: epoch e's order is the e-th ``permutation(N)`` of ``numpy.random.default_rng(seed)``."""
        rng = np.random.default_rng(seed)
        return np.stack([rng.permutation(N) for _ in range(num_epochs)]).astype(np.int32)

    @staticmethod
    def minibatches(N: int, batch_size: int) -> List[tuple]:
        """[(first, last + 1)] of an epoch: DataLoader(batch_size, drop_last=False), the last one the short one."""
        if batch_size < 1:
            raise ValueError(f"batch_size must be >= 1, got {batch_size}")
        return [(a, min(a + batch_size, N)) for a in range(0, N, batch_size)]

    @staticmethod
    def check_perms(perms, num_epochs: int, N: int) -> None:
        if tuple(perms.shape) != (num_epochs, N):
            raise ValueError(f"perms must have shape ({num_epochs}, {N}): one order of the rows per epoch, got {tuple(perms.shape)}")


class FNNTrainLog:
    """What ``fit`` returns: per epoch the sums ``train_ch3`` prints (its ``sum_loss``) and the hit count, on the device."""

    def __init__(self, sums):
        self.sums = sums          # [E, 4] float32 CUDA: OUTPUTS per epoch, each summed over the epoch's rows

    def read(self) -> np.ndarray:
        """One copy of [E, 4] to the host (synchronises with the stream that trained)."""
        return self.sums.cpu().numpy()

    def columns(self) -> dict:
        a = self.read()
        return {k: a[:, i] for i, k in enumerate(OUTPUTS)}


class FusedFNNTrain(GradBuffer, Handle):
    """An FNNTrainSpec bound on one GPU: backward(), step(), fit(), save()."""
    PREFIX = "meshenv_fnn_grad"

    def __init__(self, policy_module, optimizer, fnn=None, device: int = 0):
        """fnn: a ``FusedFNN`` loaded from ``policy_module`` (``FusedFNN.from_module``); ``fit`` ends with its ``refresh()``.
        It is bound to the live parameters here unless ``bind_live`` was called already."""
        self.spec = FNNTrainSpec(policy_module, optimizer)
        super().__init__(device, check_device=self.spec.check_device)
        self._alloc_grads()
        self.bind()
        self.optim = FusedOptimStep(self.spec.optim, device)
        self.fnn = fnn
        if fnn is not None:
            if fnn.device != self.device:
                raise ValueError(f"the FusedFNN is on {fnn.device}, the trainer on {self.device}")
            if getattr(fnn, "_live", None) is None:
                fnn.bind_live(policy_module)
        self._labels_ok = None        # the y whose labels were checked last: (weak reference, version)

    def bind(self) -> None:
        """Record the parameters' device pointers again: after anything that reallocates them (``.to()``; optimisers and
        ``load_state_dict`` write in place and need no new bind)."""
        s = self.spec
        s.check_device(self.device)
        assert s.n_grad == _capi.FNN_GRAD_FLOATS and len(s.params) == _capi.FNN_TENSORS == 2 * len(LAYERS)
        rc = self._L.meshenv_fnn_grad_bind(self._h, self._ptrs(s.params), self.grad_buffer.data_ptr(), s.n_grad)
        self._check(rc, "meshenv_fnn_grad_bind")
        self._view_grads()

    # ---------------------------------------------------------------- public
    def _data(self, x, y, validate: bool):
        """x, y as float32 contiguous tensors on the device; the labels checked once per y."""
        t = self._torch
        if not _is_tensor(x):
            x = t.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
        if not _is_tensor(y):
            y = t.from_numpy(np.ascontiguousarray(y, dtype=np.float32))
        N, _ = FNNTrainSpec.check_shapes(x, y)
        if validate:
            seen = self._labels_ok
            if seen is None or seen[0]() is not y or seen[1] != y._version:
                self._labels_ok = None
                FNNTrainSpec.check_labels(y.detach())     # where y lives: a host array costs no device read
                self._labels_ok = (weakref.ref(y), y._version)
        x = self._f32(x, "x", [(N, OBS_DIM)])
        y = self._f32(y, "y", [(N, OUT_DIM)])
        return x, y, N

    def backward(self, x, y, rows=None, accum=None, validate: bool = True):
        """The loss of a minibatch and its gradients: two launches on the current stream, no synchronisation; no argument is
        written but ``accum``.

        x [N, 18], y [N, 3] float32; rows: None (the minibatch is all N rows) or an int32 / int64 tensor [B] of row indices
        (row i of the minibatch is ``x[rows[i]]``, ``y[rows[i]]``: no gather launch).  accum: None or a float32 CUDA tensor
        [4] to which the four outputs are added on the device.  validate: the labels of ``y`` (once per tensor) and the
        range of ``rows`` are checked before anything is enqueued -- on CUDA tensors that is a read-back; pass False for data
        checked before.  Returns a float32 CUDA tensor [4]: loss, classification_loss, regression_loss (sums over the rows) and
        hits, the rows whose argmax(logits) is the class."""
        t = self._torch
        x, y, N = self._data(x, y, validate)
        n = N
        if rows is not None:
            if not _is_tensor(rows):
                rows = t.from_numpy(np.ascontiguousarray(rows))
            _, n = FNNTrainSpec.check_shapes(x, y, rows)
            if validate:
                FNNTrainSpec.check_rows(rows, N)
            if rows.dtype != t.int32 or not rows.is_contiguous() or rows.device != self.device:
                rows = rows.to(device=self.device, dtype=t.int32).contiguous()
        if accum is not None:
            if (tuple(accum.shape) != (_capi.FNN_GRAD_OUTPUTS,) or accum.dtype != t.float32 or accum.device != self.device
                    or not accum.is_contiguous()):
                raise ValueError(f"accum must be a float32 contiguous tensor of shape ({_capi.FNN_GRAD_OUTPUTS},) on {self.device}")
        out = t.empty(_capi.FNN_GRAD_OUTPUTS, dtype=t.float32, device=self.device)
        self._attach()
        self._bind_stream()
        rc = self._L.meshenv_fnn_grad_backward(self._h, n, N, x.data_ptr(), y.data_ptr(), None if rows is None else rows.data_ptr(),
                                               out.data_ptr(), None if accum is None else accum.data_ptr())
        self._check(rc, "meshenv_fnn_grad_backward")
        return out

    def step(self) -> None:
        """``optimizer.step()`` on the gradients backward() left: one launch (k_optim_step)."""
        self.optim.policy_step()

    def fit(self, x, y, num_epochs: int, batch_size: int = 128, perms=None, seed: int = 0, validate: bool = True) -> FNNTrainLog:
        """``train_ch3``: ``num_epochs`` passes over the N rows in minibatches of ``batch_size`` (the last one of an epoch the
        short one), each a backward() and a step(); then one refresh() of the bound FusedFNN.  Epoch e visits the rows in the
        order ``perms[e]`` ([num_epochs, N] integers) or, without perms, ``FNNTrainSpec.permutations(N, num_epochs, seed)[e]``.
        The labels (and given perms) are checked once, on entry, before anything is enqueued (validate=False: not at all);
        from there to the return nothing is read back and nothing is synchronised.  Returns the log of per-epoch sums."""
        t = self._torch
        if num_epochs < 1:
            raise ValueError(f"num_epochs must be >= 1, got {num_epochs}")
        x, y, N = self._data(x, y, validate)
        batches = FNNTrainSpec.minibatches(N, int(batch_size))
        if perms is None:
            perms = FNNTrainSpec.permutations(N, num_epochs, seed)
        else:
            if not _is_tensor(perms):
                perms = np.ascontiguousarray(perms)
            FNNTrainSpec.check_perms(perms, num_epochs, N)
            if validate:
                FNNTrainSpec.check_rows(perms, N)
        if not _is_tensor(perms):
            perms = t.from_numpy(perms.astype(np.int32, copy=False))
        perms = perms.to(device=self.device, dtype=t.int32).contiguous()
        log = t.zeros((num_epochs, _capi.FNN_GRAD_OUTPUTS), dtype=t.float32, device=self.device)
        for e in range(num_epochs):
            for a, b in batches:
                self.backward(x, y, rows=perms[e, a:b], accum=log[e], validate=False)
                self.step()
        if self.fnn is not None:
            self.fnn.refresh()
        return FNNTrainLog(log)

    def save(self, path) -> None:
        """``torch.save(model.state_dict(), path)`` of EBRD.py:320: what ``FusedFNN.from_state_dict`` loads."""
        self._torch.save(self.spec.module.state_dict(), path)

    def close(self):
        optim = getattr(self, "optim", None)
        if optim is not None:
            optim.close()
        super().close()
