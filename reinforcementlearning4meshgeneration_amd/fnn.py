"""The supervised element-extraction network of the reference ("FNN mesher", general/EBRD.py: ``Policy`` :85-126,
``get_action`` :174-177) on the GPU (include/meshenv_fnn.h, csrc/meshenv_fnn.h): observation -> (new point, rule type) in
one launch, and -- through ``MeshVecEnv.mesh_with`` -- the meshing loop of EBRD.py:525-548 for every env of a batch without a
host round trip per move.  This module is the inference half; the training of the network (EBRD.py ``train_ch3``) is
``fnn_train.FusedFNNTrain``, whose stepped parameters reach a loaded ``FusedFNN`` through ``bind_live`` + ``refresh`` without
leaving the device.  No trained weights ship with this package because the reference holds no weights file.

``FNNSpec`` is the host half (the fourteen tensors as float32 arrays, their packed form; no device needed); ``FusedFNN``
loads one on a GPU."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, Optional

import numpy as np

from . import _capi
from ._handle import Handle

# (name, rows, columns) of the seven torch.nn.Linear layers, in the order of MESHENV_FNN_TENSORS
LAYERS = (("fc1", 64, 18), ("fc2", 128, 64), ("fc3", 64, 128), ("fc4", 32, 64), ("fc5", 16, 32), ("action_head", 2, 16),
          ("type_head", 3, 16))
SUPPORTED = ("fc1 [64, 18], fc2 [128, 64], fc3 [64, 128], fc4 [32, 64], fc5 [16, 32], action_head [2, 16], type_head [3, 16], "
             "each with a bias, ReLU between them (general/EBRD.py Policy)")
PACKED_FLOATS = 21568


def live_parameters(module):
    """The fourteen LIVE parameter tensors of a Policy-shaped torch module, in MESHENV_FNN_TENSORS' order: float32, contiguous,
    of exactly the shapes of LAYERS.  ValueError names what is wrong and what is supported."""
    import torch
    params = []
    for name, rows, cols in LAYERS:
        layer = getattr(module, name, None)
        if layer is None or getattr(layer, "weight", None) is None or getattr(layer, "bias", None) is None:
            raise ValueError(f"the module has no layer {name!r} with a weight and a bias; supported: {SUPPORTED}")
        for part, p, shape in (("weight", layer.weight, (rows, cols)), ("bias", layer.bias, (rows,))):
            if not torch.is_tensor(p) or tuple(p.shape) != shape:
                raise ValueError(f"{name}.{part} has shape {tuple(getattr(p, 'shape', ()))}, expected {shape}; supported: {SUPPORTED}")
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise ValueError(f"{name}.{part} is {str(p.dtype).replace('torch.', '')}{'' if p.is_contiguous() else ', not contiguous'}; "
                                 "the live tensors must be float32 and contiguous")
            params.append(p)
    return params


def _np(x, what):
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32))


@dataclass
class FNNSpec:
    """The weights of one network: ``weights['fc1.weight']`` ... ``weights['type_head.bias']``, float32, torch layout."""
    weights: Dict[str, np.ndarray]

    @classmethod
    def from_state_dict(cls, sd) -> "FNNSpec":
        """sd: what ``torch.save(model.state_dict())`` of EBRD.py:320 holds (tensors or arrays under 'fc1.weight' ...
        'type_head.bias').  ValueError on a missing key or any other shape."""
        w = {}
        for name, rows, cols in LAYERS:
            for part, shape in (("weight", (rows, cols)), ("bias", (rows,))):
                key = f"{name}.{part}"
                if key not in sd:
                    raise ValueError(f"state dict has no {key!r}; supported: {SUPPORTED}")
                a = _np(sd[key], key)
                if a.shape != shape:
                    raise ValueError(f"{key} has shape {tuple(a.shape)}, expected {shape}; supported: {SUPPORTED}")
                w[key] = a
        return cls(w)

    @classmethod
    def from_module(cls, module) -> "FNNSpec":
        """Any module with ``fc1`` .. ``fc5``, ``action_head`` and ``type_head`` (``.weight [out][in]``, ``.bias``)."""
        sd = {}
        for name, _, _ in LAYERS:
            layer = getattr(module, name, None)
            if layer is None or getattr(layer, "weight", None) is None or getattr(layer, "bias", None) is None:
                raise ValueError(f"the module has no layer {name!r} with a weight and a bias; supported: {SUPPORTED}")
            sd[f"{name}.weight"], sd[f"{name}.bias"] = layer.weight, layer.bias
        return cls.from_state_dict(sd)

    def load_args(self):
        """(tensor pointers, shapes) as meshenv_fnn_pack / meshenv_fnn_load take them (the arrays stay referenced by self)."""
        ptrs, shapes = [], []
        for name, rows, cols in LAYERS:
            ptrs += [self.weights[f"{name}.weight"].ctypes.data, self.weights[f"{name}.bias"].ctypes.data]
            shapes += [rows, cols, rows, 1]
        return (C.c_void_p * len(ptrs))(*ptrs), np.ascontiguousarray(shapes, np.int32)

    def packed(self) -> np.ndarray:
        """The buffer the kernel reads (meshenv_fnn_pack; include/meshenv_fnn.h states the layout).  Needs no GPU."""
        L = _capi.load()
        out = np.empty(PACKED_FLOATS, np.float32)
        ptrs, shapes = self.load_args()
        rc = L.meshenv_fnn_pack(ptrs, shapes.ctypes.data, out.ctypes.data)
        if rc != 0:
            msg = L.meshenv_fnn_last_error(None)
            raise ValueError(f"meshenv_fnn_pack failed ({rc}): {msg.decode() if msg else ''}")
        return out


@dataclass
class FNNMeshResult:
    """What ``MeshVecEnv.mesh_with`` returns; CUDA tensors over the envs.  steps: moves made, the finishing one included;
    done / complete / code: those of each env's last move (``_capi.MOVE_*``); finished: done or code >= MOVE_RAISES;
    n_elements: elements of the env's mesh.  With record=True the histories [T, n, ...] of the steps that ran (T = total_steps):
    points, types, obs (the observation each forward read), step_code, step_done, step_complete; the rows of an env behind its
    last move hold code 255 and zeros."""
    steps: object
    done: object
    complete: object
    code: object
    finished: object
    n_elements: object
    total_steps: int = 0
    points: Optional[object] = None
    types: Optional[object] = None
    obs: Optional[object] = None
    step_code: Optional[object] = None
    step_done: Optional[object] = None
    step_complete: Optional[object] = None

    @property
    def complete_rate(self) -> float:
        return float(self.complete.float().mean().item())


class FusedFNN(Handle):
    """An FNNSpec loaded on one GPU."""
    PREFIX = "meshenv_fnn"

    def __init__(self, spec: FNNSpec, device: int = 0):
        self.spec = spec
        super().__init__(device)
        ptrs, shapes = spec.load_args()
        self._check(self._L.meshenv_fnn_load(self._h, ptrs, shapes.ctypes.data), "meshenv_fnn_load")

    @classmethod
    def from_module(cls, policy_module, device: int = 0):
        return cls(FNNSpec.from_module(policy_module), device)

    @classmethod
    def from_state_dict(cls, sd, device: int = 0):
        return cls(FNNSpec.from_state_dict(sd), device)

    def bind_live(self, policy_module) -> None:
        """Record the LIVE parameters of ``policy_module`` (the module an optimiser steps, on this device) so that refresh() can
        carry them into this object's packed weights.  Again after anything that reallocates the parameters (``.to()``)."""
        from .sb3_nets import check_device
        params = live_parameters(policy_module)
        check_device(params, self.device, "FusedFNN.bind_live")
        self._check(self._L.meshenv_fnn_bind(self._h, self._ptrs(params)), "meshenv_fnn_bind")
        self._live = params      # keeps the storages alive

    def refresh(self) -> None:
        """The bound parameters, as they are now, into the packed weights, in exactly the layout ``FNNSpec.packed`` builds on the
        host: one launch on the current stream, no host copy, no synchronisation.  Launches that follow on the same stream
        (forward, mesh_with) see the new weights."""
        if getattr(self, "_live", None) is None:
            raise ValueError("refresh() needs bind_live(policy) first")
        self._bind_stream()
        self._check(self._L.meshenv_fnn_refresh(self._h), "meshenv_fnn_refresh")

    def forward(self, obs, finished=None, raw: bool = False):
        """obs float32 CUDA [n, 18] (the static observation; a row of zeros is the reference's None).  Returns (points [n, 2]
        float64, types [n] float64 in {0, 0.5, 1}): what EBRD.get_action hands to env.move, for a batch.  raw=True adds the
        heads' float32 outputs: (points, types, actions [n, 2], logits [n, 3]).  finished: optional uint8 [n]; rows where it is
        nonzero come back as zeros."""
        t = self._torch
        if obs.dim() != 2 or obs.shape[1] != _capi.OBS_DIM or obs.shape[0] == 0:
            raise ValueError(f"obs must have shape (n, {_capi.OBS_DIM}), got {tuple(obs.shape)}")
        n = obs.shape[0]
        obs = self._f32(obs, "obs", [(n, _capi.OBS_DIM)])
        fptr = None
        if finished is not None:
            finished = finished.to(device=self.device, dtype=t.uint8).contiguous()
            if tuple(finished.shape) != (n,):
                raise ValueError(f"finished must have shape ({n},), got {tuple(finished.shape)}")
            fptr = finished.data_ptr()
        points = t.empty((n, 2), dtype=t.float64, device=self.device)
        types = t.empty(n, dtype=t.float64, device=self.device)
        actions = t.empty((n, 2), dtype=t.float32, device=self.device) if raw else None
        logits = t.empty((n, 3), dtype=t.float32, device=self.device) if raw else None
        self._bind_stream()
        rc = self._L.meshenv_fnn_forward(self._h, n, obs.data_ptr(), fptr, points.data_ptr(), types.data_ptr(),
                                         actions.data_ptr() if raw else None, logits.data_ptr() if raw else None)
        self._check(rc, "meshenv_fnn_forward")
        return (points, types, actions, logits) if raw else (points, types)

    get_action = forward      # EBRD.get_action(state, model), for a batch
