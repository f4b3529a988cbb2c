"""The synthetic training samples of the supervised mesher, generated on the device: ``MeshAugmentation.sampling`` /
``sampling_main`` of the reference's general/data_augmentation.py (``data_sampling`` of general/EBRD.py) as the kernels of
csrc/meshenv_augment.h (include/meshenv_augment.h).

    aug = DeviceMeshAugmentation()
    x, y = aug.sampling(40000, 0.7, pool=10)      # sampling_main(10, 40000, 0.7): x [39710, 18], y [39710, 3] on the device
    FusedFNNTrain(policy, opt, fnn=fnn).fit(x, y, num_epochs=...)
"""
from __future__ import annotations

import ctypes as C
import json
import math
from typing import NamedTuple

import numpy as np

from . import _capi
from ._handle import Handle

TYPES = (0.5, 0.0, 1.0)        # type index 0, 1, 2: the order sampling() concatenates
FRACTIONS = (0.5, 0.25, 0.25)
BIN_KEYS = (0.4, 0.6, 0.8, 1.0, 1.2, 1.4, 1.6, 1.8, 2.0, 2.2, 2.4)
STATS = ("proposals", "candidates", "rows", "rounds")


class AugmentScore(NamedTuple):
    """``DeviceMeshAugmentation.score``: per candidate, on the device.  ``accept`` is None without a threshold."""
    obs_rejected: object   # bool [B]: check_obs_quality
    valid: object          # bool [B]: the element passed is_valid, check_intersection and check_internal_element
    ele: object            # float64 [B]: Mesh.get_quality('strong'), 0 for an invalid element
    boundary: object       # float64 [B]: compute_boundary_quality, 0 for an invalid element
    max_ele: object        # float64 [B]: estimate_max_quality(method=3)
    max_boundary: object
    accept: object         # bool [B] or None


def rows_per_bin(n, pool=1):
    """Rows each bin of type 0.5, 0, 1 yields: Q - 1 with Q = ceil(frac * (n / pool) / 11) (the reference counts an accepted
    candidate before it appends it and leaves at the quota)."""
    return tuple(max(math.ceil(f * (n / pool) / 11) - 1, 0) for f in FRACTIONS)


def row_count(n, pool=1):
    """Rows of ``sampling(n, ..., pool=pool)``: 407 for (440, 1), 39 710 for (40 000, 10)."""
    return pool * _capi.AUGMENT_BINS * sum(rows_per_bin(n, pool))


def check_sampling_args(n, threshold, pool, round_size, max_rounds, dtype):
    """The refusals of ``sampling`` (ValueError / TypeError), made before anything is enqueued."""
    import torch
    for name, v in (("n", n), ("pool", pool), ("round_size", round_size), ("max_rounds", max_rounds)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
            raise TypeError(f"sampling: {name} must be an int, got {type(v).__name__}")
    if n < 0 or n > 2 ** 40:
        raise ValueError(f"sampling: n must be in [0, 2^40], got {n}")
    if not 1 <= pool <= _capi.AUGMENT_MAX_POOL:
        raise ValueError(f"sampling: pool must be in [1, {_capi.AUGMENT_MAX_POOL}], got {pool}")
    check_threshold("sampling", threshold)
    if not 64 <= round_size <= _capi.AUGMENT_MAX_ROUND or round_size % 64:
        raise ValueError(f"sampling: round_size must be a multiple of 64 in [64, {_capi.AUGMENT_MAX_ROUND}], got {round_size}")
    if not 1 <= max_rounds <= _capi.AUGMENT_MAX_ROUNDS:
        raise ValueError(f"sampling: max_rounds must be in [1, {_capi.AUGMENT_MAX_ROUNDS}], got {max_rounds}")
    if dtype not in (torch.float32, torch.float64):
        raise TypeError(f"sampling: dtype must be torch.float32 or torch.float64, got {dtype}")


def check_threshold(what, threshold):
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float, np.floating, np.integer)):
        raise TypeError(f"{what}: threshold must be a number, got {type(threshold).__name__}")
    if not 0.0 < float(threshold) <= 1.0:      # NaN included
        raise ValueError(f"{what}: threshold must be in (0, 1], got {threshold}")


def check_score_args(obs, act, threshold=None):
    """The refusals of ``score``: float64 tensors [B, 18] and [B, 3] with the same B."""
    import torch
    for name, v, cols in (("obs", obs, _capi.OBS_DIM), ("act", act, _capi.ACT_DIM)):
        if not isinstance(v, torch.Tensor):
            raise TypeError(f"score: {name} must be a torch tensor, got {type(v).__name__}")
        if v.dtype != torch.float64:
            raise TypeError(f"score: {name} must be float64, got {v.dtype}")
        if v.ndim != 2 or v.shape[1] != cols:
            raise ValueError(f"score: {name} must have shape [B, {cols}], got {tuple(v.shape)}")
    if obs.shape[0] != act.shape[0]:
        raise ValueError(f"score: obs has {obs.shape[0]} rows, act {act.shape[0]}")
    if obs.shape[0] > 2 ** 24:
        raise ValueError("score: at most 2^24 rows a call")
    if threshold is not None:
        check_threshold("score", threshold)


def check_propose_args(uniforms, t_index, b_index):
    """The refusals of ``propose``: float64 [B, 57], and [B] type indices in 0..2 and bins in 0..10 (host arrays)."""
    import torch
    if not isinstance(uniforms, torch.Tensor) or uniforms.dtype != torch.float64:
        raise TypeError("propose: uniforms must be a float64 torch tensor")
    if uniforms.ndim != 2 or uniforms.shape[1] != _capi.AUGMENT_UNIFORMS:
        raise ValueError(f"propose: uniforms must have shape [B, {_capi.AUGMENT_UNIFORMS}], got {tuple(uniforms.shape)}")
    t, b = np.asarray(t_index), np.asarray(b_index)
    if t.dtype.kind not in "iu" or b.dtype.kind not in "iu":
        raise TypeError("propose: t_index and b_index must be integer arrays")
    if t.shape != (uniforms.shape[0],) or b.shape != t.shape:
        raise ValueError(f"propose: t_index and b_index must have shape [{uniforms.shape[0]}]")
    if t.size and (t.min() < 0 or t.max() >= _capi.AUGMENT_TYPES or b.min() < 0 or b.max() >= _capi.AUGMENT_BINS):
        raise ValueError("propose: type indices are 0..2 (types 0.5, 0, 1), bins 0..10")
    return np.ascontiguousarray(t, np.int32), np.ascontiguousarray(b, np.int32)


def save_json(path, x, y):
    """Write (x [R, 18], y [R, 3]) in the reference's three-key format, the one ``load_training_data`` reads and
    ``build_training_data`` turns back into x and y = (type, out0, out1)."""
    x, y = _to_numpy(x), _to_numpy(y)
    if x.ndim != 2 or x.shape[1] != _capi.OBS_DIM or y.shape != (x.shape[0], 3):
        raise ValueError(f"save_json: x [R, 18] and y [R, 3], got {x.shape} and {y.shape}")
    data = {"samples": x.tolist(), "output_types": y[:, 0:1].tolist(), "outputs": y[:, 1:].tolist()}
    with open(path, "w") as f:
        json.dump(data, f)


def load_json(path):
    """(x [R, 18], y [R, 3]) float64 numpy arrays of a file in the reference's three-key format."""
    with open(path) as f:
        data = json.load(f)
    x = np.asarray(data["samples"], np.float64).reshape(-1, _capi.OBS_DIM)
    y = np.concatenate([np.asarray(data["output_types"], np.float64).reshape(-1, 1),
                        np.asarray(data["outputs"], np.float64).reshape(-1, 2)], axis=1)
    if len(x) != len(y):
        raise ValueError(f"load_json: {len(x)} samples and {len(y)} outputs")
    return x, y


def _to_numpy(a):
    if hasattr(a, "detach"):
        a = a.detach().cpu().numpy()
    return np.asarray(a, np.float64)


class DeviceMeshAugmentation(Handle):
    """``MeshAugmentation`` on one GPU: ``sampling``, ``score``, ``propose``.  ``stream``: a ``torch.cuda.Stream`` every launch
    goes to; None: torch's current stream of the device at each call."""
    PREFIX = "meshenv_augment"
    save_json = staticmethod(save_json)
    load_json = staticmethod(load_json)

    def __init__(self, device=None, stream=None):
        import torch
        if device is None:
            device = torch.cuda.current_device() if torch.cuda.is_available() else 0
        elif not isinstance(device, int):
            device = torch.device(device).index or 0
        self._user_stream = stream
        super().__init__(int(device))
        self.last_stats = None      # dict of STATS after a sampling() call
        self.last_counts = None     # int32 [pool, 3, 11]: rows written per bin

    def _bind_stream(self):
        if self._user_stream is None:
            return super()._bind_stream()
        stream = self._user_stream.cuda_stream
        if stream != self._stream:
            self._check(self._set_stream(self._h, C.c_void_p(stream)), self.PREFIX + "_set_stream")
            self._stream = stream

    def _torch_stream(self):
        t = self._torch
        return self._user_stream if self._user_stream is not None else t.cuda.current_stream(self.device)

    # ---------------------------------------------------------------- public
    def sampling(self, n, threshold, *, seed=0, pool=1, round_size=8192, max_rounds=512, dtype=None):
        """``sampling_main(pool, n, threshold)`` (pool = 1: ``MeshAugmentation.sampling(n, threshold)``): device tensors
        x [R, 18] and y [R, 3] = (type, out0, out1) of ``dtype`` (float32 by default, what ``FusedFNNTrain.fit`` takes;
        float64 is the unrounded result), R = ``row_count(n, pool)``.  The rows are a function of (n, threshold, seed, pool)
        alone.  A round draws 33 * pool * round_size proposals, shared among the bins that are still short (round_size each
        at first, more as bins finish).  RuntimeError naming the short bins when max_rounds rounds do not fill every bin; the
        handle stays usable."""
        t = self._torch
        dtype = t.float32 if dtype is None else dtype
        check_sampling_args(n, threshold, pool, round_size, max_rounds, dtype)
        if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not 0 <= seed < 2 ** 64:
            raise ValueError(f"sampling: seed must be an int in [0, 2^64), got {seed!r}")
        R = row_count(n, pool)
        with t.cuda.stream(self._torch_stream()):
            x = t.empty((R, _capi.OBS_DIM), dtype=dtype, device=self.device)
            y = t.empty((R, _capi.ACT_DIM), dtype=dtype, device=self.device)
        G = pool * _capi.AUGMENT_TYPES * _capi.AUGMENT_BINS
        counts = np.zeros(G, np.int32)
        stats = np.zeros(_capi.AUGMENT_STATS, np.uint64)
        if R == 0:                       # nothing owed (n / pool <= 22): no launch; an empty tensor has no storage to point at
            self.last_stats = dict.fromkeys(STATS, 0)
            self.last_counts = counts.reshape(pool, _capi.AUGMENT_TYPES, _capi.AUGMENT_BINS)
            return x, y
        ptrs = (x.data_ptr(), y.data_ptr(), None, None) if dtype == t.float64 else (None, None, x.data_ptr(), y.data_ptr())
        self._bind_stream()
        rc = self._L.meshenv_augment_sample(self._h, int(n), float(threshold), int(seed), int(pool), int(round_size), int(max_rounds),
                                            R, *ptrs, counts.ctypes.data, stats.ctypes.data)
        self.last_stats = dict(zip(STATS, (int(v) for v in stats)))
        self.last_counts = counts.reshape(pool, _capi.AUGMENT_TYPES, _capi.AUGMENT_BINS)
        if rc == _capi.E_RANGE:
            owed = rows_per_bin(n, pool)
            short = [f"(worker {w}, type {TYPES[k]}, bin {BIN_KEYS[b]}): {int(self.last_counts[w, k, b])} of {owed[k]}"
                     for w in range(pool) for k in range(3) for b in range(_capi.AUGMENT_BINS) if self.last_counts[w, k, b] < owed[k]]
            raise RuntimeError(f"sampling(n={n}, threshold={threshold}): {len(short)} bins are short after {max_rounds} rounds of "
                               f"{G} x {round_size} proposals: " + "; ".join(short[:12]) + (" ..." if len(short) > 12 else ""))
        self._check(rc, "meshenv_augment_sample")
        return x, y

    def score(self, obs, act, threshold=None) -> AugmentScore:
        """``compute_quality`` and ``estimate_max_quality(method=3)`` of B candidates (obs [B, 18], act [B, 3] float64), the
        observation check, and with a threshold the accept decision of ``sampling_4_type``."""
        t = self._torch
        check_score_args(obs, act, threshold)
        obs = obs.detach().to(self.device).contiguous()
        act = act.detach().to(self.device).contiguous()
        B = obs.shape[0]                 # (B = 0: nothing is launched; an empty tensor has no storage to point at)
        with t.cuda.stream(self._torch_stream()):
            flags = t.zeros((3, B), dtype=t.uint8, device=self.device)
            q = t.zeros((B, 4), dtype=t.float64, device=self.device)
        self._bind_stream()
        rc = 0 if B == 0 else self._L.meshenv_augment_score(self._h, B, obs.data_ptr(), act.data_ptr(), 0.0 if threshold is None else float(threshold),
                                           flags[0].data_ptr(), flags[1].data_ptr(), q.data_ptr(),
                                           None if threshold is None else flags[2].data_ptr())
        self._check(rc, "meshenv_augment_score")
        with t.cuda.stream(self._torch_stream()):
            return AugmentScore(flags[0].bool(), flags[1].bool(), q[:, 0], q[:, 1], q[:, 2], q[:, 3],
                                None if threshold is None else flags[2].bool())

    def propose(self, uniforms, t_index, b_index):
        """The proposal maps on recorded uniforms [B, 57] float64 (draw order; types 0 and 1 read the first 17): returns
        (angle [B], obs [B, 18], actions [B, 20, 3], obs_rejected [B]) on the device; action rows past the type's count (20 for
        type index 0, else 1) are zero."""
        t = self._torch
        t_host, b_host = check_propose_args(uniforms, t_index, b_index)
        uniforms = uniforms.detach().to(self.device).contiguous()
        B = uniforms.shape[0]
        with t.cuda.stream(self._torch_stream()):
            t_dev, b_dev = t.from_numpy(t_host).to(self.device), t.from_numpy(b_host).to(self.device)
            angle = t.zeros(B, dtype=t.float64, device=self.device)
            obs = t.zeros((B, _capi.OBS_DIM), dtype=t.float64, device=self.device)
            acts = t.zeros((B, _capi.AUGMENT_MAX_ACTIONS, 3), dtype=t.float64, device=self.device)
            rej = t.zeros(B, dtype=t.uint8, device=self.device)
        self._bind_stream()
        rc = 0 if B == 0 else self._L.meshenv_augment_propose(self._h, B, uniforms.data_ptr(), t_dev.data_ptr(), b_dev.data_ptr(), t_host.ctypes.data,
                                             b_host.ctypes.data, angle.data_ptr(), obs.data_ptr(), acts.data_ptr(), rej.data_ptr())
        self._check(rc, "meshenv_augment_propose")
        with t.cuda.stream(self._torch_stream()):
            return angle, obs, acts, rej.bool()
