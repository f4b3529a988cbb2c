"""DeviceReplayBuffer: SB3 2.x's ReplayBuffer for SAC / TD3 with the transitions kept on the device (csrc/meshenv_replay.h).
The rollout calls (MeshVecEnv.step_actor_T, collect_rollout) leave their histories on the device; add_rollout stores T vector
steps of them in one launch and sample / gather hand back SB3's ReplayBufferSamples as CUDA tensors in one launch, so no
transition crosses to the host.  Host restatement of every rule: tests/replay_ref.py."""
from __future__ import annotations

import ctypes as C
from collections import namedtuple

import numpy as np

from . import _capi

OBS_DIM, ACT_DIM = _capi.OBS_DIM, _capi.ACT_DIM
_NEXT, _ACT, _REWARD, _DONE, _TIMEOUT = 18, 36, 39, 40, 41   # float offsets inside a record (csrc/meshenv_replay.h)

# stable_baselines3.common.type_aliases.ReplayBufferSamples: the same field names in the same order
ReplayBufferSamples = namedtuple("ReplayBufferSamples", ["observations", "actions", "next_observations", "dones", "rewards"])


class DeviceReplayBuffer:
    """SB3's ReplayBuffer(buffer_size, observation_space, action_space, device, n_envs, optimize_memory_usage=False,
    handle_timeout_termination=True) for the envs of `venv` (a MeshVecEnv / SB3MeshVecEnv), on the envs' device.

    rows = max(buffer_size // n_envs, 1) vector steps are kept (SB3 calls that number buffer_size too, and so does the
    attribute here).  The transitions live in one packed float32 tensor `store` [rows, n_envs, R]; observations,
    next_observations, actions, rewards, dones and timeouts are strided views of it with SB3's shapes.  pos, full and size()
    are SB3's."""

    def __init__(self, venv, buffer_size: int = 1_000_000, handle_timeout_termination: bool = True,
                 optimize_memory_usage: bool = False):
        if optimize_memory_usage:
            raise ValueError("optimize_memory_usage=True is not supported: next_observations are stored (SB3's default)")
        if int(buffer_size) < 1:
            raise ValueError(f"buffer_size must be positive, got {buffer_size}")
        t = venv._torch
        self._venv, self._torch, self._L = venv, t, venv._L
        self.n_envs = int(venv.num_envs)
        self.device = venv.device
        self.buffer_size = self.rows = max(int(buffer_size) // self.n_envs, 1)
        if self.rows > 2 ** 31 - 1:
            raise ValueError(f"{self.rows} rows exceed the int32 row index")
        self.handle_timeout_termination = bool(handle_timeout_termination)
        self.optimize_memory_usage = False
        self.record_floats = int(self._L.meshenv_replay_record_floats())
        self.store = t.zeros((self.rows, self.n_envs, self.record_floats), dtype=t.float32, device=self.device)
        s = self.store
        self.observations = s[:, :, :OBS_DIM]
        self.next_observations = s[:, :, _NEXT:_NEXT + OBS_DIM]
        self.actions = s[:, :, _ACT:_ACT + ACT_DIM]
        self.rewards, self.dones, self.timeouts = s[:, :, _REWARD], s[:, :, _DONE], s[:, :, _TIMEOUT]
        self.pos, self.full = 0, False

    def size(self) -> int:
        return self.rows if self.full else self.pos

    def reset(self) -> None:
        self.pos, self.full = 0, False

    # ------------------------------------------------------------------------------------------------ storing
    def _box(self, scale):
        """(low, high) float32 [3] for SAC's scale_action, or None."""
        if scale is None or scale is False:
            return None
        if scale is True:
            space = self._venv.action_space
            low, high = space.low, space.high
        else:
            low, high = scale
        low, high = np.asarray(low, np.float32).reshape(-1), np.asarray(high, np.float32).reshape(-1)
        if low.shape != (ACT_DIM,) or high.shape != (ACT_DIM,):
            raise ValueError(f"scale_actions needs (low, high) of {ACT_DIM} floats each")
        if not (np.isfinite(low).all() and np.isfinite(high).all() and (high > low).all()):
            raise ValueError("scale_actions needs finite bounds with high > low")
        return low, high

    def _want(self, name, x, shape, dtype):
        if not hasattr(x, "data_ptr") or x.dtype != dtype:
            raise ValueError(f"{name} must be a {dtype} tensor, got {getattr(x, 'dtype', type(x).__name__)}")
        if tuple(x.shape) != tuple(shape):
            raise ValueError(f"{name} has shape {tuple(x.shape)}, expected {tuple(shape)} (n_envs = {self.n_envs})")
        if x.device != self.device:
            raise ValueError(f"{name} is on {x.device}, the buffer on {self.device}")
        if not x.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
        return x

    def _add(self, T, obs0, obs_after, terminal_obs, actions, reward, done, complete, low_high):
        lh = None
        if low_high is not None:
            lh = (C.c_float * 6)(*low_high[0].tolist(), *low_high[1].tolist())
        self._venv._bind_stream()
        rc = self._L.meshenv_replay_add(self._venv._handle, T, obs0.data_ptr(), obs_after.data_ptr(), terminal_obs.data_ptr(),
                                        actions.data_ptr(), reward.data_ptr(), done.data_ptr(), complete.data_ptr(), lh,
                                        1 if self.handle_timeout_termination else 0, self.store.data_ptr(), self.rows, self.pos)
        _capi.check(self._venv._handle, rc, "meshenv_replay_add")
        self.full = self.full or self.pos + T >= self.rows
        self.pos = (self.pos + T) % self.rows

    def add_rollout(self, out, obs0=None, action_key=None, scale_actions=None) -> int:
        """Store the T vector steps of one rollout call: T x (OffPolicyAlgorithm._store_transition + ReplayBuffer.add), in
        ONE launch (the kernel wraps the row index itself; with T > rows only the last rows steps are written, as T
        sequential adds would leave).  `out` is the dict of

        * collect_rollout(policy, T) (the TD3 kind): its obs block holds what every step acted on and, one slice further,
          the observation after the last step; buffer_actions ([-1, 1] already) are stored as they are;
        * step_actor_T(actor, actions0, T, want_terminal_obs=True) (the fused SAC actor): obs[t] is the observation after
          step t, so `obs0`, the [n, 18] observation the first action was chosen on (env.obs before the call -- a copy, the
          call overwrites env.obs), is required; actions[:T] are Box actions and are scaled to [-1, 1] by the venv's action
          Box as SAC's policy.scale_action does.

        action_key names another [>= T, n, 3] entry to store; scale_actions overrides the scaling: False / None-for-default,
        True (the venv's Box) or (low, high).  Returns T."""
        t = self._torch
        if not isinstance(out, dict) or "done" not in out or "obs" not in out:
            raise ValueError("add_rollout takes the dict collect_rollout or step_actor_T returned")
        if "terminal_obs" not in out:
            raise ValueError("the rollout has no terminal_obs (step_actor_T needs want_terminal_obs=True): the next "
                             "observation of a finished episode would be the reset observation")
        n = self.n_envs
        done = out["done"]
        if not hasattr(done, "dim") or done.dim() != 2 or done.shape[0] < 1:
            raise ValueError("out['done'] must be a [T, n] tensor with T >= 1")
        T = int(done.shape[0])
        from_policy = "buffer_actions" in out
        if from_policy:
            if obs0 is not None:
                raise ValueError("obs0 belongs to a step_actor_T rollout; collect_rollout's obs block already holds it")
            obs = self._want("obs", out["obs"], (T, n, OBS_DIM), t.float32)
            after = out.get("obs_after")
            if after is None:
                # collect_rollout's obs is the first T slices of its [T + 1, n, 18] block: slice t + 1 is the observation after step t
                need = obs.storage_offset() + (T + 1) * n * OBS_DIM
                if obs.untyped_storage().nbytes() // 4 < need:
                    raise ValueError("out['obs'] is not collect_rollout's own block (no slice after the last step): pass the "
                                     "dict unchanged, or add obs_after [T, n, 18]")
                after = t.as_strided(obs, (T, n, OBS_DIM), (n * OBS_DIM, OBS_DIM, 1), obs.storage_offset() + n * OBS_DIM)
            first, key, default_scale = obs[0], "buffer_actions", False
        else:
            if obs0 is None:
                raise ValueError("a step_actor_T rollout needs obs0, the observation its first action was chosen on")
            first, after, key, default_scale = obs0, out["obs"], "actions", True
        key = action_key if action_key is not None else key
        if key not in out:
            raise ValueError(f"the rollout has no {key!r}")
        actions = out[key]
        if hasattr(actions, "dim") and actions.dim() == 3 and actions.shape[0] > T:
            actions = actions[:T]           # step_actor_T's [T + 1]: slice T is the next call's first action
        low_high = self._box(default_scale if scale_actions is None else scale_actions)
        self._add(T, self._want("obs0", first, (n, OBS_DIM), t.float32),
                  self._want("obs_after", after, (T, n, OBS_DIM), t.float32),
                  self._want("terminal_obs", out["terminal_obs"], (T, n, OBS_DIM), t.float32),
                  self._want(key, actions, (T, n, ACT_DIM), t.float32),
                  self._want("reward", out["reward"], (T, n), t.float64), self._want("done", done, (T, n), t.uint8),
                  self._want("complete", out["complete"], (T, n), t.uint8), low_high)
        return T

    def add(self, obs, next_obs, action, reward, done, infos) -> None:
        """SB3's ReplayBuffer.add(obs, next_obs, action, reward, done, infos) with numpy arrays, for a stock SB3 loop: one
        upload and the same kernel with T = 1.  next_obs already holds the terminal observation of finished envs
        (_store_transition put it there); timeouts come from infos[k].get("TimeLimit.truncated", False) on the envs that
        are done -- the only ones on which SB3MeshVecEnv sets it; on others the flag samples the same (dones is 0)."""
        t, n = self._torch, self.n_envs
        if len(infos) != n:
            raise ValueError(f"infos has {len(infos)} entries, expected {n}")
        try:
            o = np.ascontiguousarray(obs, np.float32).reshape(n, OBS_DIM)
            no = np.ascontiguousarray(next_obs, np.float32).reshape(n, OBS_DIM)
            a = np.ascontiguousarray(action, np.float32).reshape(n, ACT_DIM)
            r = np.ascontiguousarray(reward, np.float64).reshape(n)
            d = (np.asarray(done).reshape(n) != 0).astype(np.uint8)
        except (TypeError, ValueError) as exc:
            raise ValueError(f"add: {exc}") from None
        comp = np.array([0 if info.get("TimeLimit.truncated", False) else 1 for info in infos], np.uint8)
        up = lambda x: t.from_numpy(x).to(self.device)   # noqa: E731
        o, no, a, r, d, comp = up(o), up(no.reshape(1, n, OBS_DIM)), up(a.reshape(1, n, ACT_DIM)), up(r.reshape(1, n)), \
            up(d.reshape(1, n)), up(comp.reshape(1, n))
        self._add(1, o, no, no, a, r, d, comp, None)

    # ------------------------------------------------------------------------------------------------ sampling
    def _sample(self, batch, seed, counter, rows_in, envs_in, want_indices):
        t = self._torch
        f32 = dict(dtype=t.float32, device=self.device)
        out = ReplayBufferSamples(t.empty((batch, OBS_DIM), **f32), t.empty((batch, ACT_DIM), **f32),
                                  t.empty((batch, OBS_DIM), **f32), t.empty((batch, 1), **f32), t.empty((batch, 1), **f32))
        rows_out = envs_out = None
        if want_indices:
            rows_out = t.empty(batch, dtype=t.int32, device=self.device)
            envs_out = t.empty(batch, dtype=t.int32, device=self.device)
        self._venv._bind_stream()
        rc = self._L.meshenv_replay_sample(
            self._venv._handle, self.store.data_ptr(), self.rows, self.size(), batch, C.c_uint64(seed & (2 ** 64 - 1)),
            C.c_uint64(counter & (2 ** 64 - 1)), rows_in.data_ptr() if rows_in is not None else None,
            envs_in.data_ptr() if envs_in is not None else None, out.observations.data_ptr(), out.actions.data_ptr(),
            out.next_observations.data_ptr(), out.dones.data_ptr(), out.rewards.data_ptr(),
            rows_out.data_ptr() if want_indices else None, envs_out.data_ptr() if want_indices else None)
        _capi.check(self._venv._handle, rc, "meshenv_replay_sample")
        return out, rows_out, envs_out

    def sample(self, batch_size: int, env=None, seed: int = 0, counter: int = 0, return_indices: bool = False):
        """SB3's ReplayBuffer.sample(batch_size): a ReplayBufferSamples of CUDA tensors (observations [B, 18], actions
        [B, 3], next_observations [B, 18], dones [B, 1] = dones * (1 - timeouts), rewards [B, 1]), one launch.  Sample i is
        (row, env) drawn uniformly from [0, size()) x [0, n_envs) by Philox keyed with `seed` at draw `counter` -- not
        numpy's global stream, which SB3 uses; pass a new counter for every batch.  return_indices: also the int32 CUDA
        tensors (batch_inds, env_inds) that were drawn."""
        if env is not None:
            raise ValueError("env= (VecNormalize) is not supported: the samples are not normalised")
        batch = int(batch_size)
        if batch < 1:
            raise ValueError(f"batch_size must be positive, got {batch_size}")
        if self.size() < 1:
            raise ValueError("cannot sample from an empty replay buffer")
        out, rows, envs = self._sample(batch, int(seed), int(counter), None, None, bool(return_indices))
        return (out, rows, envs) if return_indices else out

    def _stacked(self, n_batches: int, batch: int):
        """The five stacked tensors of ``n_batches`` batches: [n_batches, batch, 18], [.., 3], [.., 18], [.., 1], [.., 1]."""
        t = self._torch
        f32 = dict(dtype=t.float32, device=self.device)
        return tuple(t.empty((n_batches, batch, w), **f32) for w in (OBS_DIM, ACT_DIM, OBS_DIM, 1, 1))

    def sample_batches(self, batch_size: int, n_batches: int, seed: int = 0, counter: int = 0, return_indices: bool = False):
        """``n_batches`` x ``sample(batch_size)`` in ONE launch (k_replay_sample_batches): a list of ReplayBufferSamples whose
        fields are contiguous views into five stacked tensors [n_batches, batch_size, .].  Batch g has exactly the bits of
        ``sample(batch_size, seed=seed, counter=counter + g)`` (the counter wraps modulo 2^64).  return_indices: also the int32
        CUDA tensors (batch_inds, env_inds), [n_batches, batch_size] each."""
        batch, G = int(batch_size), int(n_batches)
        if batch < 1:
            raise ValueError(f"batch_size must be positive, got {batch_size}")
        if G < 1:
            raise ValueError(f"n_batches must be positive, got {n_batches}")
        if G * batch > _capi.REPLAY_BATCHES_MAX_SAMPLES:
            raise ValueError(f"{G} batches of {batch} are {G * batch} samples; at most {_capi.REPLAY_BATCHES_MAX_SAMPLES} per launch")
        if self.size() < 1:
            raise ValueError("cannot sample from an empty replay buffer")
        t = self._torch
        stacked = self._stacked(G, batch)
        rows_out = envs_out = None
        if return_indices:
            rows_out = t.empty((G, batch), dtype=t.int32, device=self.device)
            envs_out = t.empty((G, batch), dtype=t.int32, device=self.device)
        self._venv._bind_stream()
        rc = self._L.meshenv_replay_sample_batches(
            self._venv._handle, self.store.data_ptr(), self.rows, self.size(), batch, G, C.c_uint64(int(seed) & (2 ** 64 - 1)),
            C.c_uint64(int(counter) & (2 ** 64 - 1)), *[x.data_ptr() for x in stacked],
            rows_out.data_ptr() if return_indices else None, envs_out.data_ptr() if return_indices else None)
        _capi.check(self._venv._handle, rc, "meshenv_replay_sample_batches")
        out = [ReplayBufferSamples(*[x[g] for x in stacked]) for g in range(G)]
        return (out, rows_out, envs_out) if return_indices else out

    def gather(self, batch_inds, env_inds, check: bool = True):
        """SB3's ReplayBuffer._get_samples(batch_inds) with explicit env indices: int32 CUDA tensors [B] of rows in
        [0, buffer_size) and envs in [0, n_envs).  check=True validates their range first (one host synchronisation);
        without it an index out of range is not read and its sample comes back as NaN."""
        t = self._torch
        for name, x in (("batch_inds", batch_inds), ("env_inds", env_inds)):
            if not hasattr(x, "data_ptr") or x.dtype != t.int32 or x.dim() != 1:
                raise ValueError(f"{name} must be a 1-D int32 tensor")
            if x.device != self.device or not x.is_contiguous():
                raise ValueError(f"{name} must be contiguous on {self.device}")
        if batch_inds.shape != env_inds.shape or batch_inds.numel() < 1:
            raise ValueError("batch_inds and env_inds must have the same, non-zero length")
        if self.size() < 1:
            raise ValueError("cannot gather from an empty replay buffer")
        if check:
            lo = t.stack([batch_inds.min(), env_inds.min()]).tolist()
            hi = t.stack([batch_inds.max(), env_inds.max()]).tolist()
            if lo[0] < 0 or hi[0] >= self.rows or lo[1] < 0 or hi[1] >= self.n_envs:
                raise ValueError(f"indices out of range: rows [{lo[0]}, {hi[0]}] of {self.rows}, envs [{lo[1]}, {hi[1]}] of "
                                 f"{self.n_envs}")
        return self._sample(int(batch_inds.numel()), 0, 0, batch_inds, env_inds, False)[0]
