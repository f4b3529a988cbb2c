"""SB3 2.x's ``OffPolicyAlgorithm.learn`` for SAC / TD3 with nothing leaving the device (include/meshenv_offpolicy_learn.h,
csrc/meshenv_learn.h):

    while num_timesteps < total_timesteps:
        collect train_freq vector steps          uniform Box actions while num_timesteps < learning_starts (k_uniform_actions),
                                                 then the LIVE behaviour actor (FusedActor / FusedPolicy after refresh())
        replay_buffer.add, Monitor               DeviceReplayBuffer.add_rollout, EpisodeStats.update (k_episode_stats)
        if num_timesteps > learning_starts:      FusedOffPolicyTrain.train(gradient_steps): one C call
            train(gradient_steps)                behaviour.refresh(): one launch, no host rebuild

``FusedOffPolicyLearn.learn`` enqueues all of it and reads nothing back; ``EpisodeStats`` is the Monitor's
``rollout/ep_rew_mean`` / ``rollout/ep_len_mean`` on the device.  The host half (the warm-up split, ``train_freq`` /
``gradient_steps``, the refusals) needs no GPU.  Restatement: tests/offpolicy_learn_ref.py."""
from __future__ import annotations

import numpy as np

from . import _capi
from . import sb3_nets as N
from ._handle import Handle
from .offpolicy_train import FusedOffPolicyTrain, check_replay_buffer
from .replay import DeviceReplayBuffer

MASK64 = 2 ** 64 - 1
DEFAULT_WINDOW = 100                                       # SB3's stats_window_size


# ------------------------------------------------------------------------------------------------------- the host half
def parse_train_freq(train_freq) -> int:
    """SB3's ``train_freq`` in vector steps: an int, ``(k, "step")`` or a ``TrainFreq(frequency, unit)``; a frequency in
    episodes is refused."""
    freq, unit = train_freq, "step"
    if hasattr(train_freq, "frequency") and hasattr(train_freq, "unit"):
        freq, unit = train_freq.frequency, train_freq.unit
    elif isinstance(train_freq, (tuple, list)):
        if len(train_freq) != 2:
            raise ValueError(f"train_freq must be an int or (frequency, unit), got {train_freq!r}")
        freq, unit = train_freq
    unit = getattr(unit, "value", unit)
    if unit == "episode":
        raise ValueError(f"train_freq = {train_freq!r}: a frequency in episodes is not supported (the collect is a fixed number "
                         "of vector steps); use (k, \"step\")")
    if unit != "step":
        raise ValueError(f"train_freq unit must be \"step\", got {unit!r}")
    if isinstance(freq, bool) or not isinstance(freq, (int, np.integer)) or freq < 1:
        raise ValueError(f"train_freq must be a positive int of vector steps, got {freq!r}")
    return int(freq)


def warmup_split(num_timesteps: int, n_envs: int, T: int, learning_starts: int) -> int:
    """How many of the T vector steps of a collect entered at ``num_timesteps`` are warm-up steps: step j is one iff
    ``num_timesteps + j * n_envs < learning_starts`` (SB3 tests before the step's increment), so they form a prefix."""
    if learning_starts <= num_timesteps:
        return 0
    return min(T, -(-(learning_starts - num_timesteps) // n_envs))


def should_train(num_timesteps: int, learning_starts: int) -> bool:
    """SB3: ``self.num_timesteps > 0 and self.num_timesteps > self.learning_starts`` (strictly past)."""
    return num_timesteps > 0 and num_timesteps > learning_starts


def resolve_gradient_steps(gradient_steps: int, T: int) -> int:
    """``gradient_steps`` of one train(): -1 (any negative, as SB3 tests ``>= 0``) is the T vector steps just collected."""
    if isinstance(gradient_steps, bool) or not isinstance(gradient_steps, (int, np.integer)):
        raise ValueError(f"gradient_steps must be an int, got {gradient_steps!r}")
    return int(gradient_steps) if gradient_steps >= 0 else T


def plan(num_timesteps: int, total_timesteps: int, n_envs: int, T: int, learning_starts: int, gradient_steps: int):
    """The whole schedule of one learn(): a list of (warm-up steps, behaviour steps, num_timesteps after the collect,
    gradient steps of the train() that follows or 0).  ``total_timesteps`` is the absolute target; the last collect
    overshoots it as SB3's does (a collect is never cut short)."""
    out = []
    while num_timesteps < total_timesteps:
        W = warmup_split(num_timesteps, n_envs, T, learning_starts)
        num_timesteps += T * n_envs
        K = resolve_gradient_steps(gradient_steps, T) if should_train(num_timesteps, learning_starts) else 0
        out.append((W, T - W, num_timesteps, K))
    return out


def noise_sigma(model, action_noise_sigma):
    """TD3's ``NormalActionNoise(0, sigma)`` as the sigma FusedPolicy takes: the argument, or ``model.action_noise._sigma``."""
    if action_noise_sigma is not None:
        return action_noise_sigma
    noise = getattr(model, "action_noise", None)
    if noise is None:
        return None
    if type(noise).__name__ not in ("NormalActionNoise", "VectorizedActionNoise") or not hasattr(noise, "_sigma"):
        raise ValueError(f"action_noise is {type(noise).__name__}; NormalActionNoise(0, sigma) is supported (or pass action_noise_sigma)")
    if np.any(np.asarray(getattr(noise, "_mu", 0.0)) != 0):
        raise ValueError("action_noise has a non-zero mean; NormalActionNoise(0, sigma) is supported")
    return np.asarray(noise._sigma, np.float32)


class OffPolicyLearnSpec:
    """What ``learn`` reads from an SB3-shaped SAC / TD3 model, with its refusals.  No device needed."""

    def __init__(self, model, n_envs: int, auto_reset: bool = True):
        name = type(model).__name__
        self.model = model
        actor = getattr(model, "actor", None)
        if actor is None:
            raise ValueError(f"{name} has no actor: not an SB3 SAC / TD3 model")
        if getattr(model, "use_sde", False) or getattr(actor, "use_sde", False):
            raise ValueError(f"{name}.use_sde=True (gSDE) is not supported: the behaviour noise is the state-independent Gaussian")
        if getattr(model, "use_sde_at_warmup", False):
            raise ValueError(f"{name}.use_sde_at_warmup=True is not supported: the warm-up actions are uniform Box samples")
        if not auto_reset:
            raise ValueError("venv.auto_reset is off: the collect relies on the step kernel's reset of finished episodes")
        self.sac = hasattr(actor, "latent_pi")
        for attr in ("learning_starts", "train_freq"):
            if not hasattr(model, attr):
                raise ValueError(f"{name} has no {attr}")
        ls = model.learning_starts
        if isinstance(ls, bool) or not isinstance(ls, (int, np.integer)) or ls < 0:
            raise ValueError(f"learning_starts must be an int >= 0, got {ls!r}")
        self.learning_starts = int(ls)
        self.train_freq = parse_train_freq(model.train_freq)
        self.gradient_steps = getattr(model, "gradient_steps", 1)
        resolve_gradient_steps(self.gradient_steps, self.train_freq)
        self.n_envs = int(n_envs)
        if self.n_envs < 1:
            raise ValueError(f"n_envs must be positive, got {n_envs}")
        if self.sac and getattr(model, "action_noise", None) is not None:
            raise ValueError("action_noise with SAC is not supported: the behaviour is the actor's own sample")

    def num_timesteps(self) -> int:
        nt = getattr(self.model, "num_timesteps", 0)
        if isinstance(nt, bool) or not isinstance(nt, (int, np.integer)) or nt < 0:
            raise ValueError(f"num_timesteps must be an int >= 0, got {nt!r}")
        return int(nt)


# ------------------------------------------------------------------------------------------------------- episode statistics
def ring_order(count: int, window: int):
    """The ring's slots from the oldest to the newest finished episode: deque(maxlen=window) order."""
    if count <= window:
        return list(range(count))
    first = count % window
    return [(first + k) % window for k in range(window)]


class EpisodeStats(Handle):
    """SB3's Monitor + ``ep_info_buffer`` on the device: per env the running episode return (the sequential float64 sum of its
    rewards in step order, what ``sum(self.rewards)`` gives up to Python 3.11) and length, and a ring of the last ``window``
    finished episodes (return, length, complete) in SB3's order (step, then env).  ``update(out)`` is one launch over the
    histories of a rollout dict and reads nothing back; ``read()`` makes one copy.  The Monitor's ``round(r, 6)`` is NOT
    applied: round the values read if the reference's printed figures are wanted."""
    PREFIX = "meshenv_episode_stats"

    def __init__(self, n_envs: int, window: int = DEFAULT_WINDOW, device: int = 0):
        n_envs, window = int(n_envs), int(window)
        if n_envs < 1 or window < 1:
            raise ValueError(f"n_envs and window must be positive, got {n_envs}, {window}")
        super().__init__(device)
        t = self._torch
        self.n_envs, self.window = n_envs, window
        R = _capi.EPISODE_RING_DOUBLES
        self.state = t.zeros(R * window + 1, dtype=t.float64, device=self.device)   # the ring, then the uint64 count
        self.ring = self.state[:R * window].view(window, R)
        self.count = self.state[R * window:].view(t.int64)
        self.carry_return = t.zeros(n_envs, dtype=t.float64, device=self.device)
        self.carry_len = t.zeros(n_envs, dtype=t.int32, device=self.device)
        self._work = None

    def update(self, out) -> None:
        """The reward [T, n] float64, done and complete [T, n] uint8 histories of one rollout dict (collect_rollout,
        step_actor_T, collect_uniform) or an object with those three attributes."""
        t = self._torch
        get = (lambda k: out[k]) if isinstance(out, dict) else (lambda k: getattr(out, k))
        reward, done, complete = get("reward"), get("done"), get("complete")
        if not hasattr(done, "dim") or done.dim() != 2 or done.shape[0] < 1 or done.shape[1] != self.n_envs:
            raise ValueError(f"done must be a [T, {self.n_envs}] tensor with T >= 1")
        T, n = int(done.shape[0]), self.n_envs
        for name, x, dtype in (("reward", reward, t.float64), ("done", done, t.uint8), ("complete", complete, t.uint8)):
            if x.dtype != dtype or tuple(x.shape) != (T, n) or x.device != self.device or not x.is_contiguous():
                raise ValueError(f"{name} must be a contiguous {dtype} tensor of shape ({T}, {n}) on {self.device}")
        if T * n >= 2 ** 31:
            raise ValueError(f"{T} x {n} entries exceed the int32 index")
        if self._work is None or self._work[0].numel() < T * n:
            self._work = (t.empty(T * n, dtype=t.float64, device=self.device), t.empty(T * n, dtype=t.int32, device=self.device))
        self._bind_stream()
        rc = self._L.meshenv_episode_stats_update(self._h, T, n, self.window, reward.data_ptr(), done.data_ptr(), complete.data_ptr(),
                                                  self.carry_return.data_ptr(), self.carry_len.data_ptr(), self.ring.data_ptr(),
                                                  self.count.data_ptr(), self._work[0].data_ptr(), self._work[1].data_ptr())
        self._check(rc, "meshenv_episode_stats_update")

    def read(self) -> dict:
        """One device-to-host copy.  ``episodes`` (all finished so far), ``complete_rate`` (the share of the ring's episodes
        that ended complete; NaN before the first) and, once an episode has finished, ``rollout/ep_rew_mean`` and
        ``rollout/ep_len_mean``: ``np.mean`` over the filled part of the ring in deque order, SB3's ``safe_mean``."""
        R = _capi.EPISODE_RING_DOUBLES
        host = self.state.cpu().numpy()
        count = int(host[R * self.window:].view(np.uint64)[0])
        ring = host[:R * self.window].reshape(self.window, R)[ring_order(count, self.window)]
        logs = {"episodes": count, "complete_rate": float(np.mean(ring[:, 2])) if count else float("nan")}
        if count:
            logs["rollout/ep_rew_mean"] = float(np.mean(ring[:, 0]))
            logs["rollout/ep_len_mean"] = float(np.mean(ring[:, 1]))
        return logs


# ------------------------------------------------------------------------------------------------------- the loop
class OffPolicyLearnLogs:
    """What a ``learn()`` leaves: ``read()`` merges the last ``train()``'s logs with the episode statistics and
    ``time/total_timesteps``."""

    def __init__(self, train_logs, stats: EpisodeStats, num_timesteps: int, iterations: int):
        self.train_logs, self.stats = train_logs, stats
        self.num_timesteps, self.iterations = num_timesteps, iterations

    def read(self) -> dict:
        logs = {} if self.train_logs is None else dict(self.train_logs.read())
        logs.update(self.stats.read())
        logs["time/total_timesteps"] = self.num_timesteps
        return logs


class FusedOffPolicyLearn:
    """``learn(total_timesteps)`` of an SB3-shaped SAC / TD3 model on a MeshVecEnv.  Drives a DeviceReplayBuffer, a
    FusedOffPolicyTrain, the live behaviour (SAC: a FusedActor, TD3: a deterministic FusedPolicy with the action-noise sigma)
    and an EpisodeStats; all stay usable on their own."""

    def __init__(self, spec: OffPolicyLearnSpec, venv, replay_buffer=None, behaviour=None, train=None, action_noise_sigma=None,
                 window: int = DEFAULT_WINDOW):
        from .actor import FusedActor
        from .policy import KIND_DETERMINISTIC, FusedPolicy
        self.spec, self.model, self.venv = spec, spec.model, venv
        model = spec.model
        if replay_buffer is not None:
            check_replay_buffer(replay_buffer, venv.device)
        index = venv.device.index or 0
        live = FusedActor.live_params(model) if spec.sac else N.td3_actor_params(*N.td3_live_actor(model))
        N.check_device(live, venv.device, "FusedOffPolicyLearn")
        self._owned = []
        self.buffer = replay_buffer if replay_buffer is not None else DeviceReplayBuffer(venv, getattr(model, "buffer_size", 1_000_000))
        if self.buffer._venv is not venv:
            raise ValueError("replay_buffer belongs to another venv")
        self.train = train if train is not None else self._own(FusedOffPolicyTrain.from_sb3(model, self.buffer, device=index))
        if self.train.model is not model or self.train.buffer is not self.buffer:
            raise ValueError("train drives another model or replay buffer")
        if behaviour is None:      # loaded ONCE from the live parameters; refresh() carries every later step in
            behaviour = self._own(FusedActor.from_sb3(model, device=index) if spec.sac else
                                  FusedPolicy.from_sb3(model, sigma=noise_sigma(model, action_noise_sigma), device=index))
        elif spec.sac != isinstance(behaviour, FusedActor) or (not spec.sac and behaviour.spec.kind != KIND_DETERMINISTIC):
            raise ValueError("behaviour must be a FusedActor for SAC, a deterministic FusedPolicy for TD3")
        if behaviour.device != venv.device:
            raise ValueError(f"behaviour is on {behaviour.device}, the envs on {venv.device}")
        behaviour.bind_live(model)
        self.behaviour = behaviour
        self.noisy = spec.sac or behaviour.spec.weights.get("log_std_or_sigma") is not None
        self.stats = self._own(EpisodeStats(venv.num_envs, window, index))
        self.steps = 0                # vector steps collected so far: the noise / draw counter of the next one
        self.collect_calls = {"uniform": 0, "behaviour": 0}
        self.last_train_logs = None

    def _own(self, h):
        self._owned.append(h)
        return h

    def close(self):
        for h in getattr(self, "_owned", []):
            h.close()
        self._owned = []

    @classmethod
    def from_sb3(cls, model, venv, replay_buffer=None, behaviour=None, train=None, action_noise_sigma=None,
                 window: int = DEFAULT_WINDOW):
        """model: SB3 2.x's SAC / TD3 or anything shaped like it (``learning_starts``, ``train_freq``, ``gradient_steps``,
        ``batch_size``, ``buffer_size``, ``num_timesteps`` and what FusedOffPolicyTrain reads).  venv: the MeshVecEnv.  What is
        not given is built here and closed by close(); what is given stays the caller's."""
        if replay_buffer is not None and not isinstance(replay_buffer, DeviceReplayBuffer):
            check_replay_buffer(replay_buffer, None)
        spec = OffPolicyLearnSpec(model, venv.num_envs, getattr(venv, "auto_reset", True))
        return cls(spec, venv, replay_buffer, behaviour, train, action_noise_sigma, window)

    # ---------------------------------------------------------------- collection
    def _collect_behaviour(self, P: int, seed: int, counter: int):
        """P vector steps chosen by the behaviour as it is NOW, vector step j at noise counter ``counter + j``.  The first
        action is sampled on the env's current observation (never a pipelined action of an earlier, staler actor)."""
        env, b = self.venv, self.behaviour
        if self.spec.sac:
            obs0 = env.obs.clone()
            first = b.sample(obs0, seed, counter)
            out = env.step_actor_T(b, first, P, seed=seed, counter=counter + 1, want_terminal_obs=True)
            self.buffer.add_rollout(out, obs0=obs0)
        else:
            out = env.collect_rollout(b, P, seed=seed, counter=counter, deterministic=not self.noisy)
            self.buffer.add_rollout(out)
        self.collect_calls["behaviour"] += 1
        return out

    def _check_callback(self, callback, num: int, total: int, n: int, T: int) -> None:
        """The refusals of ``learn(callback=...)``, made before anything is enqueued."""
        from .eval_callback import DeviceEvalCallback, schedule
        if not isinstance(callback, DeviceEvalCallback):
            raise TypeError(f"callback must be a DeviceEvalCallback, got {type(callback).__name__}")
        if callback.eval_venv is self.venv:
            raise ValueError("the callback's eval_venv is the training env: an evaluation resets its env; give it a MeshVecEnv of its own")
        if callback.eval_venv.device != self.venv.device:
            raise ValueError(f"the callback's eval envs are on {callback.eval_venv.device}, the training envs on {self.venv.device}")
        if callback.model is not self.model:
            raise ValueError("the callback keeps another model's parameters")
        callback.room(len(schedule(callback.n_calls, num, total, n, T, callback.eval_freq)[0]))

    def learn(self, total_timesteps: int, seed: int = 0, log_interval=None, callback=None) -> OffPolicyLearnLogs:
        """SB3's ``learn(total_timesteps, reset_num_timesteps=False)``: continues from ``model.num_timesteps`` for
        ``total_timesteps`` more (a first call starts at 0).  Everything is enqueued on the current stream; nothing is copied
        to the host and nothing synchronises.  seed keys the warm-up draw, the behaviour noise and the minibatch draw (three
        Philox streams of their own).  log_interval is accepted for SB3's signature; read the returned object instead.
        callback: a DeviceEvalCallback; the evaluations SB3's EvalCallback would make during a collect are enqueued in front
        of it (the parameters change only in train()), each stamped with SB3's num_timesteps at its call."""
        spec, model, env = self.spec, self.model, self.venv
        if isinstance(total_timesteps, bool) or not isinstance(total_timesteps, (int, np.integer)) or total_timesteps < 0:
            raise ValueError(f"total_timesteps must be an int >= 0, got {total_timesteps!r}")
        n, T = spec.n_envs, parse_train_freq(model.train_freq)
        num = spec.num_timesteps()
        total = int(total_timesteps) + num
        seed = int(seed)
        iterations = 0
        if callback is not None:
            self._check_callback(callback, num, total, n, T)
        for W, P, after, K in plan(num, total, n, T, int(model.learning_starts), getattr(model, "gradient_steps", 1)):
            if callback is not None:
                callback.before_collect(self.behaviour, after - T * n, T, n)
            if W:
                out = env.collect_uniform(W, seed=seed, counter=self.steps & MASK64)
                self.buffer.add_rollout(out)
                self.stats.update(out)
                self.collect_calls["uniform"] += 1
            if P:
                self.stats.update(self._collect_behaviour(P, seed, (self.steps + W) & MASK64))
            self.steps += T
            model.num_timesteps = after
            model._current_progress_remaining = 1.0 - float(after) / float(total)
            if K > 0:
                self.last_train_logs = self.train.train(K, seed=seed)
                self.behaviour.refresh()
            iterations += 1
        return OffPolicyLearnLogs(self.last_train_logs, self.stats, spec.num_timesteps(), iterations)
