"""SB3 2.x's ``OnPolicyAlgorithm.learn`` for PPO / A2C as one object (include/meshenv_onpolicy_learn.h,
csrc/meshenv_onpolicy_train.h: k_optim_step_counted, k_learn_finish):

    while num_timesteps < total_timesteps:
        collect_rollouts(env, callback, rollout_buffer, n_steps)     MeshVecEnv.collect_rollout(gamma=...), EpisodeStats.update,
                                                                     DeviceEvalCallback.before_collect in front of it
        _update_current_progress_remaining(num_timesteps, total)
        train()                                                      FusedOnPolicyTrain.train: one C call, refresh at its tail

``FusedOnPolicyLearn.learn`` enqueues all of it.  A2C and a PPO without a ``target_kl`` know on the host how many optimiser
steps every ``train()`` applies, so nothing is read back at all.  A PPO WITH a ``target_kl`` does not: its early stop is decided
on the device, and the Adam bias corrections of the next ``train()`` depend on how many steps this one applied.
``FusedOnPolicyTrain.train`` therefore reads that count back once per call.  Inside ``learn`` the count stays on the device
(``StepCounter``): the steps look their bias corrections up in a table by it, and ``learn`` ends with ONE small read-back
(the step count, the ``_n_updates`` word, the error word), after which the optimiser's ``step`` tensors and
``model._n_updates`` are written exactly as ``train()`` writes them.

The host half (``plan``, ``bias_table``, ``segments``, ``OnPolicyLearnSpec``, ``check_handles``) needs no GPU."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi
from . import sb3_nets as N
from ._handle import Handle
from .offpolicy_learn import DEFAULT_WINDOW, MASK64, EpisodeStats
from .onpolicy_train import OUTPUTS, FusedOnPolicyTrain, hyper, step_values
from .rollout_buffer import minibatch_bounds

TABLE_CAP = _capi.LEARN_MAX_ENTRIES                        # entries (of 16 bytes per block) one bound table holds


# ------------------------------------------------------------------------------------------------------- the host half
def plan(num_timesteps: int, total_timesteps: int, n_envs: int, n_steps: int):
    """The iterations of one learn(): a list of (num_timesteps before the collect, after it, ``_current_progress_remaining``
    at its train()).  ``total_timesteps`` is the absolute target; the last collect overshoots it as SB3's does."""
    out = []
    while num_timesteps < total_timesteps:
        before = num_timesteps
        num_timesteps += n_steps * n_envs
        out.append((before, num_timesteps, 1.0 - float(num_timesteps) / float(total_timesteps)))
    return out


def bias_table(step0: float, entries: int, beta1: float, beta2: float):
    """[(bias_correction1, bias_correction2_sqrt)] of the 1st .. entries-th step after ``step0``, in Python doubles and in
    ``adam_scalars``' own expressions, from ``step_values`` (which keeps the float32 increments of ``state['step']``).  With
    them ``lr / bias_correction1`` and ``bias_correction2_sqrt``, rounded to float32, are what ``scalar_sets`` stores."""
    return [(1 - beta1 ** step, (1 - beta2 ** step) ** 0.5) for step in step_values(step0, entries)[1:]]


def segments(iterations: int, K: int, cap: int):
    """[(first iteration, iterations)]: runs of train() calls whose K steps each fit one table of ``cap`` entries together.  A
    single train() is never split: a cap below K gives segments of one iteration, each with a table of K entries."""
    per = max(1, cap // K)
    return [(first, min(per, iterations - first)) for first in range(0, iterations, per)]


def minibatches(model, rows: int) -> int:
    """K = n_epochs x minibatches per epoch of one train() over ``rows`` rows, as ``FusedOnPolicyTrain.train`` counts them."""
    hp = hyper(model)
    return hp["n_epochs"] * len(minibatch_bounds(rows, hp["batch_size"]))


class OnPolicyLearnSpec:
    """What ``learn`` reads from an SB3-shaped PPO / A2C model, with its refusals.  No device needed."""

    def __init__(self, model, n_envs: int, auto_reset: bool = True):
        name = type(model).__name__
        self.model = model
        policy = getattr(model, "policy", None)
        if hasattr(model, "actor") or policy is None or not hasattr(policy, "mlp_extractor"):
            raise ValueError(f"{name}.policy is not an actor-critic policy (mlp_extractor, action_net, value_net, log_std): "
                             "FusedOnPolicyLearn runs PPO / A2C; SAC / TD3 have FusedOffPolicyLearn")
        if getattr(model, "use_sde", False) or getattr(policy, "use_sde", False):
            raise ValueError(f"{name}.use_sde=True (gSDE) is not supported: the rollout noise is the state-independent Gaussian")
        if not auto_reset:
            raise ValueError("venv.auto_reset is off: the collect relies on the step kernel's reset of finished episodes")
        n_steps = getattr(model, "n_steps", None)
        if n_steps is None:
            raise ValueError(f"{name} has no n_steps")
        if isinstance(n_steps, bool) or not isinstance(n_steps, (int, np.integer)) or n_steps < 1:
            raise ValueError(f"n_steps must be a positive int, got {n_steps!r}")
        self.n_envs = int(n_envs)
        if self.n_envs < 1:
            raise ValueError(f"n_envs must be positive, got {n_envs}")
        if int(n_steps) * self.n_envs > _capi.ROLLOUT_MAX_ROWS:
            raise ValueError(f"n_steps x n_envs = {int(n_steps) * self.n_envs} rows; at most ROLLOUT_MAX_ROWS = {_capi.ROLLOUT_MAX_ROWS}")
        self.n_steps = int(n_steps)
        for attr in ("gamma", "gae_lambda"):
            if not hasattr(model, attr):
                raise ValueError(f"{name} has no {attr}")
        hyper(model)

    @property
    def rows(self) -> int:
        return self.n_steps * self.n_envs

    def counted(self) -> bool:
        """True for what takes the counted path: PPO with a target_kl."""
        return hyper(self.model)["target_kl"] is not None

    def num_timesteps(self) -> int:
        nt = getattr(self.model, "num_timesteps", 0)
        if isinstance(nt, bool) or not isinstance(nt, (int, np.integer)) or nt < 0:
            raise ValueError(f"num_timesteps must be an int >= 0, got {nt!r}")
        return int(nt)


def check_handles(model, policy, train) -> None:
    """The refusals of a ``policy`` / ``train`` that the caller hands in: a policy of another kind or bound to another model's
    parameters, a train() object for another model or another rollout policy."""
    from .policy import HIDDEN_WIDTHS, KIND_ACTOR_CRITIC
    if policy is not None:
        if getattr(getattr(policy, "spec", None), "kind", None) != KIND_ACTOR_CRITIC:
            raise ValueError("policy is not an actor-critic FusedPolicy: the rollout needs log_prob and value")
        live = getattr(policy, "_live", None)
        if live is not None:
            own = N.actor_critic_live(model, widths=HIDDEN_WIDTHS)[2]
            if len(live) != len(own) or any(a.data_ptr() != b.data_ptr() for a, b in zip(live, own)):
                raise ValueError("policy is bound (bind_live) to another model's parameters")
    if train is not None:
        if getattr(train, "model", None) is not model:
            raise ValueError("train drives another model")
        if policy is not None and getattr(train, "policy", None) is not policy:
            raise ValueError("train refreshes another rollout policy than policy")
        if policy is None and getattr(train, "policy", None) is None:
            raise ValueError("train has no rollout policy to refresh: build it with the FusedPolicy that collects")


# ------------------------------------------------------------------------------------------------------- the counter
class StepCounter(Handle):
    """The device-resident step count of a run of counted ``train()`` calls, its table of bias corrections and their history.

    ``bind(plan, entries, iterations)`` forms the table from the optimiser's host ``step`` as it stands (the origin), uploads it
    and zeroes the words, stream-ordered.  ``FusedOnPolicyTrain.train(out, perms, counted=counter)`` then runs without a
    read-back.  ``read()`` is the ONE copy: it raises if a launch found its count outside the table, writes the ``step`` tensors
    and ``model._n_updates`` as ``train()`` writes them, and returns (steps applied, epochs entered)."""
    PREFIX = "meshenv_onpolicy_learn"

    def __init__(self, model, device: int = 0):
        super().__init__(device)
        t = self._torch
        self.model = model
        self.words = t.zeros(_capi.LEARN_WORDS + _capi.TRAIN_MAX_MINIBATCHES, dtype=t.int32, device=self.device)
        self.history = None           # [iterations, 12] float64 on the device, OUTPUTS' order
        self.pending = []             # the TrainLogs of the train() calls since the bind
        self.entries = self.claimed = 0
        self._origin = None           # (plan.groups, per group the step values from the origin on)

    def bind(self, plan, entries: int, iterations: int) -> None:
        t = self._torch
        entries, iterations = int(entries), int(iterations)
        if not 1 <= entries <= _capi.LEARN_MAX_ENTRIES:
            raise ValueError(f"a table holds 1 .. {_capi.LEARN_MAX_ENTRIES} entries, got {entries}")
        if iterations < 1:
            raise ValueError(f"iterations must be positive, got {iterations}")
        if self.pending:
            raise ValueError("bind() before read(): the counted train() calls in flight have not been accounted for")
        blocks = len(plan.groups)
        table = (C.c_double * (entries * blocks * 2))()
        values = []
        for b, (g, steps) in enumerate(plan.groups):
            if "betas" in g:
                beta1, beta2 = g["betas"]
                rows = bias_table(steps[0].item(), entries, beta1, beta2)
            else:                                            # RMSprop: lr itself, no correction
                rows = [(1.0, 1.0)] * entries
            values.append(step_values(steps[0].item(), entries))
            for j, (bc1, bc2s) in enumerate(rows):
                table[(j * blocks + b) * 2], table[(j * blocks + b) * 2 + 1] = bc1, bc2s
        self._bind_stream()
        rc = self._L.meshenv_onpolicy_learn_bind(self._h, table, entries, blocks, self.words.data_ptr(), self.words.numel())
        self._check(rc, "meshenv_onpolicy_learn_bind")
        self.history = t.zeros((iterations, _capi.TRAIN_OUTPUTS), dtype=t.float64, device=self.device)
        self.entries, self.claimed = entries, 0
        self._origin = (plan.groups, values)

    def check(self, train, K: int) -> None:
        """What ``train(counted=...)`` asks before anything is enqueued."""
        if train.model is not self.model:
            raise ValueError("the counter belongs to another model")
        if self._origin is None:
            raise ValueError("the counter has no table bound (StepCounter.bind)")
        if self.claimed + K > self.entries:
            raise ValueError(f"{K} minibatches after {self.claimed} claimed since the bind; the table has {self.entries} entries")
        if len(self.pending) >= self.history.shape[0]:
            raise ValueError(f"the history holds {self.history.shape[0]} iterations")

    def run(self, train, head, spec, plan, K: int):
        """The C call of a counted train(): ``head`` is what meshenv_onpolicy_train_run takes up to target_kl."""
        if [id(g) for g, _ in plan.groups] != [id(g) for g, _ in self._origin[0]]:
            raise ValueError("the optimiser's param groups are not the ones the table was formed from (bind again)")
        S = _capi.MeshOptimCounted()
        for b, (g, _) in enumerate(plan.groups):
            if "betas" in g:
                (beta1, beta2), lr, eps = g["betas"], g["lr"], g["eps"]
                S.lr[b], S.w1[b], S.beta2[b], S.w2[b], S.eps[b] = lr, 1 - beta1, beta2, 1 - beta2, eps
            else:
                S.lr[b], S.w1[b], S.beta2[b], S.w2[b], S.eps[b] = g["lr"], 0.0, g["alpha"], 1 - g["alpha"], g["eps"]
        S.tau, S.one_minus_tau = spec.tau, 1 - spec.tau
        i = len(self.pending)
        rc = self._L.meshenv_onpolicy_learn_run(self._h, *head, S, self.history.data_ptr(), i, self.history.shape[0])
        self._check(rc, "meshenv_onpolicy_learn_run")
        self.claimed += K
        return self.history[i]

    def read(self):
        """The one read-back; see the class."""
        if self._origin is None:
            raise ValueError("the counter has no table bound (StepCounter.bind)")
        n_updates, error, steps = (int(v) for v in self.words[:_capi.LEARN_WORDS].cpu().tolist())
        pending, self.pending = self.pending, []
        groups, values = self._origin
        self._origin = None
        if error or not 0 <= steps <= self.entries:
            raise _capi.MeshEnvError(f"a counted step found its count outside the table of {self.entries} entries (count {steps}, "
                                     f"error word {error}): the steps from there on were not applied")
        for (g, step_tensors), vals in zip(groups, values):
            for s in step_tensors:
                s.fill_(vals[steps])
        model = self.model
        model._n_updates = getattr(model, "_n_updates", 0) + n_updates
        for logs in pending:
            logs.n_updates = model._n_updates
        return steps, n_updates


# ------------------------------------------------------------------------------------------------------- the loop
class OnPolicyLearnLogs:
    """What a ``learn()`` leaves.  ``read()``: the last iteration's train logs, the episode statistics,
    ``time/total_timesteps`` and ``time/iterations``; the train logs and the history come from ONE copy of the history
    (the episode statistics make their own).  ``history()``: the [iterations, 12] rows in ``OUTPUTS``' order."""

    def __init__(self, rows, train_logs, stats: EpisodeStats, num_timesteps: int, iterations: int):
        self._rows, self.train_logs, self.stats = rows, train_logs, stats
        self.num_timesteps, self.iterations = num_timesteps, iterations
        self._host = None

    @property
    def device(self):
        """[iterations, 12] float64 on the GPU."""
        if not hasattr(self._rows, "dim"):
            import torch
            self._rows = torch.stack(self._rows) if self._rows else torch.zeros((0, len(OUTPUTS)), dtype=torch.float64)
        return self._rows

    def history(self) -> np.ndarray:
        if self._host is None:
            self._host = self.device.cpu().numpy()
        return self._host

    def read(self) -> dict:
        logs = {}
        if self.train_logs is not None:
            self.train_logs._host = self.history()[-1].tolist()
            logs.update(self.train_logs.read())
        logs.update(self.stats.read())
        logs["time/total_timesteps"] = self.num_timesteps
        logs["time/iterations"] = self.iterations
        return logs


class FusedOnPolicyLearn:
    """``learn(total_timesteps)`` of an SB3-shaped PPO / A2C model on a MeshVecEnv.  Drives a FusedPolicy with ``bind_live``
    done, a FusedOnPolicyTrain and an EpisodeStats; what ``from_sb3`` is not given it builds and ``close()`` closes, what it is
    given stays the caller's and stays usable on its own."""

    def __init__(self, spec: OnPolicyLearnSpec, venv, policy=None, train=None, window: int = DEFAULT_WINDOW):
        from .policy import FusedPolicy
        self.spec, self.model, self.venv = spec, spec.model, venv
        model = spec.model
        check_handles(model, policy, train)
        if policy is None and train is not None:
            policy = train.policy
        index = venv.device.index or 0
        self._owned = []
        if policy is None:
            policy = self._own(FusedPolicy.from_sb3(model, device=index))
        if policy.device != venv.device:
            raise ValueError(f"policy is on {policy.device}, the envs on {venv.device}")
        if getattr(policy, "_live", None) is None:
            policy.bind_live(model)
        self.policy = policy
        self.train = train if train is not None else self._own(FusedOnPolicyTrain.from_sb3(model, policy, device=index))
        self.stats = self._own(EpisodeStats(venv.num_envs, window, index))
        self.counter = None           # the StepCounter, built by the first learn() that needs it
        self.steps = 0                # vector steps collected so far: the noise counter of the next collect
        self.iterations = 0           # across learn() calls: time/iterations
        self.readbacks = 0            # device-to-host copies learn() has made (one per segment of a counted learn())
        self.last_train_logs = None

    def _own(self, h):
        self._owned.append(h)
        return h

    def close(self):
        for h in reversed(getattr(self, "_owned", [])):
            h.close()
        self._owned = []

    @classmethod
    def from_sb3(cls, model, venv, policy=None, train=None, window: int = DEFAULT_WINDOW):
        """model: SB3 2.x's PPO / A2C or anything shaped like it (``n_steps``, ``gamma``, ``gae_lambda``, ``num_timesteps`` and
        what FusedOnPolicyTrain reads).  venv: the MeshVecEnv.  policy: the actor-critic FusedPolicy that collects (bound to
        the model with ``bind_live`` here if it is not yet), train: the FusedOnPolicyTrain built with that policy."""
        spec = OnPolicyLearnSpec(model, venv.num_envs, getattr(venv, "auto_reset", True))
        return cls(spec, venv, policy, train, window)

    def _check_callback(self, callback, num: int, total: int, n: int, T: int) -> None:
        """The refusals of ``learn(callback=...)``, made before anything is enqueued: FusedOffPolicyLearn's."""
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

    def _perms(self, perms, iterations: int, n_epochs: int, rows: int):
        """``perms`` as learn takes it -> a function iteration -> [n_epochs, rows] or None."""
        if perms is None:
            return lambda i: None
        if callable(perms):
            return perms
        t = self.train._torch
        if not t.is_tensor(perms) or perms.dtype not in (t.int32, t.int64):
            raise ValueError("perms must be None, a callable iteration -> [n_epochs, rows] or an int32 / int64 tensor")
        if tuple(perms.shape) != (iterations, n_epochs, rows):
            raise ValueError(f"perms has shape {tuple(perms.shape)}, not ({iterations}, {n_epochs}, {rows}): [iterations, n_epochs, rows]")
        if perms.device != self.venv.device:
            perms = perms.to(self.venv.device)
        return lambda i: perms[i]

    def learn(self, total_timesteps: int, seed: int = 0, callback=None, perms=None) -> OnPolicyLearnLogs:
        """SB3's ``learn(total_timesteps, reset_num_timesteps=False)``: continues from ``model.num_timesteps`` for
        ``total_timesteps`` more (a first call starts at 0); the last collect overshoots the target as SB3's does.  Everything
        is enqueued on the current stream.  seed keys the rollout noise (vector step j of the whole run at counter j).
        perms: None draws the minibatch permutations as ``train()`` draws them; an int32 / int64 tensor [iterations, n_epochs,
        rows] or a callable iteration -> [n_epochs, rows] is used as given.  callback: a DeviceEvalCallback for this model with
        an env of its own; the evaluations SB3's EvalCallback would make during a collect are enqueued in front of it (the
        parameters change only in train()), each stamped with SB3's num_timesteps at its call.

        A2C and a PPO without a target_kl: nothing is copied to the host and nothing synchronises.  A PPO with a target_kl:
        every train() takes the counted path, and between entering and returning the only copy is ONE small read-back at the
        end (the step count, the ``_n_updates`` word, the error word), after which the optimiser's ``step`` tensors and
        ``model._n_updates`` are written as ``train()`` writes them, so a stock ``optimizer.step()``, ``state_dict()``,
        ``train.train(out)`` and a second ``learn()`` see consistent host state.  The table the steps read is re-derived from
        the host ``step`` at every learn() and holds at most ``TABLE_CAP`` = 2^20 entries of 16 bytes (for the one block of the
        policy optimiser): a learn() whose iterations x K exceed that runs in segments of whole train() calls, with that same
        read-back between two segments."""
        spec, model, env, tr = self.spec, self.model, self.venv, self.train
        if isinstance(total_timesteps, bool) or not isinstance(total_timesteps, (int, np.integer)) or total_timesteps < 0:
            raise ValueError(f"total_timesteps must be an int >= 0, got {total_timesteps!r}")
        n, T = spec.n_envs, spec.n_steps
        if getattr(model, "n_steps", None) != T:
            raise ValueError(f"model.n_steps changed from {T} to {getattr(model, 'n_steps', None)!r}: build a new FusedOnPolicyLearn")
        num = spec.num_timesteps()
        total = int(total_timesteps) + num
        seed = int(seed)
        its = plan(num, total, n, T)
        hp = hyper(model)
        K = minibatches(model, spec.rows)
        perm_of = self._perms(perms, len(its), hp["n_epochs"], spec.rows)
        if callback is not None:
            self._check_callback(callback, num, total, n, T)
        counted = hp["target_kl"] is not None
        rows_dev = []
        logs = None
        for first, count in (segments(len(its), K, TABLE_CAP) if counted else [(0, len(its))]):
            if counted and count:
                if self.counter is None:
                    self.counter = self._own(StepCounter(model, env.device.index or 0))
                self.counter.bind(tr._prepared()[0], count * K, count)
            for i in range(first, first + count):
                before, after, progress = its[i]
                if callback is not None:
                    callback.before_collect(self.policy, before, T, n)
                out = env.collect_rollout(self.policy, T, seed=seed, counter=self.steps & MASK64, gamma=model.gamma,
                                          gae_lambda=model.gae_lambda)
                self.stats.update(out)
                self.steps += T
                model.num_timesteps = after
                model._current_progress_remaining = progress
                logs = tr.train(out, perm_of(i), counted=self.counter if counted else None)
                rows_dev.append(logs.device)
                self.iterations += 1
            if counted and count:
                self.counter.read()
                self.readbacks += 1
        if logs is not None:
            self.last_train_logs = logs
        return OnPolicyLearnLogs(rows_dev, logs, self.stats, spec.num_timesteps(), self.iterations)
