"""SB3 2.x's ``EvalCallback`` (the reference's ``CustomCallback``, rl/baselines/CustomizeCallback.py:241-310) decided on the
device (include/meshenv_eval_callback.h, csrc/meshenv_eval_callback.h):

    every eval_freq vector steps:                    FusedOffPolicyLearn.learn(callback=cb), or cb.evaluate_now(policy, t) by hand
        evaluate_policy(model, eval_env)             meshenv_evaluate_queued: reset, then eval_steps x (policy, step, k_eval_tally)
        evaluations.npz, eval/mean_reward            k_eval_reduce: one float64 history row per evaluation
        if mean_reward > best_mean_reward:           ... and the ``improved`` word, strictly greater, NaN never
            model.save("best_model")                 k_keep_best: the live parameters into one flat buffer, gated by that word

``evaluate_now`` enqueues all of it on the current stream and reads nothing back; ``read()`` makes one copy.  The host half
(the schedule, the snapshot set, every refusal) needs no GPU.  The optimiser state is NOT part of the snapshot (SB3's
``best_model.zip`` does hold it).  Restatement: tests/eval_callback_ref.py."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi
from . import sb3_nets as N
from ._handle import Handle
from .evaluation import episode_targets

MASK64 = 2 ** 64 - 1
COLUMNS = _capi.EVAL_COLUMNS
AC_NAMES = ("pi.0.weight", "pi.0.bias", "pi.1.weight", "pi.1.bias", "action_net.weight", "action_net.bias",
            "vf.0.weight", "vf.0.bias", "vf.1.weight", "vf.1.bias", "value_net.weight", "value_net.bias", "log_std")


# ------------------------------------------------------------------------------------------------------- the host half
def _positive_int(v, name, limit=2 ** 31):
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= v < limit:
        raise ValueError(f"{name} must be an int >= 1, got {v!r}")
    return int(v)


def eval_points(n_calls: int, T: int, eval_freq: int) -> list:
    """The vector steps j = 1 .. T of a collect entered with ``n_calls`` callback calls behind it at which SB3's EvalCallback
    evaluates: ``(n_calls + j) % eval_freq == 0`` (BaseCallback.on_step increments n_calls, then _on_step tests it)."""
    first = eval_freq - n_calls % eval_freq
    return list(range(first, T + 1, eval_freq))


def schedule(n_calls: int, num_timesteps: int, total_timesteps: int, n_envs: int, T: int, eval_freq: int):
    """The evaluations of one learn(): ([(collect index, n_calls at the evaluation, its num_timesteps stamp)], n_calls after).
    ``total_timesteps`` is the absolute target; collects are never cut short.  Parameters change only in train(), so the
    evaluation at vector step j of collect i sees the behaviour as it stands before collect i."""
    out, i = [], 0
    while num_timesteps < total_timesteps:
        out += [(i, n_calls + j, num_timesteps + j * n_envs) for j in eval_points(n_calls, T, eval_freq)]
        n_calls += T
        num_timesteps += T * n_envs
        i += 1
    return out, n_calls


def model_kind(model) -> str:
    """"sac", "td3" or "ac" (PPO / A2C), by the attributes the recognisers of sb3_nets read."""
    actor = getattr(model, "actor", None)
    if actor is not None and hasattr(actor, "latent_pi"):
        return "sac"
    if actor is not None and hasattr(actor, "mu"):
        return "td3"
    return "ac"


def snapshot_set(model):
    """(kind, [(name, live tensor)]): what ``best_model`` keeps.  SAC: the actor's ten tensors, both critics, both target
    critics and ``log_ent_coef`` when it is learned; TD3: actor, actor target, critics, critic targets; PPO / A2C: the 13
    tensors of the ActorCriticPolicy.  Every refusal is the recognisers' own."""
    from .actor import FusedActor
    from .policy import HIDDEN_WIDTHS
    kind = model_kind(model)
    named = []

    def add(prefix, tensors):
        named.extend((f"{prefix}.{i // 2}.{'bias' if i % 2 else 'weight'}", x) for i, x in enumerate(tensors))

    if kind == "ac":
        _, _, tensors = N.actor_critic_live(model, widths=HIDDEN_WIDTHS)
        named = list(zip(AC_NAMES, tensors))
    else:
        k = N.KIND_SAC if kind == "sac" else N.KIND_TD3
        if kind == "sac":
            add("actor", FusedActor.live_params(model))
        else:
            add("actor", N.td3_actor_params(*N.td3_live_actor(model)))
            if getattr(model, "actor_target", None) is None:
                raise ValueError(f"{type(model).__name__} has no actor_target: not an SB3 TD3 model")
            add("actor_target", N.td3_actor_params(*N.td3_actor(model.actor_target)))
        for attr in ("critic", "critic_target"):
            for j, q in enumerate(N.twin_params(k, *N.twin_critics(model, attr))):
                add(f"{attr}.q{j}", q)
        if kind == "sac" and getattr(model, "log_ent_coef", None) is not None:
            named.append(("log_ent_coef", N.ent_coef(model.log_ent_coef, None)[0]))
    if len(named) > _capi.KEEP_BEST_MAX_ENTRIES:
        raise ValueError(f"{len(named)} tensors; one snapshot holds up to {_capi.KEEP_BEST_MAX_ENTRIES}")
    return kind, named


def best_layout(named):
    """([float offset of every tensor], floats in all): each tensor starts on a 16-byte boundary of the best buffer."""
    offsets, at = [], 0
    for _, x in named:
        offsets.append(at)
        at += -(-int(x.numel()) // 4) * 4
    return offsets, max(at, 4)


def check_policy(kind: str, policy) -> None:
    """The policy an evaluation steps must be of the model's kind: a FusedActor for SAC, a deterministic FusedPolicy for TD3,
    an actor-critic FusedPolicy for PPO / A2C."""
    from .actor import FusedActor
    from .policy import KIND_ACTOR_CRITIC, KIND_DETERMINISTIC, FusedPolicy
    if kind == "sac":
        ok = isinstance(policy, FusedActor)
    else:
        ok = isinstance(policy, FusedPolicy) and policy.spec.kind == (KIND_DETERMINISTIC if kind == "td3" else KIND_ACTOR_CRITIC)
    if not ok:
        want = {"sac": "a FusedActor (SAC)", "td3": "a deterministic FusedPolicy (TD3)", "ac": "an actor-critic FusedPolicy (PPO / A2C)"}[kind]
        raise ValueError(f"the model is evaluated through {want}, got {type(policy).__name__}")


def sb3_order(step, owner):
    """The order of SB3's ``episode_rewards``: by the vector step an episode ended at, then by env."""
    return np.lexsort((owner, step))


# ------------------------------------------------------------------------------------------------------- the callback
class DeviceEvalCallback(Handle):
    """``EvalCallback(eval_env, n_eval_episodes, eval_freq, deterministic)`` with the decision on the device.

    eval_venv: a MeshVecEnv of its own on the model's device (an evaluation resets it; ``learn`` refuses its training env).
    model: SB3's SAC / TD3 / PPO / A2C or anything shaped like it; its live tensors (``snapshot_set``) are what is kept.
    behaviour: the policy ``learn(callback=...)`` evaluates, refreshed before each evaluation (None: learn's own behaviour).
    n_eval_episodes / episodes_per_env: as ``MeshVecEnv.evaluate``.  eval_freq: in vector steps, SB3's.  eval_steps: the FIXED
    number of vector steps of every evaluation: nothing is read back, so the run cannot stop early; episodes that do not
    end within it are not recorded (``short`` counts their envs).  Evaluation k draws its noise (deterministic=False) at
    counter ``k * eval_steps`` under ``eval_seed``.  capacity: evaluations the history holds; one more is refused, and
    capacity x max(episodes, envs) must stay below 2^31 (the per-evaluation records are kept for ``save_npz``)."""
    PREFIX = "meshenv_eval_callback"

    def __init__(self, eval_venv, model, behaviour=None, n_eval_episodes=None, episodes_per_env=None, eval_freq: int = 1000,
                 eval_steps: int = 256, deterministic: bool = True, eval_seed: int = 0, capacity: int = 256):
        self.eval_freq = _positive_int(eval_freq, "eval_freq")
        self.eval_steps = _positive_int(eval_steps, "eval_steps")
        self.capacity = _positive_int(capacity, "capacity")
        if not hasattr(eval_venv, "evaluate") or not hasattr(eval_venv, "num_envs"):
            raise TypeError(f"eval_venv must be a MeshVecEnv, got {type(eval_venv).__name__}")
        n = int(eval_venv.num_envs)
        self.targets = episode_targets(n, n_eval_episodes, episodes_per_env)
        self.kind, named = snapshot_set(model)
        N.check_device([x for _, x in named], eval_venv.device, "DeviceEvalCallback (the eval env's device)")
        if behaviour is not None:
            check_policy(self.kind, behaviour)
            if behaviour.device != eval_venv.device:
                raise ValueError(f"behaviour is on {behaviour.device}, the eval envs on {eval_venv.device}")
        if self.capacity * max(int(self.targets.sum()), n) >= 2 ** 31:
            raise ValueError("capacity x episodes exceeds the int32 index of the kept records")
        super().__init__(eval_venv.device.index or 0)
        t = self._torch
        self.eval_venv, self.model, self.behaviour = eval_venv, model, behaviour
        self.deterministic, self.eval_seed = bool(deterministic), int(eval_seed)
        self.n_envs = n
        self.n_calls = 0                       # SB3's BaseCallback.n_calls: vector steps seen, across learn() calls
        self.evaluations = 0                   # evaluations enqueued so far: the next history row
        if behaviour is not None:
            behaviour.bind_live(model)
        # the tally's buffers.  The records SB3 writes to evaluations.npz (return, length, and step + count for their order) are
        # kept per evaluation; the rest is scratch that every evaluation overwrites.
        self.offsets = np.zeros(n, np.int32)
        self.offsets[1:] = np.cumsum(self.targets, dtype=np.int64)[:-1]
        self.total = int(self.targets.sum())
        m, cap = max(self.total, 1), self.capacity
        i32, f64 = dict(dtype=t.int32, device=self.device), dict(dtype=t.float64, device=self.device)
        self._kept = dict(count_dev=t.zeros((cap, n), **i32), ep_step_dev=t.zeros((cap, m), **i32),
                          ep_length_dev=t.zeros((cap, m), **i32), ep_return_dev=t.zeros((cap, m), **f64))
        self._scratch = dict(target_dev=t.from_numpy(self.targets).to(self.device), offset_dev=t.from_numpy(self.offsets).to(self.device),
                             length_dev=t.zeros(n, **i32), seen_dev=t.zeros(n, **i32), return_dev=t.zeros(n, **f64),
                             return_raw_dev=t.zeros(n, **f64), short_dev=t.zeros(1, **i32), ep_env_dev=t.zeros(m, **i32),
                             ep_domain_dev=t.zeros(m, **i32), ep_flags_dev=t.zeros(m, **i32), ep_n_elements_dev=t.zeros(m, **i32),
                             ep_archive_dev=t.zeros(m, **i32), ep_return_raw_dev=t.zeros(m, **f64))
        # the history rows, then the state: best_mean, best_eval, last_mean, evaluations
        R, S = _capi.EVAL_ROW_DOUBLES, _capi.EVAL_STATE_DOUBLES
        self._log = t.zeros(cap * R + S, **f64)
        self._log[cap * R:] = t.tensor([-np.inf, -1.0, np.nan, 0.0], **f64)
        self.history, self.state = self._log[:cap * R].view(cap, R), self._log[cap * R:]
        self.improved = t.zeros(1, **i32)
        # the best buffer and the copy table
        self._named = named
        self._offsets, floats = best_layout(named)
        self.best = t.zeros(floats, dtype=t.float32, device=self.device)
        self._entries = self.entries(named, self._offsets)

    @staticmethod
    def entries(named, offsets):
        """The C table of a meshenv_keep_best call: (name, tensor) pairs and the float offset of each in the best buffer."""
        tab = (_capi.MeshKeepEntry * len(named))()
        for e, (_, x), at in zip(tab, named, offsets):
            e.src_dev, e.dst_offset, e.numel = x.data_ptr(), int(at), int(x.numel())
        return tab

    def buffers(self, k: int):
        """The MeshEvalBuffers of evaluation k: its own rows of the kept records, the shared scratch, the eval env's step
        buffers."""
        env = self.eval_venv
        B = _capi.MeshEvalBuffers()
        B.struct_size = C.sizeof(_capi.MeshEvalBuffers)
        for name, x in self._scratch.items():
            setattr(B, name, x.data_ptr())
        for name, x in self._kept.items():
            setattr(B, name, x[k].data_ptr())
        B.obs_dev, B.reward_dev, B.done_dev, B.complete_dev = (x.data_ptr() for x in (env.obs, env.reward, env.done, env.complete))
        return B

    def room(self, evaluations: int = 1) -> None:
        """Refuses, on the host and before anything is enqueued, what the history cannot hold."""
        if self.evaluations + evaluations > self.capacity:
            raise ValueError(f"{self.evaluations} evaluations made and {evaluations} more asked for; capacity = {self.capacity}")

    def evaluate_now(self, policy, num_timesteps: int) -> int:
        """One evaluation of ``policy`` (a FusedActor / FusedPolicy of the model's kind, as it is NOW), stamped
        ``num_timesteps``: the queued evaluation, k_eval_reduce, k_keep_best, all on the current stream; nothing is read back.
        Returns the evaluation's row."""
        k = self.evaluations
        self.room()
        check_policy(self.kind, policy)
        env = self.eval_venv
        if policy.device != self.device:
            raise ValueError(f"policy is on {policy.device}, the eval envs on {self.device}")
        if isinstance(num_timesteps, bool) or not isinstance(num_timesteps, (int, np.integer)) or num_timesteps < 0:
            raise ValueError(f"num_timesteps must be an int >= 0, got {num_timesteps!r}")
        B = self.buffers(k)
        env._bind_stream()
        policy._bind_stream()
        self._bind_stream()
        sac = self.kind == "sac"
        L = self._L
        rc = L.meshenv_evaluate_queued(env._handle, None if sac else policy._h, policy._h if sac else None,
                                       0 if self.deterministic else 1, C.c_uint64(self.eval_seed & MASK64),
                                       C.c_uint64((k * self.eval_steps) & MASK64), self.eval_steps, C.byref(B))
        env._check(rc, "meshenv_evaluate_queued")
        rc = L.meshenv_eval_reduce(self._h, self.n_envs, self.total, C.byref(B), k, self.capacity, float(num_timesteps),
                                   self.history.data_ptr(), self.state.data_ptr(), self.improved.data_ptr())
        self._check(rc, "meshenv_eval_reduce")
        rc = L.meshenv_keep_best(self._h, self._entries, len(self._entries), self.best.data_ptr(), self.best.numel(),
                                 self.improved.data_ptr())
        self._check(rc, "meshenv_keep_best")
        self.evaluations = k + 1
        return k

    def before_collect(self, policy, num_timesteps: int, T: int, n_envs: int) -> int:
        """What ``learn`` calls in front of a collect of T vector steps entered at ``num_timesteps``: the evaluations SB3 would
        make during it, each stamped with SB3's ``num_timesteps`` at its call.  Returns how many were enqueued."""
        points = eval_points(self.n_calls, T, self.eval_freq)
        if points:
            if self.behaviour is not None:
                policy = self.behaviour
                policy.refresh()
            for j in points:
                self.evaluate_now(policy, num_timesteps + j * n_envs)
        self.n_calls += T
        return len(points)

    # ---------------------------------------------------------------- reading
    def read(self, episodes: bool = False) -> dict:
        """ONE device-to-host copy: the history of the evaluations made so far, by column (``timesteps`` int64 and COLUMNS[1:],
        float64 except the integer counts and ``improved``), ``best_mean_reward`` (-inf before the first improvement),
        ``best_eval`` (-1), ``last_mean_reward`` (NaN before the first evaluation) and ``evaluations``.  episodes=True adds SB3's
        per-episode ``results`` and ``ep_lengths`` ([evaluations, episodes], SB3's order; see ``save_npz``) at the price of
        four more copies."""
        R = _capi.EVAL_ROW_DOUBLES
        host = self._log.cpu().numpy()
        E = self.evaluations
        rows, state = host[:self.capacity * R].reshape(self.capacity, R)[:E], host[self.capacity * R:]
        out = {"timesteps": rows[:, 0].astype(np.int64)}
        for c, name in enumerate(COLUMNS):
            if c:
                out[name] = rows[:, c].astype(np.int64) if name in ("recorded", "short") else rows[:, c].astype(bool) if name == "improved" else rows[:, c].copy()
        out.update(best_mean_reward=float(state[0]), best_eval=int(state[1]), last_mean_reward=float(state[2]), evaluations=E)
        if episodes:
            out["results"], out["ep_lengths"] = self.episodes()
        return out

    def episodes(self):
        """(results float64 [evaluations, episodes], ep_lengths int64 [evaluations, episodes]): every evaluation's recorded
        episodes in SB3's order (step, then env), then NaN / 0 for the episodes that did not end within eval_steps."""
        E, n, total = self.evaluations, self.n_envs, self.total
        kept = {k: v[:E].cpu().numpy() for k, v in self._kept.items()}
        owner = np.repeat(np.arange(n), self.targets)
        results, lengths = np.full((E, total), np.nan), np.zeros((E, total), np.int64)
        for e in range(E):
            keep = (np.arange(total) - self.offsets[owner]) < np.minimum(kept["count_dev"][e], self.targets)[owner]
            order = sb3_order(kept["ep_step_dev"][e][:total][keep], owner[keep])
            results[e, :len(order)] = kept["ep_return_dev"][e][:total][keep][order]
            lengths[e, :len(order)] = kept["ep_length_dev"][e][:total][keep][order]
        return results, lengths

    def save_npz(self, path) -> None:
        """``evaluations.npz`` in the reference's layout: ``timesteps`` [E], ``results`` [E, episodes], ``ep_lengths``
        [E, episodes].  An evaluation whose episodes all ended within eval_steps fills its row as SB3 does; a shorter one ends
        in NaN / 0."""
        got = self.read(episodes=True)
        np.savez(path, timesteps=got["timesteps"], results=got["results"], ep_lengths=got["ep_lengths"])

    # ---------------------------------------------------------------- the best model
    def best_state(self) -> dict:
        """name -> view of the best buffer, shaped as the live tensor.  Zeros until an evaluation improved."""
        return {name: self.best[at:at + x.numel()].view(x.shape) for (name, x), at in zip(self._named, self._offsets)}

    def load_best(self, model=None) -> None:
        """The kept parameters into the live tensors of ``model`` (the callback's own by default): a host call, made outside
        ``learn``.  The caller then calls ``refresh()`` on its behaviours (and on a FusedTDTarget it drives by hand).  The
        optimiser state is left as it is."""
        t = self._torch
        kind, named = snapshot_set(model if model is not None else self.model)
        if kind != self.kind or [(k, tuple(x.shape)) for k, x in named] != [(k, tuple(x.shape)) for k, x in self._named]:
            raise ValueError("load_best: the model's snapshot set differs from the one kept")
        if int(self.state[1].item()) < 0:
            raise ValueError("load_best: no evaluation has improved on -inf yet; nothing was kept")
        best = self.best_state()
        with t.no_grad():
            for name, x in named:
                x.copy_(best[name])
