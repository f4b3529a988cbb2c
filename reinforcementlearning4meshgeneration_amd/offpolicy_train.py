"""The body of SB3 2.x's ``SAC.train(gradient_steps, batch_size)`` / ``TD3.train(...)`` as ONE call into the library
(include/meshenv_offpolicy_train.h, csrc/meshenv_offpolicy_train.h: k_optim_step_noted, k_offpolicy_finish;
csrc/meshenv_replay.h: k_replay_sample_batches):

    SAC   for gradient_step in range(gradient_steps):
              sample; ent_coef = exp(log_ent_coef.detach()); the entropy-coefficient step; TD target;
              critic loss and step; actor loss and step
              if gradient_step % target_update_interval == 0: polyak_update(critic, critic_target, tau)
          _n_updates += gradient_steps
    TD3   for _ in range(gradient_steps):
              _n_updates += 1; sample; target with clipped noise; critic loss and step
              if _n_updates % policy_delay == 0: actor loss and step; polyak_update of critic and actor

``FusedOffPolicyTrain.train(gradient_steps)`` enqueues every launch of every gradient step (per chunk of steps one draw of all
their minibatches, per step the launches of ``FusedTDTarget.target``, ``FusedCriticGrad.backward``, the critic step and, on
actor steps, the actor backward and the actor program, and ``FusedTDTarget.refresh``; then the log kernel) and returns.
Nothing is read back: which steps update the actor and the targets, and so every optimiser's ``step`` afterwards, is known on
the host before the call.  The order inside a step is the one examples/sac_train_step.py composes from the same classes (the
entropy-coefficient step travels with the actor step, after the actor backward has read the unstepped ``log_ent_coef``; the
target reads the snapshot of the previous refresh), and the call reproduces that composition bit for bit.

    tr = FusedOffPolicyTrain.from_sb3(model, replay_buffer)     # replay_buffer: the DeviceReplayBuffer
    logs = tr.train(gradient_steps)                             # queued; logs.device is the [8] float64 tensor on the GPU
    print(logs.read())                                          # one copy: SB3's train/... keys as Python floats

Step k of a call draws its minibatch (Philox tag 1), its target noise (tag 2) and its actor noise (tag 3) at
``(seed, counter + k)``; ``counter`` continues from the handle's running count, so two ``train()`` calls never reuse a draw,
and ``seed`` defaults to ``DEFAULT_SEED`` = 0.

The functions of this module that take no device (``hyper``, ``sac_polyak_schedule``, ``td3_actor_schedule``,
``actor_programs``, ``pick_chunk``, ``check_gradient_steps``, ``draw_counters``, ``OffPolicyTrainSpec``) are the host half: every refusal is made by them or by the
classes this one drives."""
from __future__ import annotations

import ctypes as C
from typing import List, Optional

from . import _capi
from ._handle import Handle
from .actor_grad import ActorGradSpec, FusedActorGrad
from .critic_grad import CriticGradSpec, FusedCriticGrad
from .onpolicy_train import scalar_sets, step_values, update_learning_rate  # noqa: F401  (step_values: part of this module's interface)
from .optim_step import PROGRAMS, FusedOptimStep, OptimStepSpec
from .replay import DeviceReplayBuffer
from .sb3_nets import KIND_SAC
from .td3_actor_grad import FusedTD3ActorGrad, TD3ActorGradSpec
from .td_target import FusedTDTarget, TDTargetSpec

OUTPUTS = ("critic_loss", "actor_loss", "ent_coef_loss", "ent_coef", "gradient_steps", "actor_steps", "polyak_updates",
           "last_critic_loss")                            # meshenv_offpolicy_train.h's enum
COUNTS = ("gradient_steps", "actor_steps", "polyak_updates")
MAX_STEPS = _capi.OFFTRAIN_MAX_STEPS
SAMPLE_FLOATS = _capi.OFFTRAIN_SAMPLE_FLOATS              # 18 + 3 + 18 + 1 + 1 per sample
SAMPLE_WORKSPACE_BYTES = 64 << 20                         # the cap on the sample workspace of one train()
DEFAULT_SEED = 0
MASK64 = 2 ** 64 - 1


def _positive_int(value, what) -> int:
    if isinstance(value, bool) or not isinstance(value, int) or value < 1:
        raise ValueError(f"{what} must be a positive int, got {value!r}")
    return value


def hyper(model, sac: bool, batch_size=None) -> dict:
    """What ``SAC.train`` / ``TD3.train`` read from the model at the call: ``batch_size`` (the argument wins, as SB3's does),
    ``target_update_interval`` (SAC, default 1), ``policy_delay`` (TD3, default 2) and ``_n_updates`` (default 0)."""
    batch = getattr(model, "batch_size", None) if batch_size is None else batch_size
    if batch is None:
        raise ValueError("no batch_size: the model has none and none was passed")
    n_updates = getattr(model, "_n_updates", 0)
    if isinstance(n_updates, bool) or not isinstance(n_updates, int) or n_updates < 0:
        raise ValueError(f"_n_updates must be an int >= 0, got {n_updates!r}")
    hp = dict(batch_size=_positive_int(batch, "batch_size"), n_updates=n_updates)
    if sac:
        hp["target_update_interval"] = _positive_int(getattr(model, "target_update_interval", 1), "target_update_interval")
    else:
        hp["policy_delay"] = _positive_int(getattr(model, "policy_delay", 2), "policy_delay")
    return hp


def sac_polyak_schedule(K: int, target_update_interval: int) -> List[bool]:
    """Per gradient step of one ``SAC.train``: does it end with polyak_update?  ``gradient_step % target_update_interval == 0``
    with the index inside the call, not ``_n_updates``."""
    return [k % target_update_interval == 0 for k in range(K)]


def td3_actor_schedule(K: int, policy_delay: int, n_updates: int) -> List[bool]:
    """Per gradient step of one ``TD3.train`` entered at ``_n_updates = n_updates``: does it update the actor and the targets?
    ``_n_updates`` is incremented first, so step k tests ``(n_updates + k + 1) % policy_delay == 0``."""
    return [(n_updates + k + 1) % policy_delay == 0 for k in range(K)]


def actor_programs(sac: bool, K: int, hp: dict) -> List[int]:
    """meshenv_offpolicy_train_run's ``actor_program``: per step the index of the FusedOptimStep program of its actor step, or
    -1.  SAC steps the actor (and the entropy coefficient) every step, with the Polyak update on the scheduled ones; TD3 steps
    actor and targets together on the delayed steps."""
    with_polyak, alone = PROGRAMS.index("actor_polyak"), PROGRAMS.index("actor")
    if sac:
        return [with_polyak if p else alone for p in sac_polyak_schedule(K, hp["target_update_interval"])]
    return [with_polyak if a else -1 for a in td3_actor_schedule(K, hp["policy_delay"], hp["n_updates"])]


def pick_chunk(K: int, batch: int, cap_bytes: int = SAMPLE_WORKSPACE_BYTES) -> int:
    """Gradient steps whose minibatches one draw fetches: as many as fit ``cap_bytes`` of sample workspace, at least one."""
    return max(1, min(K, cap_bytes // (batch * SAMPLE_FLOATS * 4)))


def check_gradient_steps(gradient_steps) -> int:
    """``gradient_steps`` of one call: an int in [1, MAX_STEPS]."""
    K = gradient_steps
    if isinstance(K, bool) or not isinstance(K, int) or K < 1:
        raise ValueError(f"gradient_steps must be a positive int, got {gradient_steps!r} (SB3's -1 is the caller's to resolve)")
    if K > MAX_STEPS:
        raise ValueError(f"{K} gradient steps; at most {MAX_STEPS} per train()")
    return K


def draw_counters(running: int, counter, K: int):
    """(the counter of a call's first step, the running count it leaves): ``counter`` None continues from ``running``; both
    wrap modulo 2^64 as the kernels' 64-bit add does."""
    first = (running if counter is None else int(counter)) & MASK64
    return first, (first + K) & MASK64


class OffPolicyTrainSpec:
    """The host half: the four specs a train() drives, built from an SB3-shaped SAC / TD3 model, with their refusals (batch
    norm, ``n_critics != 2``, other architectures, the optimisers' classes and flags) and this call's own (gSDE,
    ``optimize_memory_usage``, a ``VecNormalize`` wrapper).  SAC or TD3 is what ``TDTargetSpec.from_sb3`` recognises."""

    def __init__(self, model, target: Optional[TDTargetSpec] = None, critic: Optional[CriticGradSpec] = None, actor=None,
                 optim: Optional[OptimStepSpec] = None):
        self.model = model
        name = type(model).__name__
        if getattr(model, "use_sde", False) or getattr(getattr(model, "actor", None), "use_sde", False):
            raise ValueError(f"{name}.use_sde=True (gSDE) is not supported: the actor's noise is the state-independent Gaussian")
        if getattr(model, "optimize_memory_usage", False):
            raise ValueError(f"{name}.optimize_memory_usage=True is not supported: next_observations are stored (SB3's default)")
        if getattr(model, "_vec_normalize_env", None) is not None:
            raise ValueError(f"{name} has a _vec_normalize_env (VecNormalize): the samples are not normalised")
        self.target = TDTargetSpec.from_sb3(model) if target is None else target
        self.sac = self.target.kind == KIND_SAC
        self.critic = CriticGradSpec.from_sb3(model) if critic is None else critic
        if actor is None:
            actor = ActorGradSpec.from_sb3(model) if self.sac else TD3ActorGradSpec.from_sb3(model)
        self.actor = actor
        if self.critic.kind != self.target.kind or isinstance(actor, ActorGradSpec) != self.sac:
            raise ValueError("the target, critic-gradient and actor-gradient specs are not of one algorithm")
        self.optim = OptimStepSpec.from_sb3(model) if optim is None else optim
        if self.optim.critic is None or not self.optim.actor:
            raise ValueError("the optimiser spec has no critic or no actor optimiser: FusedOffPolicyTrain steps both")
        self.learned = self.sac and actor.log_ent_coef is not None
        stepped = {id(p) for p in self.optim.critic.param_groups[0]["params"]}
        if stepped != {id(p) for p in self.critic.tensors()}:
            raise ValueError("the critic optimiser's parameters are not the tensors FusedCriticGrad writes gradients for")
        stepped = {id(p) for opt in self.optim.actor for p in opt.param_groups[0]["params"]}
        grads = actor.grad_tensors() if self.sac else list(actor.actor)
        if stepped != {id(p) for p in grads}:
            raise ValueError("the actor-step optimisers' parameters are not the tensors the actor backward writes gradients for")
        if self.learned and any(p is actor.log_ent_coef for p in self.optim.critic.param_groups[0]["params"]):
            raise ValueError("the critic optimiser steps log_ent_coef: the noted critic step reads it")
        hyper(model, self.sac, getattr(model, "batch_size", None) or 1)

    @classmethod
    def from_sb3(cls, model) -> "OffPolicyTrainSpec":
        return cls(model)

    def check_device(self, device) -> None:
        self.target.check_device(device)

    def optimizers(self):
        return [self.optim.critic] + list(self.optim.actor)


def check_replay_buffer(replay_buffer, device) -> DeviceReplayBuffer:
    if not isinstance(replay_buffer, DeviceReplayBuffer):
        raise ValueError(f"replay_buffer is {type(replay_buffer).__name__}, not a DeviceReplayBuffer: the minibatches are drawn on the device")
    if getattr(replay_buffer, "optimize_memory_usage", False):
        raise ValueError("replay_buffer.optimize_memory_usage=True is not supported")
    if device is not None and replay_buffer.device != device:
        raise ValueError(f"replay_buffer is on {replay_buffer.device}, not on {device}")
    return replay_buffer


class OffPolicyTrainLogs:
    """What a ``train()`` leaves: ``device`` is the [8] float64 tensor on the GPU (``OUTPUTS``' order), ``read()`` the log
    dictionary under SB3's key names."""

    def __init__(self, device, sac: bool, learned: bool, n_updates: int):
        self.device = device
        self._sac, self._learned = sac, learned
        self.n_updates = n_updates
        self._host = None

    def values(self) -> dict:
        """OUTPUTS' names -> Python floats (the counts as ints): one copy, kept."""
        if self._host is None:
            self._host = self.device.cpu().tolist()
        return {k: int(v) if k in COUNTS else v for k, v in zip(OUTPUTS, self._host)}

    def read(self) -> dict:
        """SB3's ``logger.record`` keys of ``SAC.train`` (``TD3.train``) as Python floats: ``train/n_updates``,
        ``train/critic_loss``, ``train/actor_loss`` (TD3: only when an actor step ran), ``train/ent_coef`` and, with a learned
        coefficient, ``train/ent_coef_loss``; and ``gradient_steps``, ``actor_steps``, ``polyak_updates``,
        ``last_critic_loss`` under their own names."""
        v = self.values()
        logs = {"train/n_updates": self.n_updates}
        if self._sac:
            logs["train/ent_coef"] = v["ent_coef"]
        if v["actor_steps"] > 0:
            logs["train/actor_loss"] = v["actor_loss"]
        logs["train/critic_loss"] = v["critic_loss"]
        if self._learned:
            logs["train/ent_coef_loss"] = v["ent_coef_loss"]
        logs.update({k: v[k] for k in COUNTS + ("last_critic_loss",)})
        return logs


class FusedOffPolicyTrain(Handle):
    """``train(gradient_steps)``: one C call per ``SAC.train()`` / ``TD3.train()``.  Drives a FusedTDTarget, a FusedCriticGrad,
    a FusedActorGrad or FusedTD3ActorGrad, a FusedOptimStep and the DeviceReplayBuffer; all stay usable on their own."""
    PREFIX = "meshenv_offpolicy_train"

    def __init__(self, spec: OffPolicyTrainSpec, replay_buffer, td=None, cg=None, ag=None, fo=None, device: int = 0):
        self.spec, self.model = spec, spec.model
        check_replay_buffer(replay_buffer, None)
        super().__init__(device, check_device=spec.check_device)
        self.buffer = check_replay_buffer(replay_buffer, self.device)
        self._owned = []              # the handles built here: close() closes them with this one
        self.td = td if td is not None else self._own(FusedTDTarget(spec.target, device))
        self.cg = cg if cg is not None else self._own(FusedCriticGrad(spec.critic, device))
        if ag is None:
            ag = self._own(FusedActorGrad(spec.actor, device) if spec.sac else FusedTD3ActorGrad(spec.actor, device))
        self.ag = ag
        self.fo = fo if fo is not None else self._own(FusedOptimStep(spec.optim, device))
        for name, h in (("td", self.td), ("cg", self.cg), ("ag", self.ag), ("fo", self.fo)):
            if h.device != self.device:
                raise ValueError(f"{name} is on {h.device}, not on {self.device}")
        self.calls = 0                # C calls so far: one per train()
        self.counter = 0              # the running count of gradient steps drawn: the next train()'s default counter
        self._kept = {}               # program -> the plan and the objects it was checked on (_prepared)
        self._work = None             # the sample workspace: (chunk, batch, five stacked tensors, the [batch] target buffer)

    def _own(self, h):
        self._owned.append(h)
        return h

    def close(self):
        super().close()               # waits for the stream the launches went to
        for h in getattr(self, "_owned", []):
            h.close()
        self._owned = []

    @classmethod
    def from_sb3(cls, model, replay_buffer, td=None, cg=None, ag=None, fo=None, device: int = 0):
        """model: SB3 2.x's SAC / TD3 or anything shaped like it.  replay_buffer: the DeviceReplayBuffer its rollouts fill.
        td, cg, ag, fo: a FusedTDTarget / FusedCriticGrad / FusedActorGrad (TD3: FusedTD3ActorGrad) / FusedOptimStep of the
        caller's for the same model, or None to build them.  Refuses, by name, what those classes refuse."""
        spec = OffPolicyTrainSpec(model, None if td is None else td.spec, None if cg is None else cg.spec,
                                  None if ag is None else ag.spec, None if fo is None else fo.spec)
        return cls(spec, replay_buffer, td, cg, ag, fo, device)

    # ---------------------------------------------------------------- the checked plans
    def _prepared(self, program: str):
        """(plan, its key) of a program: ``_attach`` and ``OptimStepSpec.prepare``, whose checks look at every gradient and
        state tensor.  A plan is kept and handed out again while every OBJECT it was made from is still the one in place (each
        param group, each ``p.grad``, each state dict and the tensors in it), the groups' scalars are still Python floats and
        the ``step`` values of an optimiser still agree; anything else (a ``load_state_dict``, a gradient of the caller's, a
        new state entry) goes through the checks again."""
        fo = self.fo
        opts = fo.spec._optimizers_of(program)
        kept = self._kept.get(program)
        if kept is not None:
            plan, key, per_opt = kept
            ok = True
            for opt, (group, items) in zip(opts, per_opt):
                groups = opt.param_groups
                ok = len(groups) == 1 and groups[0] is group and fo.spec._group(opt, "an optimiser") is group
                ok = ok and type(group["lr"]) is float and type(group["eps"]) is float and all(type(b) is float for b in group["betas"])
                if not ok:
                    break
                state, step0 = opt.state, items[0][4].item()
                for p, grad, st, tensors, step in items:
                    if p.grad is not grad or state.get(p) is not st or len(st) != 3 or st["step"] is not step or step.item() != step0 or \
                            any(st[k] is not x for k, x in tensors):
                        ok = False
                        break
                if not ok:
                    break
            if ok:
                return plan, key
        self._kept.pop(program, None)
        self.cg._attach()
        self.ag._attach()
        plan = fo.spec.prepare(program)
        key = plan.key()
        per_opt, keep = [], True
        for opt in opts:
            group = opt.param_groups[0]
            if "betas" not in group:               # RMSprop: not an off-policy recipe; checked every call
                keep = False
                break
            items = [(p, p.grad, opt.state[p], tuple((k, opt.state[p][k]) for k in ("exp_avg", "exp_avg_sq")), opt.state[p]["step"])
                     for p in group["params"]]
            keep = keep and all(len(st) == 3 for _, _, st, _, _ in items)
            per_opt.append((group, items))
        if keep:
            self._kept[program] = (plan, key, per_opt)
        return plan, key

    def _workspace(self, chunk: int, batch: int):
        w = self._work
        if w is None or w[0] < chunk or w[1] != batch:
            t = self._torch
            stacked = self.buffer._stacked(chunk, batch)
            self._work = w = (chunk, batch, stacked, t.empty(batch, dtype=t.float32, device=self.device))
        return w

    # ---------------------------------------------------------------- public
    def train(self, gradient_steps: int, batch_size: Optional[int] = None, seed: Optional[int] = None, counter: Optional[int] = None,
              sample_chunk: Optional[int] = None) -> OffPolicyTrainLogs:
        """The whole of ``train(gradient_steps, batch_size)``.  batch_size: None reads ``model.batch_size``.  seed: None is
        ``DEFAULT_SEED``; counter: None continues from the handle's running count (``self.counter``), which the call leaves at
        ``counter + gradient_steps``.  sample_chunk: how many steps' minibatches one draw fetches; None fills a workspace of
        at most ``SAMPLE_WORKSPACE_BYTES``."""
        t, model, spec, fo = self._torch, self.model, self.spec, self.fo
        K = check_gradient_steps(gradient_steps)
        sac = spec.sac
        hp = hyper(model, sac, batch_size)
        batch = hp["batch_size"]
        buf = self.buffer
        if buf.size() < 1:
            raise ValueError("cannot train from an empty replay buffer")
        for opt in spec.optimizers():                    # _update_learning_rate(optimizers)
            update_learning_rate(model, opt)
        seed = DEFAULT_SEED if seed is None else int(seed)
        counter, counter_after = draw_counters(self.counter, counter, K)
        chunk = pick_chunk(K, batch) if sample_chunk is None else _positive_int(sample_chunk, "sample_chunk")
        chunk = min(chunk, K)
        if chunk * batch > _capi.REPLAY_BATCHES_MAX_SAMPLES:
            raise ValueError(f"sample_chunk {chunk} x batch {batch} exceeds {_capi.REPLAY_BATCHES_MAX_SAMPLES} samples per draw")
        programs = actor_programs(sac, K, hp)
        used = sorted({p for p in programs if p >= 0})
        n_actor = sum(p >= 0 for p in programs)
        # prepare's checks once per program; the scalar sets from the state as it is
        plans = {"critic": self._prepared("critic")}
        for p in used:
            plans[PROGRAMS[p]] = self._prepared(PROGRAMS[p])
        stream = t.cuda.current_stream(self.device).cuda_stream
        for h in (self, self.td, self.cg, self.ag, fo):
            if h._stream != stream:
                h._bind_stream()
        buf._venv._bind_stream()
        for name, (plan, key) in plans.items():
            if fo._bound.get(name) != key:
                fo._bind(plan, key)
        critic_sets, critic_values = scalar_sets(fo.spec, plans["critic"][0], K)
        actor_sets, actor_values, actor_plan = None, [], None
        if n_actor:
            actor_plan = plans[PROGRAMS[used[0]]][0]     # "actor" and "actor_polyak" step the same optimisers
            actor_sets, actor_values = scalar_sets(fo.spec, actor_plan, n_actor)
        _, _, stacked, target = self._workspace(chunk, batch)
        out_dev = t.empty(_capi.OFFTRAIN_OUTPUTS, dtype=t.float64, device=self.device)
        ag = self.ag
        rc = self._L.meshenv_offpolicy_train_run(
            self._h, buf._venv._handle, self.td._h, self.cg._h, ag._h if sac else None, None if sac else ag._h, fo._h,
            PROGRAMS.index("critic"), buf.store.data_ptr(), buf.rows, buf.size(), batch, K, C.c_uint64(seed & MASK64),
            C.c_uint64(counter & MASK64), self._ptrs(stacked), chunk, target.data_ptr(), (C.c_int32 * K)(*programs), critic_sets,
            actor_sets, n_actor, out_dev.data_ptr())
        self._check(rc, "meshenv_offpolicy_train_run")
        self.calls += 1
        self.counter = counter_after
        # every optimiser's step, known on the host: nothing is read back
        for (g, step_tensors), vals in zip(plans["critic"][0].groups, critic_values):
            for s in step_tensors:
                s.fill_(vals[K])
        if n_actor:
            for (g, step_tensors), vals in zip(actor_plan.groups, actor_values):
                for s in step_tensors:
                    s.fill_(vals[n_actor])
        model._n_updates = hp["n_updates"] + K
        return OffPolicyTrainLogs(out_dev, sac, spec.learned, model._n_updates)
