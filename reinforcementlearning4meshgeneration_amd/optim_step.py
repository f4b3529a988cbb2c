"""The optimiser steps and the Polyak update of SB3's ``SAC.train`` / ``TD3.train`` on the GPU (include/meshenv_optim.h:
meshenv_optim_*, csrc/meshenv_optim.h: k_optim_step): the statements that follow the two ``backward`` calls,

    self.critic.optimizer.step()
    self.actor.optimizer.step();  self.ent_coef_optimizer.step()
    polyak_update(self.critic.parameters(), self.critic_target.parameters(), self.tau)      # TD3: the actor's too

as two launches: ``critic_step()`` and ``actor_step(polyak=True)``; and the one statement of ``PPO.train`` / ``A2C.train``,

    self.policy.optimizer.step()

as one: ``policy_step()``, for PPO's Adam and for A2C's default ``torch.optim.RMSprop(alpha=0.99, eps=1e-5)`` (momentum = 0,
not centered: ``torch.optim.rmsprop._single_tensor_rmsprop``; its ``square_avg`` is updated in place like Adam's moments).
The kernel applies torch's Adam (the order of operations
of ``torch.optim.adam._single_tensor_adam``, non-capturable) IN PLACE to the live parameters and to the optimiser's OWN state
tensors (``exp_avg``, ``exp_avg_sq``; ``step`` is incremented on the host), so ``optimizer.state_dict()``,
``load_state_dict()`` and a stock ``optimizer.step()`` in between keep working, and applies ``t = t (1 - tau) + tau p`` to the
target networks.  ``p.grad`` is read and never written: zeroing it stays the caller's, and ``FusedTDTarget.refresh()`` stays a
call of its own.

``OptimStepSpec`` is the host half (the bound optimisers, the Polyak pairs, the segment table, the scalars of a step and every
refusal; no device needed).  The bias corrections are computed on the host in doubles from the incremented step, exactly as
torch does, and travel as kernel arguments; ``lr`` is read from ``param_groups[0]`` at every call."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

from . import _capi
from ._handle import Handle
from .sb3_nets import check_device

CHUNK = _capi.OPTIM_CHUNK            # elements per workgroup
THREADS = 256
ADAM, POLYAK, ADAM_POLYAK, RMSPROP = _capi.OPTIM_ADAM, _capi.OPTIM_POLYAK, _capi.OPTIM_ADAM_POLYAK, _capi.OPTIM_RMSPROP
PROGRAMS = ("critic", "actor_polyak", "actor", "polyak", "policy")      # meshenv_optim_bind's program index
SUPPORTED = ("torch.optim.Adam with one param group, float32 contiguous parameters, and none of amsgrad, maximize, "
             "weight_decay, capturable, differentiable, decoupled_weight_decay, fused")
_FLAGS = ("amsgrad", "maximize", "capturable", "differentiable", "decoupled_weight_decay", "fused")
SUPPORTED_RMSPROP = ("torch.optim.RMSprop with one param group, float32 contiguous parameters, momentum = 0, and none of centered, "
                     "weight_decay, maximize, capturable, differentiable")
_FLAGS_RMSPROP = ("centered", "maximize", "capturable", "differentiable")


def adam_scalars(step: float, lr: float, beta1: float, beta2: float) -> Tuple[float, float]:
    """(step_size, bias_correction2_sqrt) of ``_single_tensor_adam`` at the incremented ``step``, in Python doubles and in
    torch's own expressions."""
    bias_correction1 = 1 - beta1 ** step
    bias_correction2 = 1 - beta2 ** step
    step_size = lr / bias_correction1
    bias_correction2_sqrt = bias_correction2 ** 0.5
    return step_size, bias_correction2_sqrt


def _is_rmsprop(opt) -> bool:
    import torch
    return type(opt) is torch.optim.RMSprop


@dataclass
class Segment:
    """One tensor of a launch: what meshenv_optim_bind takes per segment."""
    op: int
    block: int                       # which optimiser of the launch (the block of scalars it reads)
    param: object
    target: Optional[object] = None
    name: str = ""

    @property
    def n(self) -> int:
        return int(self.param.numel())


@dataclass
class Row:
    """A segment with the tensors of this call: (param, grad, exp_avg, exp_avg_sq, target), None where the op takes none
    (RMSprop: its square_avg travels as exp_avg_sq and there is no exp_avg)."""
    seg: Segment
    tensors: tuple

    @property
    def pointers(self) -> tuple:
        return tuple(0 if t is None else t.data_ptr() for t in self.tensors)

    @property
    def vec(self) -> int:
        """1 when every pointer is 16-byte aligned: the kernel's 128-bit path; decided per segment, never assumed."""
        return int(all(q % 16 == 0 for q in self.pointers))


@dataclass
class Plan:
    program: str
    rows: List[Row]
    groups: list                     # per optimiser of the launch: (param group, [step tensors])

    def key(self) -> tuple:
        return tuple(r.pointers for r in self.rows)


class OptimStepSpec:
    """critic: the optimiser ``critic_step`` runs (or None); actor: the optimisers ``actor_step`` runs, in order (SAC: the
    actor's and the entropy coefficient's); polyak: [(source parameters, target parameters)]; tau in [0, 1]; policy: the
    optimiser ``policy_step`` runs (PPO / A2C: ``model.policy.optimizer``).  Every slot takes a torch.optim.Adam or a
    torch.optim.RMSprop."""

    def __init__(self, critic=None, actor: Sequence = (), polyak: Sequence = (), tau: float = 0.005, policy=None):
        self.critic = critic
        self.policy = policy
        self.actor = list(actor)
        if len(self.actor) > _capi.OPTIM_BLOCKS:
            raise ValueError(f"{len(self.actor)} optimisers in one launch; at most {_capi.OPTIM_BLOCKS}")
        self.tau = tau
        for i, opt in enumerate(self.optimizers()):
            self._check_optimizer(opt, self._opt_name(opt))
        self.pairs = []               # [(source, target)]
        for k, (src, dst) in enumerate(polyak):
            src, dst = list(src), list(dst)
            if len(src) != len(dst):
                raise ValueError(f"polyak pair {k}: {len(src)} parameters but {len(dst)} target parameters")
            for i, (p, t) in enumerate(zip(src, dst)):
                if tuple(p.shape) != tuple(t.shape):
                    raise ValueError(f"polyak pair {k}, tensor {i}: parameter {tuple(p.shape)} but target {tuple(t.shape)}")
                self._check_tensor(p, f"polyak pair {k}, parameter {i}")
                self._check_tensor(t, f"polyak pair {k}, target {i}")
                self.pairs.append((p, t))
        seen_s, seen_t = set(), set()
        stepped = {id(p) for opt in self.optimizers() for p in opt.param_groups[0]["params"]}
        for p, t in self.pairs:
            if id(p) in seen_s or id(t) in seen_t or p is t:
                raise ValueError("a tensor appears twice among the Polyak pairs")
            if id(t) in stepped:
                raise ValueError("a Polyak target is also a parameter of a bound optimiser")
            seen_s.add(id(p))
            seen_t.add(id(t))
        self._segments = {name: self._build(name) for name in PROGRAMS}

    # ---------------------------------------------------------------- tau
    @property
    def tau(self) -> float:
        return self._tau

    @tau.setter
    def tau(self, value):
        v = float(value)
        if not 0.0 <= v <= 1.0:                      # NaN fails both comparisons
            raise ValueError(f"tau must lie in [0, 1], got {value!r}")
        self._tau = v

    # ---------------------------------------------------------------- refusals
    def optimizers(self):
        return ([self.critic] if self.critic is not None else []) + self.actor + ([self.policy] if self.policy is not None else [])

    def _opt_name(self, opt) -> str:
        if opt is self.critic:
            return "the critic optimiser"
        if opt is self.policy:
            return "the policy optimiser"
        return f"actor-step optimiser {[id(o) for o in self.actor].index(id(opt))}"

    @staticmethod
    def _check_tensor(p, what) -> None:
        import torch
        if p.dtype != torch.float32:
            raise ValueError(f"{what} of shape {tuple(p.shape)} is {str(p.dtype).replace('torch.', '')}, not float32; supported: {SUPPORTED}")
        if not p.is_contiguous():
            raise ValueError(f"{what} of shape {tuple(p.shape)} is not contiguous; supported: {SUPPORTED}")
        if p.numel() == 0:
            raise ValueError(f"{what} of shape {tuple(p.shape)} has no elements")

    @classmethod
    def _group(cls, opt, name):
        """param_groups[0] after the checks that a later ``add_param_group`` or an edited flag would break."""
        groups = opt.param_groups
        if _is_rmsprop(opt):
            if len(groups) != 1:
                raise ValueError(f"{name} has {len(groups)} param groups; supported: {SUPPORTED_RMSPROP}")
            g = groups[0]
            if g.get("momentum", 0) != 0:
                raise ValueError(f"{name} has momentum={g['momentum']!r}; supported: {SUPPORTED_RMSPROP}")
            for flag in _FLAGS_RMSPROP:
                if g.get(flag):
                    raise ValueError(f"{name} has {flag}={g[flag]!r}; supported: {SUPPORTED_RMSPROP}")
            if g.get("weight_decay", 0) != 0:
                raise ValueError(f"{name} has weight_decay={g['weight_decay']!r}; supported: {SUPPORTED_RMSPROP}")
            return g
        if len(groups) != 1:
            raise ValueError(f"{name} has {len(groups)} param groups; supported: {SUPPORTED}")
        g = groups[0]
        for flag in _FLAGS:
            if g.get(flag):
                raise ValueError(f"{name} has {flag}={g[flag]!r}; supported: {SUPPORTED}")
        if g.get("weight_decay", 0) != 0:
            raise ValueError(f"{name} has weight_decay={g['weight_decay']!r}; supported: {SUPPORTED}")
        return g

    @classmethod
    def _check_optimizer(cls, opt, name) -> None:
        import torch
        if type(opt) is not torch.optim.Adam and not _is_rmsprop(opt):
            raise ValueError(f"{name} is {type(opt).__module__}.{type(opt).__name__}, not torch.optim.Adam or torch.optim.RMSprop; "
                             f"supported: {SUPPORTED}; or {SUPPORTED_RMSPROP}")
        g = cls._group(opt, name)
        for i, p in enumerate(g["params"]):
            cls._check_tensor(p, f"{name}: parameter {i}")

    # ---------------------------------------------------------------- the segment table
    def _build(self, program) -> List[Segment]:
        target_of = {id(p): t for p, t in self.pairs}
        if program == "critic":
            opts, polyak = ([self.critic] if self.critic is not None else []), False
        elif program == "policy":
            opts, polyak = ([self.policy] if self.policy is not None else []), False
        elif program == "polyak":
            opts, polyak = [], True
        else:
            opts, polyak = self.actor, program == "actor_polyak"
        segs, fused = [], set()
        for b, opt in enumerate(opts):
            for i, p in enumerate(opt.param_groups[0]["params"]):
                t = target_of.get(id(p)) if polyak else None
                if t is not None:
                    if _is_rmsprop(opt):             # a target must see the stepped value; no such op is built
                        raise ValueError(f"{self._opt_name(opt)}: parameter {i} is stepped by RMSprop and is a Polyak source; there is "
                                         "no RMSprop + Polyak launch")
                    fused.add(id(p))
                op = RMSPROP if _is_rmsprop(opt) else ADAM if t is None else ADAM_POLYAK
                segs.append(Segment(op, b, p, t, f"optimiser {b} parameter {i}"))
        if polyak:
            # a source stepped by this launch is updated by the thread that stepped it; every other pair is a segment of its
            # own and reads what earlier launches left (critic -> critic_target after critic_step)
            segs += [Segment(POLYAK, 0, p, t, f"polyak pair {i}") for i, (p, t) in enumerate(self.pairs) if id(p) not in fused]
        return segs

    def segments(self, program: str) -> List[Segment]:
        return self._segments[program]

    @staticmethod
    def jobs(rows) -> List[Tuple[int, int]]:
        """[(segment, first element)] per workgroup, as meshenv_optim_bind lays them out: CHUNK elements of one segment each."""
        return [(i, first) for i, r in enumerate(rows) for first in range(0, r.seg.n, CHUNK)]

    @staticmethod
    def thread_elements(row: Row, first: int, tid: int) -> List[int]:
        """The elements thread ``tid`` of the workgroup at (row, first) owns: k_optim_step's mapping, restated."""
        n = row.seg.n
        if row.vec:
            return list(range(first + 4 * tid, min(first + 4 * tid + 4, n)))
        return list(range(first + tid, min(first + CHUNK, n), THREADS))

    # ---------------------------------------------------------------- one call, host side
    def _optimizers_of(self, program):
        if program == "critic":
            return [self.critic] if self.critic is not None else []
        if program == "policy":
            return [self.policy] if self.policy is not None else []
        return [] if program == "polyak" else self.actor

    def prepare(self, program: str) -> Plan:
        """The tensors of this call: validates the optimisers, the gradients and the state, creating the state of a parameter
        that has none the way ``Adam._init_group`` / ``RMSprop._init_group`` does.  Nothing is stepped yet (``commit``)."""
        import torch
        segs = self._segments[program]
        if not segs:
            raise ValueError(f"nothing bound for {program!r}: " +
                             ("no critic optimiser" if program == "critic" else "no Polyak pairs" if program == "polyak" else
                              "no policy optimiser" if program == "policy" else "no actor optimisers"))
        groups, tensors = [], {}
        for b, opt in enumerate(self._optimizers_of(program)):
            name = self._opt_name(opt)
            g = self._group(opt, name)
            rms = _is_rmsprop(opt)
            if rms:
                if any(torch.is_tensor(g[k]) for k in ("lr", "alpha", "eps")):
                    raise ValueError(f"{name}: lr, alpha and eps must be Python floats, not tensors")
            elif torch.is_tensor(g["lr"]) or any(torch.is_tensor(x) for x in g["betas"]):
                raise ValueError(f"{name}: lr and betas must be Python floats, not tensors")
            moments = ("square_avg",) if rms else ("exp_avg", "exp_avg_sq")
            steps = []
            for i, p in enumerate(g["params"]):
                what = f"{name}: parameter {i} of shape {tuple(p.shape)}"
                grad = p.grad
                if grad is None:
                    raise ValueError(f"{what} has .grad None; every parameter of a bound optimiser needs a gradient at the call")
                if grad.dtype != torch.float32:
                    raise ValueError(f"{what}: .grad is {str(grad.dtype).replace('torch.', '')}, not float32")
                if not grad.is_contiguous() or grad.shape != p.shape:
                    raise ValueError(f"{what}: .grad is not contiguous")
                if grad.device != p.device:
                    raise ValueError(f"{what}: .grad is on {grad.device}, the parameter on {p.device}")
                st = opt.state[p]
                if len(st) == 0 and rms:              # RMSprop._init_group, capturable off, momentum = 0, not centered
                    st["step"] = torch.zeros((), dtype=torch.float32)
                    st["square_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                elif len(st) == 0:                    # Adam._init_group, capturable and fused off
                    st["step"] = torch.tensor(0.0, dtype=torch.float32)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                step = st["step"]
                if not torch.is_tensor(step) or step.device.type != "cpu":
                    raise ValueError(f"{what}: state['step'] is not a CPU tensor (capturable or fused state?)")
                if rms and set(st) != {"step", "square_avg"}:
                    raise ValueError(f"{what}: its RMSprop state holds {sorted(st)}, not 'step' and 'square_avg' alone "
                                     "(the state of momentum or centered?)")
                for k in moments:
                    s = st[k]
                    if s.dtype != torch.float32 or not s.is_contiguous() or s.shape != p.shape or s.device != p.device:
                        raise ValueError(f"{what}: state[{k!r}] is not a float32 contiguous tensor like the parameter")
                steps.append(step)
                tensors[id(p)] = (grad, None, st["square_avg"]) if rms else (grad, st["exp_avg"], st["exp_avg_sq"])
            if not steps:
                raise ValueError(f"{name} has no parameters")
            values = [float(s) for s in steps]
            if any(v != values[0] for v in values):
                raise ValueError(f"{name}: state['step'] differs between its parameters ({sorted(set(values))}); one launch takes one step")
            groups.append((g, steps))
        rows = []
        for s in segs:
            g_, m_, v_ = tensors[id(s.param)] if s.op & ADAM or s.op == RMSPROP else (None, None, None)
            rows.append(Row(s, (s.param, g_, m_, v_, s.target)))
        return Plan(program, rows, groups)

    def commit(self, plan: Plan) -> "_capi.MeshOptimScalars":
        """Increment every ``step`` of the plan and return the scalars of the step, computed as torch computes them."""
        S = _capi.MeshOptimScalars()
        for b, (g, steps) in enumerate(plan.groups):
            for s in steps:
                s += 1
            if "betas" not in g:                     # an RMSprop group: alpha in beta2, 1 - alpha in w2, lr in step_size; the others unread
                S.step_size[b], S.bc2_sqrt[b], S.w1[b] = g["lr"], 1.0, 0.0
                S.beta2[b], S.w2[b], S.eps[b] = g["alpha"], 1 - g["alpha"], g["eps"]
                continue
            beta1, beta2 = g["betas"]
            S.step_size[b], S.bc2_sqrt[b] = adam_scalars(steps[0].item(), g["lr"], beta1, beta2)
            S.w1[b], S.beta2[b], S.w2[b], S.eps[b] = 1 - beta1, beta2, 1 - beta2, g["eps"]
        S.tau, S.one_minus_tau = self._tau, 1 - self._tau
        return S

    # ---------------------------------------------------------------- constructors
    @classmethod
    def sac(cls, critic_optimizer, actor_optimizer, ent_coef_optimizer=None, critic_params=(), critic_target_params=(),
            tau: float = 0.005) -> "OptimStepSpec":
        actor = [actor_optimizer] + ([ent_coef_optimizer] if ent_coef_optimizer is not None else [])
        return cls(critic_optimizer, actor, [(critic_params, critic_target_params)], tau)

    @classmethod
    def td3(cls, critic_optimizer, actor_optimizer, critic_params=(), critic_target_params=(), actor_params=(),
            actor_target_params=(), tau: float = 0.005) -> "OptimStepSpec":
        return cls(critic_optimizer, [actor_optimizer], [(critic_params, critic_target_params), (actor_params, actor_target_params)], tau)

    @classmethod
    def on_policy(cls, optimizer) -> "OptimStepSpec":
        return cls(policy=optimizer)

    @classmethod
    def from_sb3(cls, model) -> "OptimStepSpec":
        """A PPO / A2C model or its ActorCriticPolicy (``.policy``, or the object itself, has ``mlp_extractor`` and a non-None
        ``optimizer``): that optimiser is bound to ``policy``.  Otherwise duck-typed on SB3 2.x's SAC
        (``critic.optimizer``, ``actor.optimizer``, ``ent_coef_optimizer`` when
        ``log_ent_coef`` is learned, ``critic`` -> ``critic_target``) and TD3 / DDPG (``critic.optimizer``,
        ``actor.optimizer``, ``critic`` -> ``critic_target``, ``actor`` -> ``actor_target``), with ``model.tau``."""
        for pol in (getattr(model, "policy", None), model):
            if pol is not None and hasattr(pol, "mlp_extractor") and getattr(pol, "optimizer", None) is not None:
                return cls.on_policy(pol.optimizer)
        name = type(model).__name__
        actor, critic, critic_target = (getattr(model, k, None) for k in ("actor", "critic", "critic_target"))
        if actor is None or critic is None or critic_target is None:
            raise ValueError(f"{name} has no actor / critic / critic_target: not an SB3 SAC, TD3 or DDPG model")
        for who, m in (("actor", actor), ("critic", critic)):
            if getattr(m, "optimizer", None) is None:
                raise ValueError(f"{name}.{who} has no optimizer: not an SB3 SAC, TD3 or DDPG model")
        if not hasattr(model, "tau"):
            raise ValueError(f"{name} has no tau")
        _no_batch_norm(model, name)
        actor_target = getattr(model, "actor_target", None)
        if actor_target is not None:                 # TD3 / DDPG
            return cls.td3(critic.optimizer, actor.optimizer, _params(critic), _params(critic_target), _params(actor),
                           _params(actor_target), model.tau)
        ent = getattr(model, "ent_coef_optimizer", None) if getattr(model, "log_ent_coef", None) is not None else None
        return cls.sac(critic.optimizer, actor.optimizer, ent, _params(critic), _params(critic_target), model.tau)

    def check_device(self, device) -> None:
        check_device([p for opt in self.optimizers() for p in opt.param_groups[0]["params"]], device, "FusedOptimStep")
        check_device([x for pair in self.pairs for x in pair], device, "FusedOptimStep", "Polyak tensor")


def _params(module) -> list:
    """``module.parameters()``; a stand-in without it lists its ``q_networks`` / ``latent_pi, mu, log_std`` / ``mu``."""
    if hasattr(module, "parameters"):
        return list(module.parameters())
    parts = list(getattr(module, "q_networks", [])) or [getattr(module, k) for k in ("latent_pi", "mu", "log_std") if hasattr(module, k)]
    if not parts:
        raise ValueError(f"{type(module).__name__} has neither parameters() nor q_networks / mu")
    return [p for part in parts for p in part.parameters()]


def _no_batch_norm(model, name) -> None:
    """SB3 copies the batch-norm running statistics with a polyak_update of tau = 1; that is not built."""
    for attr in ("batch_norm_stats", "critic_batch_norm_stats", "actor_batch_norm_stats"):
        stats = getattr(model, attr, None)
        if stats is not None and len(list(stats)) > 0:
            raise ValueError(f"{name}.{attr} holds {len(list(stats))} batch-norm running statistics; networks with batch norm are not supported")
    for who in ("actor", "critic"):
        m = getattr(model, who)
        if hasattr(m, "named_buffers"):
            found = [k for k, _ in m.named_buffers() if "running_" in k]
            if found:
                raise ValueError(f"{name}.{who} has batch-norm running statistics ({found[0]}, ...); networks with batch norm are not supported")


class FusedOptimStep(Handle):
    """An OptimStepSpec bound on one GPU: critic_step(), actor_step(polyak=True), polyak(), policy_step(); one launch each on
    the current stream, no synchronisation while the tensors' pointers stay what they were."""
    PREFIX = "meshenv_optim"

    def __init__(self, spec: OptimStepSpec, device: int = 0):
        self.spec = spec
        super().__init__(device, check_device=spec.check_device)
        self._bound = {}              # program -> the pointers its device tables hold
        self.binds = 0                # uploads so far: stays put in the steady state

    @classmethod
    def sac(cls, critic_optimizer, actor_optimizer, ent_coef_optimizer=None, critic_params=(), critic_target_params=(),
            tau: float = 0.005, device: int = 0):
        return cls(OptimStepSpec.sac(critic_optimizer, actor_optimizer, ent_coef_optimizer, critic_params, critic_target_params, tau), device)

    @classmethod
    def td3(cls, critic_optimizer, actor_optimizer, critic_params=(), critic_target_params=(), actor_params=(),
            actor_target_params=(), tau: float = 0.005, device: int = 0):
        return cls(OptimStepSpec.td3(critic_optimizer, actor_optimizer, critic_params, critic_target_params, actor_params,
                                     actor_target_params, tau), device)

    @classmethod
    def on_policy(cls, optimizer, device: int = 0):
        """PPO's / A2C's one optimiser (``model.policy.optimizer``), for ``policy_step()``."""
        return cls(OptimStepSpec.on_policy(optimizer), device)

    @classmethod
    def from_sb3(cls, model, device: int = 0):
        return cls(OptimStepSpec.from_sb3(model), device)

    def _bind(self, plan: Plan, key) -> None:
        rows = plan.rows
        for r in rows:
            for x in r.tensors:
                if x is not None and x.device != self.device:
                    raise ValueError(f"{r.seg.name}: a tensor of shape {tuple(x.shape)} is on {x.device}, not on {self.device}")
        n = len(rows)
        cols = [(C.c_void_p * n)(*[k[j] or None for k in key]) for j in range(5)]
        i32 = lambda xs: (C.c_int32 * n)(*xs)   # noqa: E731
        rc = self._L.meshenv_optim_bind(self._h, PROGRAMS.index(plan.program), n, *cols, (C.c_int64 * n)(*[r.seg.n for r in rows]),
                                        i32([r.seg.op for r in rows]), i32([r.seg.block for r in rows]), i32([r.vec for r in rows]))
        self._check(rc, "meshenv_optim_bind")
        self._bound[plan.program] = key
        self.binds += 1

    def _run(self, program: str) -> None:
        plan = self.spec.prepare(program)
        self._bind_stream()
        key = plan.key()
        if self._bound.get(program) != key:          # host-side pointer comparison; an upload only when one has changed
            self._bind(plan, key)
        scalars = self.spec.commit(plan)
        self._check(self._L.meshenv_optim_step(self._h, PROGRAMS.index(program), C.byref(scalars)), "meshenv_optim_step")

    # ---------------------------------------------------------------- public
    def critic_step(self) -> None:
        """Adam on the critic optimiser: ``critic.optimizer.step()``.  One launch."""
        self._run("critic")

    def actor_step(self, polyak: bool = True) -> None:
        """Adam on the actor optimiser and, for SAC, the entropy-coefficient optimiser; then, with ``polyak``, every Polyak
        pair (a target whose source this launch steps sees the stepped value).  One launch."""
        self._run("actor_polyak" if polyak else "actor")

    def polyak(self) -> None:
        """``polyak_update`` of every pair alone.  One launch."""
        self._run("polyak")

    def policy_step(self) -> None:
        """Adam or RMSprop on the policy optimiser: ``model.policy.optimizer.step()`` of PPO / A2C.  One launch."""
        self._run("policy")
