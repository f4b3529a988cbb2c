"""The actor loss and the entropy-coefficient loss of SAC and their gradients on the GPU (include/meshenv.h:
meshenv_actor_grad_*, csrc/meshenv_actor_grad.h): the statements of SB3 2.x's ``SAC.train`` that follow the critic update,

    actions_pi, log_prob = self.actor.action_log_prob(replay_data.observations)
    ent_coef = th.exp(self.log_ent_coef.detach())
    ent_coef_loss = -(self.log_ent_coef * (log_prob + self.target_entropy).detach()).mean()
    q_values_pi = th.cat(self.critic(replay_data.observations, actions_pi), dim=1)
    min_qf_pi, _ = th.min(q_values_pi, dim=1, keepdim=True)
    actor_loss = (ent_coef * log_prob - min_qf_pi).mean()
    self.actor.optimizer.zero_grad(); actor_loss.backward()

for the recipe the reference runs (rl/baselines/RL_Mesh.py:179-205): actor ReLU [128, 128, 128] with ``mu`` / ``log_std``
heads, twin critics ReLU [128, 128, 128] on ``cat(obs, action)`` = 21, float32.  ``FusedActorGrad.backward`` returns
``(actor_loss, ent_coef_loss)`` and leaves the gradients in ``p.grad`` of the ten LIVE actor parameters and of
``log_ent_coef``, so ``model.actor.optimizer.step()`` and ``model.ent_coef_optimizer.step()`` stay stock torch.  Every
parameter -- the critics' too -- is read as it is at the call (no refresh); the gradients are views into one flat buffer the
object owns and are OVERWRITTEN by every call.

One difference from eager torch, on purpose: ``actor_loss.backward()`` also accumulates into the critics' ``.grad``; this
call leaves them exactly as they were.  SB3 zeroes them before the next critic step and ``FusedCriticGrad`` overwrites them,
so nothing reads what eager leaves there.

``ActorGradSpec`` is the host half (the parameter tensors, the constants and every refusal; no device needed).  SAC only."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import List, Optional

from . import sb3_nets as N
from ._handle import GradBuffer, Handle
from .sb3_nets import ACT_DIM, KIND_SAC, OBS_DIM

HIDDEN = 128
PHILOX_TAG = 3                     # k_actor_grad's own stream (rollout noise 0, replay draw 1, TD target 2)


@dataclass
class ActorGradSpec:
    actor: List = field(default_factory=list)     # w1 b1 w2 b2 w3 b3 mu_w mu_b log_std_w log_std_b: meshenv_actor_grad_bind's order
    q1: List = field(default_factory=list)        # the live critics, read only
    q2: List = field(default_factory=list)
    log_ent_coef: Optional[object] = None         # the learned [1] tensor, or None with a fixed ent_coef
    ent_coef: float = 0.0
    target_entropy: float = -float(ACT_DIM)

    kind = KIND_SAC
    kind_name = "sac"
    hidden = HIDDEN

    def tensors(self):
        return list(self.actor) + list(self.q1) + list(self.q2) + ([self.log_ent_coef] if self.log_ent_coef is not None else [])

    def grad_tensors(self):
        """The parameters that receive a gradient: the actor's ten, then log_ent_coef when it is learned."""
        return list(self.actor) + ([self.log_ent_coef] if self.log_ent_coef is not None else [])

    # ---------------------------------------------------------------- the flat gradient buffer
    @property
    def ent_offset(self) -> int:
        """First float of log_ent_coef.grad: right after the actor's gradients."""
        return sum(int(p.numel()) for p in self.actor)

    @property
    def n_grad(self) -> int:
        """Floats in the gradient buffer: the actor's parameters in order, log_ent_coef, padded to a multiple of 64."""
        return (self.ent_offset + 1 + 63) // 64 * 64

    def offsets(self):
        """[(parameter, first float in the gradient buffer)] for the 10 (fixed ent_coef) / 11 parameters."""
        out, at = [], 0
        for p in self.grad_tensors():
            out.append((p, at))
            at += int(p.numel())
        return out

    # ---------------------------------------------------------------- constructors
    @classmethod
    def sac(cls, actor_layers, mu, log_std, q1, q2, log_ent_coef=None, ent_coef=None, target_entropy=-3.0) -> "ActorGradSpec":
        lec, fixed = N.ent_coef(log_ent_coef, ent_coef)
        return cls(N.sac_actor_params(actor_layers, mu, log_std), *N.twin_params(KIND_SAC, q1, q2), log_ent_coef=lec, ent_coef=fixed,
                   target_entropy=N.finite(target_entropy, "target_entropy"))

    @classmethod
    def from_sb3(cls, model) -> "ActorGradSpec":
        """Duck-typed on SB3 2.x's SAC: ``actor.latent_pi / .mu / .log_std``, ``critic.q_networks`` (the live critics, not
        ``critic_target``), ``log_ent_coef`` or ``ent_coef_tensor``, ``target_entropy``."""
        actor = getattr(model, "actor", None)
        if not hasattr(actor, "latent_pi"):
            if hasattr(getattr(model, "actor_target", None), "mu") or hasattr(actor, "mu"):
                raise ValueError(f"{type(model).__name__} is a TD3 / DDPG model (a deterministic actor without latent_pi): "
                                 "not yet: SAC only (FusedTD3ActorGrad computes TD3's actor loss gradient)")
            raise ValueError(f"{type(model).__name__} has no actor.latent_pi: not an SB3 SAC model")
        qs = N.twin_critics(model, "critic", who="SAC")
        te = getattr(model, "target_entropy", None)
        if te is None or isinstance(te, str):
            raise ValueError(f"model.target_entropy is {te!r}; SB3 sets it to a float in _setup_model")
        return cls.sac(N.sac_actor(actor), actor.mu, actor.log_std, qs[0], qs[1], target_entropy=float(te), **N.model_ent_coef(model))

    def check_device(self, device) -> None:
        """Every bound tensor lives on `device` (a torch.device): the kernel reads them through raw pointers."""
        N.check_device(self.tensors(), device, "FusedActorGrad")


class FusedActorGrad(GradBuffer, Handle):
    """An ActorGradSpec bound on one GPU.  backward() returns (actor_loss, ent_coef_loss) (0-dim float32 CUDA tensors; the
    second is None with a fixed ent_coef) and overwrites p.grad of the actor's parameters and of log_ent_coef."""
    PREFIX = "meshenv_actor_grad"

    def __init__(self, spec: ActorGradSpec, device: int = 0):
        self.spec = spec
        super().__init__(device, spec.ent_coef, spec.target_entropy, check_device=spec.check_device)
        self._alloc_grads()
        self.bind()

    kind = "sac"

    @classmethod
    def sac(cls, actor_layers, mu, log_std, q1, q2, log_ent_coef=None, ent_coef=None, target_entropy=-3.0, device: int = 0):
        return cls(ActorGradSpec.sac(actor_layers, mu, log_std, q1, q2, log_ent_coef, ent_coef, target_entropy), device)

    @classmethod
    def from_sb3(cls, model, device: int = 0):
        return cls(ActorGradSpec.from_sb3(model), device)

    def bind(self) -> None:
        """Record the parameters' device pointers again: after anything that reallocates them (``.to()``; optimisers and
        ``load_state_dict`` write in place and need no new bind)."""
        s = self.spec
        s.check_device(self.device)
        arr = self._ptrs
        lec = s.log_ent_coef.data_ptr() if s.log_ent_coef is not None else None
        rc = self._L.meshenv_actor_grad_bind(self._h, arr(s.actor), len(s.actor), arr(s.q1), arr(s.q2), len(s.q1), lec,
                                             self.grad_buffer.data_ptr(), s.n_grad)
        self._check(rc, "meshenv_actor_grad_bind")
        self._view_grads()

    # ---------------------------------------------------------------- public
    def backward(self, samples=None, *, observations=None, noise=None, seed=None, counter=None, return_parts: bool = False):
        """(actor_loss, ent_coef_loss) of a batch and their gradients: ``samples`` (a ReplayBufferSamples: observations is
        read) or ``observations`` [B, 18] by keyword.  eps of ``actions_pi`` is ``noise`` ([B, 3] of N(0, 1) draws), drawn in
        the kernel when ``seed`` is given (Philox4x32-10 at (seed, counter, sample index) with this call's own tag 3: pass a
        fresh counter every batch), or 0 with neither.  Two launches on the current stream, no synchronisation.

        The coefficient of the loss is ``expf(log_ent_coef)`` as it is at the call: call ``backward`` BEFORE
        ``ent_coef_optimizer.step()`` to keep SB3's order (it takes ``ent_coef`` before it steps the coefficient).

        return_parts: also a dict of actions_pi [B, 3], log_prob [B], q1_pi, q2_pi [B], dq_da [B, 3] (the selected critic's
        dQ/daction; q1 <= q2 selects critic 1), d_mu, d_log_std [B, 3] (the head gradients), and acts, acts1, acts2: per
        hidden layer the [B, 128] post-ReLU activations of the actor and of the two critics (``a > 0`` is the mask the
        backward pass used) and, with noise, eps [B, 3]; backward(noise=parts["eps"]) reproduces a sampled call bit for bit."""
        t = self._torch
        if samples is not None:
            if observations is not None:
                raise ValueError("pass either samples or observations")
            observations = samples.observations
        if observations is None:
            raise ValueError("observations are required")
        if noise is not None and seed is not None:
            raise ValueError("pass either noise or seed")
        if counter is not None and seed is None:
            raise ValueError("counter goes with seed")
        if observations.dim() != 2 or observations.shape[0] == 0:
            raise ValueError(f"observations must have shape (B, {OBS_DIM}), got {tuple(observations.shape)}")
        B = int(observations.shape[0])
        obs = self._f32(observations, "observations", [(B, OBS_DIM)])
        if noise is not None:
            noise = self._f32(noise, "noise", [(B, ACT_DIM)])
        f32 = dict(dtype=t.float32, device=self.device)
        losses = t.empty(2, **f32)
        parts, pp, pa = {}, None, None
        if return_parts:
            parts = dict(actions_pi=t.empty((B, ACT_DIM), **f32), log_prob=t.empty(B, **f32), q1_pi=t.empty(B, **f32),
                         q2_pi=t.empty(B, **f32), dq_da=t.empty((B, ACT_DIM), **f32), d_mu=t.empty((B, ACT_DIM), **f32),
                         d_log_std=t.empty((B, ACT_DIM), **f32))
            arr = self._ptrs
            pp = arr(list(parts.values()))
            for k in ("acts", "acts1", "acts2"):
                parts[k] = [t.empty((B, HIDDEN), **f32) for _ in range(3)]
            pa = arr(parts["acts"] + parts["acts1"] + parts["acts2"])
            if noise is not None or seed is not None:
                parts["eps"] = t.empty((B, ACT_DIM), **f32)
        self._attach()
        self._bind_stream()
        rc = self._L.meshenv_actor_grad_backward(
            self._h, B, obs.data_ptr(), noise.data_ptr() if noise is not None else None, 1 if seed is not None else 0,
            C.c_uint64((seed or 0) & (2 ** 64 - 1)), C.c_uint64(int(counter or 0) & (2 ** 64 - 1)), losses.data_ptr(),
            parts["eps"].data_ptr() if "eps" in parts else None, pp, pa)
        self._check(rc, "meshenv_actor_grad_backward")
        out = (losses[0], losses[1] if self.spec.log_ent_coef is not None else None)
        return (*out, parts) if return_parts else out
