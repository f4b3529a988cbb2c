"""DDPG's critic and actor loss gradients on the GPU (include/meshenv_ddpg_grad.h, csrc/meshenv_wide_grad.h): the two
gradient statements of SB3 2.x's ``TD3.train``, which DDPG inherits, for the networks ``DDPG('MlpPolicy', env)`` builds (the
reference's rl/baselines/RL_Mesh.py:113-228): a ReLU [400, 300] actor with a ``Linear(300, 3)`` + ``Tanh`` head on 18
observations, ONE ReLU [400, 300] critic on ``cat(obs, action)`` = 21, float32,

    critic_loss = sum(F.mse_loss(q, target_q_values) for q in critic(obs, actions));  zero_grad(); critic_loss.backward()
    actor_loss = -critic.q1_forward(obs, actor(obs)).mean();                           zero_grad(); actor_loss.backward()

``FusedDDPGGrad.critic_backward`` / ``actor_backward`` return the loss and leave the gradients in ``p.grad`` of the six LIVE
critic / actor parameters, so ``FusedOptimStep.critic_step()`` / ``actor_step()`` (or the torch optimisers) consume them as
they are.  Every parameter is read as it is at the call (no refresh); the gradients are views into one flat buffer the
object owns, and each call OVERWRITES its own network's set and leaves the other's alone.

``loss_scale`` (1.0 or 0.5) multiplies ``critic_loss`` and with it the critic's gradients: 1.0 is the statement above, 0.5 the
convention of ``FusedCriticGrad``'s td3 kind.

One difference from eager torch, on purpose, as in ``FusedTD3ActorGrad``: ``actor_loss.backward()`` also accumulates into
the critic's ``.grad``; ``actor_backward`` leaves it exactly as it was.

``DDPGGradSpec`` is the host half (the parameter tensors and every refusal; no device needed)."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List

from . import _capi
from . import sb3_nets as N
from ._handle import GradBuffer, Handle
from .sb3_nets import ACT_DIM, DDPG_WIDTHS, KIND_DDPG, OBS_DIM

MAX_ROWS = _capi.DDPG_GRAD_MAX_ROWS
LOSS_SCALES = (0.5, 1.0)


def _pad64(n: int) -> int:
    return (n + 63) // 64 * 64


@dataclass
class DDPGGradSpec:
    actor: List = field(default_factory=list)     # w1 b1 w2 b2 w3 b3: meshenv_ddpg_grad_bind's order
    q1: List = field(default_factory=list)        # the live critic: w1 b1 w2 b2 out_w out_b
    loss_scale: float = 1.0

    kind = KIND_DDPG
    kind_name = "ddpg"
    widths = DDPG_WIDTHS

    def __post_init__(self):
        ls = self.loss_scale
        if isinstance(ls, bool) or not isinstance(ls, (int, float)) or float(ls) not in LOSS_SCALES:
            N._refuse(f"loss_scale = {self.loss_scale!r}; FusedDDPGGrad takes 1.0 (SB3's TD3.train) or 0.5 (FusedCriticGrad's td3 kind)")
        self.loss_scale = float(self.loss_scale)

    def tensors(self):
        return list(self.actor) + list(self.q1)

    # ---------------------------------------------------------------- the flat gradient buffer
    @property
    def n_actor(self) -> int:
        """Floats of the actor's set: its parameters in order, padded to a multiple of 64."""
        return _pad64(sum(int(p.numel()) for p in self.actor))

    @property
    def n_critic(self) -> int:
        return _pad64(sum(int(p.numel()) for p in self.q1))

    @property
    def n_grad(self) -> int:
        """Floats in the gradient buffer: the actor's set, then the critic's."""
        return self.n_actor + self.n_critic

    def actor_offsets(self):
        """[(parameter, first float in the gradient buffer)] for the six actor parameters."""
        out, at = [], 0
        for p in self.actor:
            out.append((p, at))
            at += int(p.numel())
        return out

    def critic_offsets(self):
        out, at = [], self.n_actor
        for p in self.q1:
            out.append((p, at))
            at += int(p.numel())
        return out

    def offsets(self):
        return self.actor_offsets() + self.critic_offsets()

    # ---------------------------------------------------------------- constructors
    @classmethod
    def ddpg(cls, actor_layers, mu, q1, loss_scale: float = 1.0) -> "DDPGGradSpec":
        """actor_layers: the actor's two hidden Linear layers; mu: its output Linear (the Tanh follows it); q1: the one
        q_network (an nn.Sequential or a list of its Linear layers)."""
        return cls(N.ddpg_actor_params(actor_layers, mu), N.ddpg_critic_params(q1), loss_scale)

    @classmethod
    def from_sb3(cls, model, loss_scale: float = 1.0) -> "DDPGGradSpec":
        """Duck-typed on SB3 2.x's DDPG: ``actor.mu`` (the live actor, not ``actor_target``) and ``critic.q_networks[0]`` (the
        live critic, n_critics = 1), both of hidden widths [400, 300]."""
        if not N.is_ddpg(model, "actor", "critic"):
            N._refuse(f"{type(model).__name__} is not a DDPG model (actor.mu and ONE critic.q_networks entry of hidden widths "
                      f"{list(DDPG_WIDTHS)}): FusedCriticGrad / FusedTD3ActorGrad take TD3, FusedCriticGrad / FusedActorGrad SAC")
        layers, mu = N.td3_live_actor(model)
        return cls.ddpg(layers, mu, N.first_critic(model, "critic", "FusedDDPGGrad"), loss_scale)

    def check_device(self, device) -> None:
        """Every bound tensor lives on `device` (a torch.device): the kernels read them through raw pointers."""
        N.check_device(self.tensors(), device, "FusedDDPGGrad")


def check_batch(B: int) -> int:
    if B > MAX_ROWS:
        N._refuse(f"a batch of {B} rows; FusedDDPGGrad takes at most {MAX_ROWS} rows a call")
    return B


class FusedDDPGGrad(GradBuffer, Handle):
    """A DDPGGradSpec bound on one GPU.  critic_backward() / actor_backward() return the loss (a 0-dim float32 CUDA tensor)
    and overwrite p.grad of the critic's / the actor's six parameters."""
    PREFIX = "meshenv_ddpg_grad"
    kind = "ddpg"

    def __init__(self, spec: DDPGGradSpec, device: int = 0):
        self.spec = spec
        super().__init__(device, spec.loss_scale, check_device=spec.check_device)
        self._alloc_grads()
        self.bind()

    @classmethod
    def ddpg(cls, actor_layers, mu, q1, loss_scale: float = 1.0, device: int = 0):
        return cls(DDPGGradSpec.ddpg(actor_layers, mu, q1, loss_scale), device)

    @classmethod
    def from_sb3(cls, model, loss_scale: float = 1.0, device: int = 0):
        return cls(DDPGGradSpec.from_sb3(model, loss_scale), device)

    @property
    def loss_scale(self) -> float:
        return self.spec.loss_scale

    def bind(self) -> None:
        """Record the parameters' device pointers again: after anything that reallocates them (``.to()``; optimisers and
        ``load_state_dict`` write in place and need no new bind)."""
        s = self.spec
        s.check_device(self.device)
        rc = self._L.meshenv_ddpg_grad_bind(self._h, self._ptrs(s.actor), len(s.actor), self._ptrs(s.q1), len(s.q1),
                                            self.grad_buffer.data_ptr(), s.n_grad)
        self._check(rc, "meshenv_ddpg_grad_bind")
        self._view_grads()
        n = len(s.actor)
        self._actor_views, self._critic_views = self._views[:n], self._views[n:]

    def _attach_set(self, views):
        self._views = views
        try:
            self._attach()
        finally:
            self._views = self._actor_views + self._critic_views

    # ---------------------------------------------------------------- public
    def critic_backward(self, samples=None, target_q_values=None, *, observations=None, actions=None, return_parts: bool = False):
        """critic_loss of a batch and the critic's gradients: ``samples`` (a ReplayBufferSamples: observations and actions
        are read) or the two tensors by keyword, and target_q_values [B, 1] or [B] (a constant).  Three launches on the
        current stream, no synchronisation.  return_parts: also a dict of q1 [B] and acts1: the [B, 400] and [B, 300]
        post-ReLU activations (``a > 0`` is the mask the backward pass used)."""
        t = self._torch
        if samples is not None:
            if observations is not None or actions is not None:
                raise ValueError("pass either samples or observations / actions")
            observations, actions = samples.observations, samples.actions
        if observations is None or actions is None or target_q_values is None:
            raise ValueError("observations, actions and target_q_values are required")
        if observations.dim() != 2 or observations.shape[0] == 0:
            raise ValueError(f"observations must have shape (B, {OBS_DIM}), got {tuple(observations.shape)}")
        B = check_batch(int(observations.shape[0]))
        obs = self._f32(observations, "observations", [(B, OBS_DIM)])
        act = self._f32(actions, "actions", [(B, ACT_DIM)])
        y = self._f32(target_q_values, "target_q_values", [(B, 1), (B,)])
        f32 = dict(dtype=t.float32, device=self.device)
        loss = t.empty((), **f32)
        parts, pp = {}, None
        if return_parts:
            parts = dict(q1=t.empty(B, **f32), acts1=[t.empty((B, w), **f32) for w in DDPG_WIDTHS])
            pp = self._ptrs([parts["q1"]] + parts["acts1"])
        self._attach_set(self._critic_views)
        self._bind_stream()
        rc = self._L.meshenv_ddpg_grad_critic_backward(self._h, B, obs.data_ptr(), act.data_ptr(), y.data_ptr(), loss.data_ptr(), pp)
        self._check(rc, "meshenv_ddpg_grad_critic_backward")
        return (loss, parts) if return_parts else loss

    def actor_backward(self, samples=None, *, observations=None, return_parts: bool = False):
        """actor_loss of a batch and the actor's gradients: ``samples`` (a ReplayBufferSamples: observations is read) or
        ``observations`` [B, 18] by keyword.  Three launches on the current stream, no synchronisation.

        return_parts: also a dict of actions_pi [B, 3] (the actor's actions), q1_pi [B], dq_da [B, 3] (dQ1/daction), d_pre
        [B, 3] (the gradient of the loss at the head's pre-activation), and acts, acts1: the [B, 400] and [B, 300] post-ReLU
        activations of the actor and of the critic."""
        t = self._torch
        if samples is not None:
            if observations is not None:
                raise ValueError("pass either samples or observations")
            observations = samples.observations
        if observations is None:
            raise ValueError("observations are required")
        if observations.dim() != 2 or observations.shape[0] == 0:
            raise ValueError(f"observations must have shape (B, {OBS_DIM}), got {tuple(observations.shape)}")
        B = check_batch(int(observations.shape[0]))
        obs = self._f32(observations, "observations", [(B, OBS_DIM)])
        f32 = dict(dtype=t.float32, device=self.device)
        loss = t.empty((), **f32)
        parts, pp, pa = {}, None, None
        if return_parts:
            parts = dict(actions_pi=t.empty((B, ACT_DIM), **f32), q1_pi=t.empty(B, **f32), dq_da=t.empty((B, ACT_DIM), **f32),
                         d_pre=t.empty((B, ACT_DIM), **f32))
            pp = self._ptrs(list(parts.values()))
            for k in ("acts", "acts1"):
                parts[k] = [t.empty((B, w), **f32) for w in DDPG_WIDTHS]
            pa = self._ptrs(parts["acts"] + parts["acts1"])
        self._attach_set(self._actor_views)
        self._bind_stream()
        rc = self._L.meshenv_ddpg_grad_actor_backward(self._h, B, obs.data_ptr(), loss.data_ptr(), pp, pa)
        self._check(rc, "meshenv_ddpg_grad_actor_backward")
        return (loss, parts) if return_parts else loss
