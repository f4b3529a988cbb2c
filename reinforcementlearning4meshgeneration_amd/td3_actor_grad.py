"""The actor loss of TD3 / DDPG and its gradients on the GPU (include/meshenv_td3_actor_grad.h,
csrc/meshenv_td3_actor_grad.h): the statements of SB3 2.x's ``TD3.train`` that run every ``policy_delay`` steps,

    actor_loss = -self.critic.q1_forward(replay_data.observations, self.actor(replay_data.observations)).mean()
    self.actor.optimizer.zero_grad(); actor_loss.backward()

for the recipe the reference runs (rl/baselines/RL_Mesh.py:206-222): actor ReLU [256, 256] with a ``Linear(256, 3)`` +
``Tanh`` head on 18 observations, critic ``q_networks[0]`` ReLU [256, 256] on ``cat(obs, action)`` = 21, float32.  Only the
first critic is read: TD3's second critic and DDPG's absence of one make no difference to this statement.
``FusedTD3ActorGrad.backward`` returns ``actor_loss`` and leaves the gradients in ``p.grad`` of the six LIVE actor parameters,
so ``model.actor.optimizer.step()`` (or ``FusedOptimStep.actor_step``) consumes them as they are.  Every parameter -- the
critic's too -- is read as it is at the call (no refresh); the gradients are views into one flat buffer the object owns and
are OVERWRITTEN by every call.

One difference from eager torch, on purpose: ``actor_loss.backward()`` also accumulates into the critic's ``.grad``; this
call leaves it exactly as it was.  SB3 zeroes it before the next critic step and ``FusedCriticGrad`` overwrites it, so nothing
reads what eager leaves there.

``TD3ActorGradSpec`` is the host half (the parameter tensors and every refusal; no device needed).  SAC's statement is
``FusedActorGrad``'s."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List

from . import sb3_nets as N
from ._handle import GradBuffer, Handle
from .sb3_nets import ACT_DIM, KIND_TD3, OBS_DIM

HIDDEN = 256


@dataclass
class TD3ActorGradSpec:
    actor: List = field(default_factory=list)     # w1 b1 w2 b2 w3 b3: meshenv_td3_actor_grad_bind's order
    q1: List = field(default_factory=list)        # the live first critic, read only: w1 b1 w2 b2 out_w out_b

    kind = KIND_TD3
    kind_name = "td3"
    hidden = HIDDEN

    def tensors(self):
        return list(self.actor) + list(self.q1)

    # ---------------------------------------------------------------- the flat gradient buffer
    @property
    def n_grad(self) -> int:
        """Floats in the gradient buffer: the actor's parameters in order, padded to a multiple of 64."""
        return (sum(int(p.numel()) for p in self.actor) + 63) // 64 * 64

    def offsets(self):
        """[(parameter, first float in the gradient buffer)] for the six actor parameters."""
        out, at = [], 0
        for p in self.actor:
            out.append((p, at))
            at += int(p.numel())
        return out

    # ---------------------------------------------------------------- constructors
    @classmethod
    def td3(cls, actor_layers, mu, q1) -> "TD3ActorGradSpec":
        """actor_layers: the actor's two hidden Linear layers; mu: its output Linear (the Tanh follows it); q1: the first
        q_network (an nn.Sequential or a list of its Linear layers)."""
        return cls(N.td3_actor_params(actor_layers, mu), N._critic(q1, KIND_TD3, "q_networks[0]"))

    @classmethod
    def from_sb3(cls, model) -> "TD3ActorGradSpec":
        """Duck-typed on SB3 2.x's TD3 / DDPG: ``actor.mu`` (the live actor, not ``actor_target``) and
        ``critic.q_networks[0]`` (the live critic, not ``critic_target``; n_critics >= 1)."""
        layers, mu = N.td3_live_actor(model)
        return cls.td3(layers, mu, N.first_critic(model, "critic"))

    def check_device(self, device) -> None:
        """Every bound tensor lives on `device` (a torch.device): the kernel reads them through raw pointers."""
        N.check_device(self.tensors(), device, "FusedTD3ActorGrad")


class FusedTD3ActorGrad(GradBuffer, Handle):
    """A TD3ActorGradSpec bound on one GPU.  backward() returns actor_loss (a 0-dim float32 CUDA tensor) and overwrites
    p.grad of the actor's six parameters."""
    PREFIX = "meshenv_td3_actor_grad"

    def __init__(self, spec: TD3ActorGradSpec, device: int = 0):
        self.spec = spec
        super().__init__(device, check_device=spec.check_device)
        self._alloc_grads()
        self.bind()

    kind = "td3"

    @classmethod
    def td3(cls, actor_layers, mu, q1, device: int = 0):
        return cls(TD3ActorGradSpec.td3(actor_layers, mu, q1), device)

    @classmethod
    def from_sb3(cls, model, device: int = 0):
        return cls(TD3ActorGradSpec.from_sb3(model), device)

    def bind(self) -> None:
        """Record the parameters' device pointers again: after anything that reallocates them (``.to()``; optimisers and
        ``load_state_dict`` write in place and need no new bind)."""
        s = self.spec
        s.check_device(self.device)
        rc = self._L.meshenv_td3_actor_grad_bind(self._h, self._ptrs(s.actor), len(s.actor), self._ptrs(s.q1), len(s.q1),
                                                 self.grad_buffer.data_ptr(), s.n_grad)
        self._check(rc, "meshenv_td3_actor_grad_bind")
        self._view_grads()

    # ---------------------------------------------------------------- public
    def backward(self, samples=None, *, observations=None, return_parts: bool = False):
        """actor_loss of a batch and its gradients: ``samples`` (a ReplayBufferSamples: observations is read) or
        ``observations`` [B, 18] by keyword.  Two launches on the current stream, no synchronisation.

        return_parts: also a dict of actions_pi [B, 3] (the actor's actions), q1_pi [B], dq_da [B, 3] (dQ1/daction), d_pre
        [B, 3] (the gradient of the loss at the head's pre-activation), and acts, acts1: the two [B, 256] post-ReLU
        activations of the actor and of the critic (``a > 0`` is the mask the backward pass used)."""
        t = self._torch
        if samples is not None:
            if observations is not None:
                raise ValueError("pass either samples or observations")
            observations = samples.observations
        if observations is None:
            raise ValueError("observations are required")
        if observations.dim() != 2 or observations.shape[0] == 0:
            raise ValueError(f"observations must have shape (B, {OBS_DIM}), got {tuple(observations.shape)}")
        B = int(observations.shape[0])
        obs = self._f32(observations, "observations", [(B, OBS_DIM)])
        f32 = dict(dtype=t.float32, device=self.device)
        loss = t.empty((), **f32)
        parts, pp, pa = {}, None, None
        if return_parts:
            parts = dict(actions_pi=t.empty((B, ACT_DIM), **f32), q1_pi=t.empty(B, **f32), dq_da=t.empty((B, ACT_DIM), **f32),
                         d_pre=t.empty((B, ACT_DIM), **f32))
            pp = self._ptrs(list(parts.values()))
            for k in ("acts", "acts1"):
                parts[k] = [t.empty((B, HIDDEN), **f32) for _ in range(2)]
            pa = self._ptrs(parts["acts"] + parts["acts1"])
        self._attach()
        self._bind_stream()
        rc = self._L.meshenv_td3_actor_grad_backward(self._h, B, obs.data_ptr(), loss.data_ptr(), pp, pa)
        self._check(rc, "meshenv_td3_actor_grad_backward")
        return (loss, parts) if return_parts else loss
