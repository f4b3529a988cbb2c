"""The critic loss of SAC and TD3 and its gradients on the GPU (include/meshenv.h: meshenv_critic_grad_*,
csrc/meshenv_critic_grad.h): the statements of SB3 2.x's ``SAC.train`` / ``TD3.train`` that follow the TD target,

    current_q_values = self.critic(replay_data.observations, replay_data.actions)
    critic_loss = 0.5 * sum(F.mse_loss(current_q, target_q_values) for current_q in current_q_values)
    self.critic.optimizer.zero_grad(); critic_loss.backward()

for the twin critics the reference trains (rl/baselines/RL_Mesh.py:179-222): ReLU [128, 128, 128] (SAC) and ReLU [256, 256]
(TD3), input ``cat(obs, action)`` = 21, float32.  ``FusedCriticGrad.backward`` returns ``critic_loss`` and leaves the
gradients in ``p.grad`` of the LIVE critic parameters, so ``model.critic.optimizer.step()`` stays stock torch.  The
parameters are read as they are at the call (no refresh); the gradients are views into one flat buffer the object owns and
are OVERWRITTEN by every call.  ``CriticGradSpec`` is the host half (kind, the parameter tensors, every refusal; no device
needed)."""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List

from . import sb3_nets as N
from ._handle import GradBuffer, Handle
from .sb3_nets import ACT_DIM, HIDDEN, KIND_SAC, KIND_TD3, OBS_DIM


@dataclass
class CriticGradSpec:
    kind: int
    q1: List = field(default_factory=list)     # w1 b1 w2 b2 [w3 b3] out_w out_b: meshenv_critic_grad_bind's order
    q2: List = field(default_factory=list)

    @property
    def kind_name(self) -> str:
        return "sac" if self.kind == KIND_SAC else "td3"

    @property
    def hidden(self) -> int:
        return HIDDEN[self.kind][0]

    def tensors(self):
        return list(self.q1) + list(self.q2)

    # ---------------------------------------------------------------- the flat gradient buffer
    @property
    def stride(self) -> int:
        """Floats per critic in the gradient buffer: its parameters in order, padded to a multiple of 64."""
        return (sum(int(p.numel()) for p in self.q1) + 63) // 64 * 64

    @property
    def n_grad(self) -> int:
        return 2 * self.stride

    def offsets(self):
        """[(parameter, first float in the gradient buffer)] for all 16 (SAC) / 12 (TD3) parameters."""
        out = []
        for k, ps in enumerate((self.q1, self.q2)):
            at = k * self.stride
            for p in ps:
                out.append((p, at))
                at += int(p.numel())
        return out

    # ---------------------------------------------------------------- constructors
    @classmethod
    def _twin(cls, kind, q1, q2) -> "CriticGradSpec":
        return cls(kind, *N.twin_params(kind, q1, q2))

    @classmethod
    def sac(cls, q1, q2) -> "CriticGradSpec":
        return cls._twin(KIND_SAC, q1, q2)

    @classmethod
    def td3(cls, q1, q2) -> "CriticGradSpec":
        return cls._twin(KIND_TD3, q1, q2)

    @classmethod
    def from_sb3(cls, model) -> "CriticGradSpec":
        """Duck-typed on SB3 2.x's SAC / TD3: ``model.critic.q_networks`` (the live critics, not ``critic_target``)."""
        qs = N.twin_critics(model, "critic", ddpg=True)
        return cls._twin(N.critic_kind(qs[0], "q_networks[0]"), qs[0], qs[1])

    def check_device(self, device) -> None:
        """Every bound tensor lives on `device` (a torch.device): the kernel reads them through raw pointers."""
        N.check_device(self.tensors(), device, "FusedCriticGrad")


class FusedCriticGrad(GradBuffer, Handle):
    """A CriticGradSpec bound on one GPU.  backward() returns critic_loss (0-dim float32 CUDA tensor) and overwrites p.grad
    of every bound parameter."""
    PREFIX = "meshenv_critic_grad"

    def __init__(self, spec: CriticGradSpec, device: int = 0):
        self.spec = spec
        super().__init__(device, spec.kind, check_device=spec.check_device)
        self._alloc_grads()
        self.bind()

    @property
    def kind(self) -> str:
        return self.spec.kind_name

    @classmethod
    def sac(cls, q1, q2, device: int = 0):
        return cls(CriticGradSpec.sac(q1, q2), device)

    @classmethod
    def td3(cls, q1, q2, device: int = 0):
        return cls(CriticGradSpec.td3(q1, q2), device)

    @classmethod
    def from_sb3(cls, model, device: int = 0):
        return cls(CriticGradSpec.from_sb3(model), device)

    def bind(self) -> None:
        """Record the parameters' device pointers again: after anything that reallocates them (``.to()``; optimisers and
        ``load_state_dict`` write in place and need no new bind)."""
        s = self.spec
        s.check_device(self.device)
        rc = self._L.meshenv_critic_grad_bind(self._h, self._ptrs(s.q1), self._ptrs(s.q2), len(s.q1), self.grad_buffer.data_ptr(),
                                              s.n_grad)
        self._check(rc, "meshenv_critic_grad_bind")
        self._view_grads()

    # ---------------------------------------------------------------- public
    def backward(self, samples=None, target_q_values=None, *, observations=None, actions=None, return_parts: bool = False):
        """critic_loss of a batch and its gradients: ``samples`` (a ReplayBufferSamples: observations and actions are read)
        or the two tensors by keyword, and target_q_values [B, 1] or [B] (a constant: no gradient flows into it).  Two
        launches on the current stream, no synchronisation.  return_parts: also a dict of q1, q2 [B] and acts1, acts2: per
        hidden layer the [B, H] post-ReLU activations of that critic (``a > 0`` is the mask the backward pass used)."""
        t = self._torch
        if samples is not None:
            if observations is not None or actions is not None:
                raise ValueError("pass either samples or observations / actions")
            observations, actions = samples.observations, samples.actions
        if observations is None or actions is None or target_q_values is None:
            raise ValueError("observations, actions and target_q_values are required")
        if observations.dim() != 2 or observations.shape[0] == 0:
            raise ValueError(f"observations must have shape (B, {OBS_DIM}), got {tuple(observations.shape)}")
        B = int(observations.shape[0])
        obs = self._f32(observations, "observations", [(B, OBS_DIM)])
        act = self._f32(actions, "actions", [(B, ACT_DIM)])
        y = self._f32(target_q_values, "target_q_values", [(B, 1), (B,)])
        f32 = dict(dtype=t.float32, device=self.device)
        loss = t.empty((), **f32)
        parts, a1, a2 = {}, None, None
        if return_parts:
            H, NL = HIDDEN[self.spec.kind]
            parts = dict(q1=t.empty(B, **f32), q2=t.empty(B, **f32), acts1=[t.empty((B, H), **f32) for _ in range(NL)],
                         acts2=[t.empty((B, H), **f32) for _ in range(NL)])
            a1, a2 = self._ptrs(parts["acts1"]), self._ptrs(parts["acts2"])
        self._attach()
        self._bind_stream()
        rc = self._L.meshenv_critic_grad_backward(
            self._h, B, obs.data_ptr(), act.data_ptr(), y.data_ptr(), loss.data_ptr(),
            parts["q1"].data_ptr() if parts else None, parts["q2"].data_ptr() if parts else None, a1, a2)
        self._check(rc, "meshenv_critic_grad_backward")
        return (loss, parts) if return_parts else loss
