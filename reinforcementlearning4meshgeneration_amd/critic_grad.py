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

import ctypes as C
from dataclasses import dataclass, field
from typing import List

from . import _capi
from .td_target import ACT_DIM, HIDDEN, KIND_SAC, KIND_TD3, OBS_DIM, _critic, _flatten_only
from .policy import _sequential

SUPPORTED_CRITICS = ("twin critics ReLU [128, 128, 128] (SAC) or ReLU [256, 256] (TD3); 18 observations, 3 actions, critic input "
                     "cat(obs, action) = 21, float32")


def _kind_of(q, what):
    """SAC or TD3 from the widths of a q_network (the refusals of a shape that is neither come from td_target._critic)."""
    linears, _ = _sequential(q)
    widths = [tuple(getattr(l.weight, "shape", ()))[:1] for l in linears[:-1]]
    if widths == [(256,)] * 2:
        return KIND_TD3
    if widths == [(128,)] * 3:
        return KIND_SAC
    raise ValueError(f"{what}: hidden layers {[w[0] if w else None for w in widths]}; supported: {SUPPORTED_CRITICS}")


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
        return cls(kind, _critic(q1, kind, "q_networks[0]"), _critic(q2, kind, "q_networks[1]"))

    @classmethod
    def sac(cls, q1, q2) -> "CriticGradSpec":
        return cls._twin(KIND_SAC, q1, q2)

    @classmethod
    def td3(cls, q1, q2) -> "CriticGradSpec":
        return cls._twin(KIND_TD3, q1, q2)

    @classmethod
    def from_sb3(cls, model) -> "CriticGradSpec":
        """Duck-typed on SB3 2.x's SAC / TD3: ``model.critic.q_networks`` (the live critics, not ``critic_target``)."""
        critic = getattr(model, "critic", None)
        if critic is None or not hasattr(critic, "q_networks"):
            raise ValueError(f"{type(model).__name__} has no critic.q_networks: not an SB3 SAC or TD3 model")
        qs = list(critic.q_networks)
        n_critics = int(getattr(critic, "n_critics", len(qs)))
        if n_critics != 2 or len(qs) != 2:
            ddpg = " (DDPG: one critic)" if n_critics == 1 else ""
            raise ValueError(f"n_critics = {n_critics}{ddpg}; the twin critics of SAC / TD3 (n_critics = 2) are supported")
        _flatten_only(critic, "critic", shared=bool(getattr(critic, "share_features_extractor", False)))
        return cls._twin(_kind_of(qs[0], "q_networks[0]"), qs[0], qs[1])

    def check_device(self, device) -> None:
        """Every bound tensor lives on `device` (a torch.device): the kernel reads them through raw pointers."""
        for x in self.tensors():
            if x.device != device:
                raise ValueError(f"a parameter of shape {tuple(x.shape)} is on {x.device}; FusedCriticGrad binds float32 "
                                 f"contiguous CUDA tensors on {device}")


class FusedCriticGrad:
    """A CriticGradSpec bound on one GPU.  backward() returns critic_loss (0-dim float32 CUDA tensor) and overwrites p.grad
    of every bound parameter."""

    def __init__(self, spec: CriticGradSpec, device: int = 0):
        import torch
        self._torch = torch
        self._L = _capi.load()
        if not torch.cuda.is_available():
            raise _capi.MeshEnvError("FusedCriticGrad needs a ROCm GPU")
        self.spec = spec
        self.device = torch.device("cuda", device)
        spec.check_device(self.device)
        self._h = C.c_void_p()
        stream = torch.cuda.current_stream(self.device).cuda_stream
        rc = self._L.meshenv_critic_grad_create(device, C.c_void_p(stream), spec.kind, C.byref(self._h))
        if rc != 0:
            raise _capi.MeshEnvError(f"meshenv_critic_grad_create failed ({rc}): "
                                     f"{self._L.meshenv_critic_grad_last_error(None).decode()}")
        self._stream = stream
        self.grad_buffer = torch.zeros(spec.n_grad, dtype=torch.float32, device=self.device)
        self._views = []
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

    # ---------------------------------------------------------------- plumbing
    def _check(self, rc, what):
        if rc != 0:
            msg = self._L.meshenv_critic_grad_last_error(self._h)
            raise _capi.MeshEnvError(f"{what} failed (code {rc}): {msg.decode() if msg else ''}")

    def _bind_stream(self):
        stream = self._torch.cuda.current_stream(self.device).cuda_stream
        if stream != self._stream:
            self._check(self._L.meshenv_critic_grad_set_stream(self._h, C.c_void_p(stream)), "meshenv_critic_grad_set_stream")
            self._stream = stream

    def bind(self) -> None:
        """Record the parameters' device pointers again: after anything that reallocates them (``.to()``; optimisers and
        ``load_state_dict`` write in place and need no new bind)."""
        s = self.spec
        s.check_device(self.device)
        arr = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])   # noqa: E731
        rc = self._L.meshenv_critic_grad_bind(self._h, arr(s.q1), arr(s.q2), len(s.q1), self.grad_buffer.data_ptr(), s.n_grad)
        self._check(rc, "meshenv_critic_grad_bind")
        self._views = [(p, self.grad_buffer[at:at + p.numel()].view(p.shape)) for p, at in s.offsets()]

    def _attach(self):
        """p.grad of every parameter is its view of the gradient buffer: whatever it held (None, a tensor of the caller's)
        is replaced; host-side pointer comparisons only."""
        for p, v in self._views:
            g = p.grad
            if g is None or g.data_ptr() != v.data_ptr() or g.shape != v.shape or g.dtype != v.dtype or not g.is_contiguous():
                p.grad = v

    def _f32(self, x, name, shape):
        t = self._torch
        if x.requires_grad:
            x = x.detach()
        if x.dtype != t.float32 or not x.is_contiguous() or x.device != self.device:
            x = x.to(device=self.device, dtype=t.float32).contiguous()
        if tuple(x.shape) not in shape:
            raise ValueError(f"{name} must have shape {' or '.join(str(s) for s in shape)}, got {tuple(x.shape)}")
        return x

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
            arr = lambda ts: (C.c_void_p * len(ts))(*[x.data_ptr() for x in ts])   # noqa: E731
            a1, a2 = arr(parts["acts1"]), arr(parts["acts2"])
        self._attach()
        self._bind_stream()
        rc = self._L.meshenv_critic_grad_backward(
            self._h, B, obs.data_ptr(), act.data_ptr(), y.data_ptr(), loss.data_ptr(),
            parts["q1"].data_ptr() if parts else None, parts["q2"].data_ptr() if parts else None, a1, a2)
        self._check(rc, "meshenv_critic_grad_backward")
        return (loss, parts) if return_parts else loss

    def close(self):
        if self._h:
            self._L.meshenv_critic_grad_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
