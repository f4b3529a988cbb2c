"""The loss of PPO and A2C and its gradients on the GPU (include/meshenv_ppo_grad.h, csrc/meshenv_ppo_grad.h): the statement
of SB3 2.x's ``PPO.train`` / ``A2C.train`` that runs once per minibatch,

    values, log_prob, entropy = policy.evaluate_actions(obs, actions)
    advantages = (advantages - advantages.mean()) / (advantages.std() + 1e-8)      # normalize_advantage and B > 1
    ratio = exp(log_prob - old_log_prob)
    policy_loss = -min(advantages * ratio, advantages * clamp(ratio, 1 - clip_range, 1 + clip_range)).mean()
    value_loss = mse_loss(returns, values);  entropy_loss = -mean(entropy)
    loss = policy_loss + ent_coef * entropy_loss + vf_coef * value_loss
    policy.optimizer.zero_grad(); loss.backward(); clip_grad_norm_(policy.parameters(), max_grad_norm)

(``clip_range=None``: A2C's ``policy_loss = -(advantages * log_prob).mean()``) for the recipes the reference runs
(rl/baselines/RL_Mesh.py:113-177: PPO ReLU [128, 128] x 2) and SB3's default A2C (Tanh [64, 64]): pi and vf towers of two hidden
layers of width 64 or 128, ReLU or Tanh, a state-independent ``log_std``, float32.  ``FusedPPOGrad.backward`` returns the
losses and leaves the (clipped) gradients in ``p.grad`` of the 13 LIVE parameters, so ``model.policy.optimizer.step()`` consumes
them as they are.  Every parameter is read as it is at the call; the gradients are views into one flat buffer the object owns
and are OVERWRITTEN by every call.  ``FusedPolicy.bind_live`` + ``refresh()`` then carries the stepped parameters into the
rollout policy without leaving the device (examples/ppo_train_step.py).

``PPOGradSpec`` is the host half (the parameter tensors and every refusal; no device needed)."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import List

from . import _capi
from . import sb3_nets as N
from ._handle import GradBuffer, Handle
from .sb3_nets import ACT_DIM, OBS_DIM

ACTIVATIONS = {"relu": 0, "tanh": 1}
OUTPUTS = ("loss", "policy_loss", "value_loss", "entropy_loss", "approx_kl", "clip_fraction", "grad_norm")
PARTS = ("log_prob", "ratio", "values", "advantages", "pass")


@dataclass
class PPOGradSpec:
    hidden: int
    activation: str
    params: List = field(default_factory=list)   # pi w1 b1 w2 b2 wh bh, vf likewise, log_std: meshenv_ppo_grad_bind's order

    kind_name = "actor_critic"

    def tensors(self):
        return list(self.params)

    # ---------------------------------------------------------------- the flat gradient buffer
    @property
    def n_grad(self) -> int:
        """Floats in the gradient buffer: the 13 parameters in order, padded to a multiple of 64."""
        return (sum(int(p.numel()) for p in self.params) + 63) // 64 * 64

    def offsets(self):
        """[(parameter, first float in the gradient buffer)] for the 13 parameters."""
        out, at = [], 0
        for p in self.params:
            out.append((p, at))
            at += int(p.numel())
        return out

    # ---------------------------------------------------------------- constructors
    @classmethod
    def actor_critic(cls, pi_layers, vf_layers, action_net, value_net, log_std, activation="relu") -> "PPOGradSpec":
        """pi_layers / vf_layers: the two hidden Linear layers of each tower; action_net, value_net: the heads; log_std: the
        [3] parameter; activation: 'relu' / 'tanh' or a torch.nn.ReLU / Tanh class or instance."""
        H, act, params = N.actor_critic_params(pi_layers, vf_layers, action_net, value_net, log_std, activation)
        return cls(H, act, params)

    @classmethod
    def from_sb3(cls, model) -> "PPOGradSpec":
        """Duck-typed on SB3 2.x's PPO / A2C (through ``.policy``) or an ``ActorCriticPolicy``.  The hyper-parameters
        (clip_range, ent_coef, vf_coef, max_grad_norm) are NOT frozen here: pass the model's current ones to backward()."""
        N.no_value_clip(model)
        return cls(*N.actor_critic_live(model))

    def check_device(self, device) -> None:
        """Every bound tensor lives on `device` (a torch.device): the kernel reads them through raw pointers."""
        N.check_device(self.tensors(), device, "FusedPPOGrad")


class FusedPPOGrad(GradBuffer, Handle):
    """A PPOGradSpec bound on one GPU.  backward() returns the losses (0-dim float32 CUDA tensors) and overwrites p.grad of
    the policy's 13 parameters."""
    PREFIX = "meshenv_ppo_grad"

    def __init__(self, spec: PPOGradSpec, device: int = 0):
        self.spec = spec
        super().__init__(device, check_device=spec.check_device)
        self._alloc_grads()
        self.bind()

    kind = "actor_critic"

    @classmethod
    def actor_critic(cls, pi_layers, vf_layers, action_net, value_net, log_std, activation="relu", device: int = 0):
        return cls(PPOGradSpec.actor_critic(pi_layers, vf_layers, action_net, value_net, log_std, activation), device)

    @classmethod
    def from_sb3(cls, model, device: int = 0):
        return cls(PPOGradSpec.from_sb3(model), device)

    def bind(self) -> None:
        """Record the parameters' device pointers again: after anything that reallocates them (``.to()``; optimisers and
        ``load_state_dict`` write in place and need no new bind)."""
        s = self.spec
        s.check_device(self.device)
        assert s.n_grad == _capi.PPO_GRAD_FLOATS[s.hidden]
        rc = self._L.meshenv_ppo_grad_bind(self._h, s.hidden, ACTIVATIONS[s.activation], self._ptrs(s.params), len(s.params),
                                           self.grad_buffer.data_ptr(), s.n_grad)
        self._check(rc, "meshenv_ppo_grad_bind")
        self._view_grads()

    # ---------------------------------------------------------------- public
    def backward(self, rollout_data=None, *, observations=None, actions=None, old_log_prob=None, advantages=None, returns=None,
                 clip_range=0.2, ent_coef=0.0, vf_coef=0.5, normalize_advantage=True, max_grad_norm=0.5,
                 return_parts: bool = False):
        """The loss of a minibatch and its gradients: ``rollout_data`` (anything with SB3's RolloutBufferSamples fields:
        observations, actions, old_log_prob, advantages, returns) or the five tensors by keyword.  At most four launches on
        the current stream, no synchronisation; no argument is written.

        clip_range=None selects A2C's loss (old_log_prob is not read); max_grad_norm=None skips clip_grad_norm_ (grad_norm is
        then NaN).  Returns a dict of 0-dim float32 CUDA tensors: loss, policy_loss, value_loss, entropy_loss, approx_kl,
        clip_fraction, grad_norm (the total norm before clipping).

        return_parts: the dict also holds log_prob, ratio, values, advantages (as used: normalised) and pass (1.0 where the
        row's surrogate passes its gradient) [B] each, and acts_pi, acts_vf: the two [B, H] kept activations of each tower."""
        t = self._torch
        if rollout_data is not None:
            if any(x is not None for x in (observations, actions, old_log_prob, advantages, returns)):
                raise ValueError("pass either rollout_data or the tensors by keyword")
            observations, actions, advantages, returns = (rollout_data.observations, rollout_data.actions, rollout_data.advantages,
                                                          rollout_data.returns)
            old_log_prob = getattr(rollout_data, "old_log_prob", None)
        a2c = clip_range is None
        if observations is None or actions is None or advantages is None or returns is None or (old_log_prob is None and not a2c):
            raise ValueError("observations, actions, advantages, returns and (for PPO's loss) old_log_prob are required")
        if observations.dim() != 2 or observations.shape[0] == 0:
            raise ValueError(f"observations must have shape (B, {OBS_DIM}), got {tuple(observations.shape)}")
        clip = 0.0 if a2c else N.finite(clip_range, "clip_range")
        if not a2c and not clip > 0.0:
            raise ValueError(f"clip_range must be > 0 (or None for A2C's loss), got {clip_range!r}")
        ent, vf = N.finite(ent_coef, "ent_coef"), N.finite(vf_coef, "vf_coef")
        mgn = 0.0 if max_grad_norm is None else N.finite(max_grad_norm, "max_grad_norm")
        if max_grad_norm is not None and not mgn > 0.0:
            raise ValueError(f"max_grad_norm must be > 0 (or None), got {max_grad_norm!r}")
        B, H = int(observations.shape[0]), self.spec.hidden
        obs = self._f32(observations, "observations", [(B, OBS_DIM)])
        act = self._f32(actions, "actions", [(B, ACT_DIM)])
        adv = self._f32(advantages, "advantages", [(B,), (B, 1)])
        ret = self._f32(returns, "returns", [(B,), (B, 1)])
        old = None if a2c else self._f32(old_log_prob, "old_log_prob", [(B,), (B, 1)])
        f32 = dict(dtype=t.float32, device=self.device)
        out = t.empty(_capi.PPO_GRAD_OUTPUTS, **f32)
        parts, pp, pa = {}, None, None
        if return_parts:
            parts = {k: t.empty(B, **f32) for k in PARTS}
            pp = self._ptrs(list(parts.values()))
            for k in ("acts_pi", "acts_vf"):
                parts[k] = [t.empty((B, H), **f32) for _ in range(2)]
            pa = self._ptrs(parts["acts_pi"] + parts["acts_vf"])
        self._attach()
        self._bind_stream()
        rc = self._L.meshenv_ppo_grad_backward(self._h, B, obs.data_ptr(), act.data_ptr(), None if old is None else old.data_ptr(),
                                               adv.data_ptr(), ret.data_ptr(), 1 if a2c else 0, C.c_double(clip), C.c_float(ent),
                                               C.c_float(vf), 1 if normalize_advantage else 0, 0 if max_grad_norm is None else 1,
                                               C.c_float(mgn), out.data_ptr(), pp, pa)
        self._check(rc, "meshenv_ppo_grad_backward")
        res = {k: out[i] for i, k in enumerate(OUTPUTS)}
        res.update(parts)
        return res
