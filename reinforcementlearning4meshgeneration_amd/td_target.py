"""TD targets of SAC, TD3 and DDPG on the GPU (include/meshenv.h: meshenv_target_*, csrc/meshenv_target.h, csrc/meshenv_wide.h): the
``with th.no_grad():`` block of SB3 2.x's ``SAC.train`` / ``TD3.train`` that turns a sampled batch into ``target_q_values``,
one launch from the tensors ``DeviceReplayBuffer.sample`` returns.

Three kinds, the networks the reference trains (rl/baselines/RL_Mesh.py:113-228):

* SAC: actor ReLU [128, 128, 128] with ``mu`` / ``log_std`` heads, twin critics ReLU [128, 128, 128];
* TD3: ``actor_target`` ReLU [256, 256] + tanh, twin critics ReLU [256, 256];
* DDPG (``DDPG('MlpPolicy', env)``: SB3's defaults): ``actor_target`` ReLU [400, 300] + tanh, ONE critic ReLU [400, 300];
  ``TD3.train``'s block with ``n_critics = 1``, so no twin minimum and no ``q2``.  SB3's DDPG sets
  ``target_policy_noise = 0.1`` and ``target_noise_clip = 0.0``: the smoothing noise is clipped to +-0.

The weights are the LIVE torch parameters on the device: ``FusedTDTarget`` records their pointers once and ``refresh()``
copies them into the kernel's layout in one launch on the current stream (no host copy, no synchronisation), so a training
loop calls ``refresh()`` after its optimiser / Polyak steps and ``target(...)`` after ``sample``.  ``TDTargetSpec`` is the
host half (kind, constants, the parameter tensors and every refusal; no device needed).  Layers are ``torch.nn.Linear``-like
objects (``.weight [out][in]``, ``.bias``)."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import List, Optional

from . import sb3_nets as N
from ._handle import Handle
from .sb3_nets import ACT_DIM, HIDDEN, KIND_DDPG, KIND_SAC, KIND_TD3, OBS_DIM, SUPPORTED  # noqa: F401  (part of this module's interface)


@dataclass
class TDTargetSpec:
    kind: int
    gamma: float
    actor: List = field(default_factory=list)     # the tensors in meshenv_target_bind's order
    q1: List = field(default_factory=list)
    q2: List = field(default_factory=list)
    log_ent_coef: Optional[object] = None         # SAC: the learned [1] tensor, or None with a fixed ent_coef
    ent_coef: float = 0.0
    policy_noise: float = 0.0
    noise_clip: float = 0.0

    @property
    def kind_name(self) -> str:
        return {KIND_SAC: "sac", KIND_TD3: "td3", KIND_DDPG: "ddpg"}[self.kind]

    @property
    def hidden(self) -> int:
        """The hidden width (DDPG: the first of its two, sb3_nets.DDPG_WIDTHS)."""
        return N.DDPG_WIDTHS[0] if self.kind == KIND_DDPG else HIDDEN[self.kind][0]

    def tensors(self):
        return list(self.actor) + list(self.q1) + list(self.q2) + ([self.log_ent_coef] if self.log_ent_coef is not None else [])

    @staticmethod
    def _gamma(gamma):
        g = float(gamma)
        if not 0.0 <= g <= 1.0:
            raise ValueError(f"gamma must lie in [0, 1], got {gamma!r}")
        return g

    # ---------------------------------------------------------------- constructors
    @classmethod
    def sac(cls, actor_layers, mu, log_std, q1, q2, gamma, log_ent_coef=None, ent_coef=None) -> "TDTargetSpec":
        lec, fixed = N.ent_coef(log_ent_coef, ent_coef)
        return cls(KIND_SAC, cls._gamma(gamma), N.sac_actor_params(actor_layers, mu, log_std), *N.twin_params(KIND_SAC, q1, q2),
                   log_ent_coef=lec, ent_coef=fixed)

    @classmethod
    def td3(cls, actor_layers, mu, q1, q2, gamma, policy_noise=0.2, noise_clip=0.5) -> "TDTargetSpec":
        pn, nc = cls._noise(policy_noise, noise_clip)
        actor = N._mlp(actor_layers, [("mu", ACT_DIM, mu)], OBS_DIM, KIND_TD3, "actor")
        return cls(KIND_TD3, cls._gamma(gamma), actor, *N.twin_params(KIND_TD3, q1, q2), policy_noise=pn, noise_clip=nc)

    @staticmethod
    def _noise(policy_noise, noise_clip):
        pn, nc = float(policy_noise), float(noise_clip)
        if not (0.0 <= pn < float("inf")) or not (0.0 <= nc < float("inf")):
            raise ValueError(f"policy_noise and noise_clip must be finite and >= 0, got {policy_noise!r}, {noise_clip!r}")
        return pn, nc

    @classmethod
    def ddpg(cls, actor_layers, mu, q1, gamma, policy_noise=0.1, noise_clip=0.0) -> "TDTargetSpec":
        """actor_target's two hidden layers and mu, critic_target.q_networks[0]; the defaults are what SB3's DDPG passes."""
        pn, nc = cls._noise(policy_noise, noise_clip)
        return cls(KIND_DDPG, cls._gamma(gamma), N.ddpg_actor_params(actor_layers, mu), N.ddpg_critic_params(q1), [],
                   policy_noise=pn, noise_clip=nc)

    @classmethod
    def from_sb3(cls, model) -> "TDTargetSpec":
        """Duck-typed on SB3 2.x's SAC (``actor.latent_pi / .mu / .log_std``, ``critic_target.q_networks``, ``gamma``,
        ``log_ent_coef`` or ``ent_coef_tensor``) and TD3 (``actor_target.mu``, ``critic_target.q_networks``, ``gamma``,
        ``target_policy_noise``, ``target_noise_clip``); DDPG is TD3's layout with ``critic_target.n_critics == 1`` and the
        widths [400, 300] on both networks (``sb3_nets.is_ddpg``) -- every other single-critic model is refused."""
        is_sac = hasattr(getattr(model, "actor", None), "latent_pi")
        is_td3 = not is_sac and hasattr(getattr(model, "actor_target", None), "mu")
        if is_td3 and N.is_ddpg(model):
            layers, mu, q = N.ddpg_target_nets(model)
            return cls.ddpg(layers, mu, q, model.gamma, model.target_policy_noise, model.target_noise_clip)
        qs = N.twin_critics(model, "critic_target", ddpg=is_td3)
        if is_sac:
            actor = model.actor
            return cls.sac(N.sac_actor(actor), actor.mu, actor.log_std, qs[0], qs[1], model.gamma, **N.model_ent_coef(model))
        if is_td3:
            return cls.td3(*N.td3_actor(model.actor_target), qs[0], qs[1], model.gamma, model.target_policy_noise,
                           model.target_noise_clip)
        raise ValueError(f"{type(model).__name__} has neither SAC's actor.latent_pi nor TD3's actor_target.mu")

    def check_device(self, device) -> None:
        """Every bound tensor lives on `device` (a torch.device): the kernel reads them through raw pointers."""
        N.check_device(self.tensors(), device, "FusedTDTarget")


class FusedTDTarget(Handle):
    """A TDTargetSpec bound on one GPU.  target() returns target_q_values [B, 1] as a float32 CUDA tensor."""
    PREFIX = "meshenv_target"

    def __init__(self, spec: TDTargetSpec, device: int = 0):
        self.spec = spec
        super().__init__(device, spec.kind, spec.gamma, spec.ent_coef, spec.policy_noise, spec.noise_clip,
                         check_device=spec.check_device)
        self.bind()
        self.refresh()

    @property
    def kind(self) -> str:
        return self.spec.kind_name

    @classmethod
    def sac(cls, actor_layers, mu, log_std, q1, q2, gamma, log_ent_coef=None, ent_coef=None, device: int = 0):
        return cls(TDTargetSpec.sac(actor_layers, mu, log_std, q1, q2, gamma, log_ent_coef, ent_coef), device)

    @classmethod
    def td3(cls, actor_layers, mu, q1, q2, gamma, policy_noise=0.2, noise_clip=0.5, device: int = 0):
        return cls(TDTargetSpec.td3(actor_layers, mu, q1, q2, gamma, policy_noise, noise_clip), device)

    @classmethod
    def ddpg(cls, actor_layers, mu, q1, gamma, policy_noise=0.1, noise_clip=0.0, device: int = 0):
        return cls(TDTargetSpec.ddpg(actor_layers, mu, q1, gamma, policy_noise, noise_clip), device)

    @classmethod
    def from_sb3(cls, model, device: int = 0):
        return cls(TDTargetSpec.from_sb3(model), device)

    def bind(self) -> None:
        """Record the parameters' device pointers again: after anything that reallocates them (``.to()``; SB3's optimisers,
        ``polyak_update`` and ``load_state_dict`` write in place and need no new bind).  Follow with refresh()."""
        s = self.spec
        s.check_device(self.device)
        arr = self._ptrs
        lec = s.log_ent_coef.data_ptr() if s.log_ent_coef is not None else None
        rc = self._L.meshenv_target_bind(self._h, arr(s.actor), len(s.actor), arr(s.q1), arr(s.q2) if s.q2 else None, len(s.q1), lec)
        self._check(rc, "meshenv_target_bind")

    def refresh(self) -> None:
        """Snapshot the live parameters (and log_ent_coef) into the kernel's layout: one launch on the current stream, no
        synchronisation.  target() uses the values of the last refresh."""
        self._bind_stream()
        self._check(self._L.meshenv_target_refresh(self._h), "meshenv_target_refresh")

    # ---------------------------------------------------------------- public
    def target(self, samples=None, *, next_observations=None, rewards=None, dones=None, noise=None, seed=None,
               counter: int = 0, return_parts: bool = False):
        """target_q_values [B, 1] of a batch: ``samples`` (a ReplayBufferSamples: next_observations, rewards, dones are
        read) or the three tensors by keyword.  eps is ``noise`` ([B, 3] of N(0, 1) draws), drawn in the kernel when ``seed``
        is given (Philox4x32-10 at (seed, counter, sample index), a stream of its own: pass a fresh counter every batch), or
        0 with neither.  return_parts: also a dict of next_actions [B, 3] (in [-1, 1]), next_log_prob [B] (SAC), q1, q2 [B] (DDPG: q1)
        and, with noise, eps [B, 3]; target(noise=parts["eps"]) reproduces a sampled call bit for bit."""
        t = self._torch
        if samples is not None:
            if next_observations is not None or rewards is not None or dones is not None:
                raise ValueError("pass either samples or next_observations / rewards / dones")
            next_observations, rewards, dones = samples.next_observations, samples.rewards, samples.dones
        if next_observations is None or rewards is None or dones is None:
            raise ValueError("next_observations, rewards and dones are required")
        if noise is not None and seed is not None:
            raise ValueError("pass either noise or seed")
        if next_observations.dim() != 2 or next_observations.shape[0] == 0:
            raise ValueError(f"next_observations must have shape (B, {OBS_DIM}), got {tuple(next_observations.shape)}")
        B = int(next_observations.shape[0])
        obs = self._f32(next_observations, "next_observations", [(B, OBS_DIM)])
        rew = self._f32(rewards, "rewards", [(B, 1), (B,)])
        don = self._f32(dones, "dones", [(B, 1), (B,)])
        if noise is not None:
            noise = self._f32(noise, "noise", [(B, ACT_DIM)])
        f32 = dict(dtype=t.float32, device=self.device)
        y = t.empty((B, 1), **f32)
        parts = {}
        if return_parts:
            parts = dict(next_actions=t.empty((B, ACT_DIM), **f32), q1=t.empty(B, **f32))
            if self.spec.kind != KIND_DDPG:
                parts["q2"] = t.empty(B, **f32)
            if self.spec.kind == KIND_SAC:
                parts["next_log_prob"] = t.empty(B, **f32)
            if noise is not None or seed is not None:
                parts["eps"] = t.empty((B, ACT_DIM), **f32)
        ptr = lambda k: parts[k].data_ptr() if k in parts else None   # noqa: E731
        self._bind_stream()
        rc = self._L.meshenv_target_forward(
            self._h, B, obs.data_ptr(), rew.data_ptr(), don.data_ptr(), noise.data_ptr() if noise is not None else None,
            1 if seed is not None else 0, C.c_uint64((seed or 0) & (2 ** 64 - 1)), C.c_uint64(int(counter) & (2 ** 64 - 1)),
            y.data_ptr(), ptr("next_actions"), ptr("next_log_prob"), ptr("q1"), ptr("q2"), ptr("eps"))
        self._check(rc, "meshenv_target_forward")
        return (y, parts) if return_parts else y
