"""Fused PPO / A2C / TD3 / DDPG policy forward on the GPU (include/meshenv.h: meshenv_policy_*, csrc/meshenv_policy.h,
csrc/meshenv_wide.h): the policy side of the rollout loop for the reference's on-policy and deterministic-actor algorithms
(rl/baselines/RL_Mesh.py:113-228), so that observation -> action -> step stays on the device.

Two kinds, two hidden layers of width 64, 128 or 256, ReLU or Tanh:

* actor-critic (SB3 ``ActorCriticPolicy``: PPO with ``net_arch=dict(pi=[128, 128], vf=[128, 128])``, A2C with the SB3
  defaults Tanh [64, 64]): outputs ``actions`` (clipped to the Box, what ``collect_rollouts`` hands to ``env.step``),
  ``buffer_actions`` (the unclipped Gaussian sample that ``RolloutBuffer`` stores), ``log_prob`` and ``value``;
* deterministic (SB3 ``TD3Policy``, ``actor.mu``; TD3 [256, 256] ReLU): ``buffer_actions`` = the tanh action in [-1, 1]
  (plus ``NormalActionNoise(0, sigma)``, clipped) that ``ReplayBuffer`` stores, ``actions`` = it rescaled to the Box.

DDPG, which the reference builds as ``DDPG('MlpPolicy', env)``, has SB3's default ``net_arch`` [400, 300] with ReLU: the
deterministic kind with two widths, a kernel family of its own (csrc/meshenv_wide.h).  It is asked for by name --
``PolicySpec.ddpg`` / ``FusedPolicy.ddpg``, or ``from_sb3`` of a DDPG model (``actor.mu`` [400, 300] beside ONE [400, 300]
critic) -- so that ``deterministic(...)`` and ``from_sb3`` of any other object keep refusing what they refused before.

``PolicySpec`` is the host half (shapes, kind, weights as float32 arrays; no device needed); ``FusedPolicy`` loads one on
a GPU.  Layers are ``torch.nn.Linear``-like objects (``.weight [out][in]``, ``.bias``)."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Dict, Optional

import numpy as np

from . import _capi
from ._handle import Handle
from . import sb3_nets as N
from .sb3_nets import _sequential
from .vec_env import ACTION_HIGH, ACTION_LOW

KIND_ACTOR_CRITIC, KIND_DETERMINISTIC = 0, 1
ACTIVATIONS = {"relu": 0, "tanh": 1}
HIDDEN_WIDTHS = (64, 128, 256)
DDPG_SUPPORTED = ("PolicySpec.ddpg, or from_sb3 of a DDPG model (one [400, 300] critic): DDPG's ReLU [400, 300] tanh actor, Linear(18, 400), "
                  "Linear(400, 300), Linear(300, 3)")
SUPPORTED = ("two hidden layers of width 64, 128 or 256 (the same width), ReLU or Tanh, 18 inputs, 3 actions: "
             "actor-critic (pi and vf towers, action_net [3], value_net [1], log_std [3]) or deterministic (tanh actor); or, by "
             "name, " + DDPG_SUPPORTED)


def _np(x, what):
    if hasattr(x, "detach"):
        x = x.detach().cpu().numpy()
    a = np.ascontiguousarray(np.asarray(x, dtype=np.float32))
    if not np.all(np.isfinite(a)):
        raise ValueError(f"{what} holds non-finite values")
    return a


def _activation(act) -> str:
    """'relu' / 'tanh', a torch.nn.ReLU / Tanh class or instance."""
    name = act if isinstance(act, str) else (act.__name__ if isinstance(act, type) else type(act).__name__)
    name = name.lower()
    if name not in ACTIVATIONS:
        raise ValueError(f"unsupported activation {act!r}; supported: {SUPPORTED}")
    return name


@dataclass
class PolicySpec:
    kind: int
    hidden: int
    activation: str
    weights: Dict[str, Optional[np.ndarray]] = field(default_factory=dict)
    low: np.ndarray = field(default_factory=lambda: ACTION_LOW.copy())
    high: np.ndarray = field(default_factory=lambda: ACTION_HIGH.copy())
    hidden2: Optional[int] = None      # DDPG's second width (hidden is then the first); None: both layers are `hidden` wide

    @property
    def kind_name(self) -> str:
        return "actor_critic" if self.kind == KIND_ACTOR_CRITIC else "deterministic"

    @property
    def widths(self):
        return (self.hidden, self.hidden if self.hidden2 is None else self.hidden2)

    # ---------------------------------------------------------------- constructors
    @staticmethod
    def _tower(layers, head, n_out, what):
        layers = list(layers)
        if len(layers) != 2:
            raise ValueError(f"{what}: {len(layers)} hidden layers; supported: {SUPPORTED}")
        w1, b1 = _np(layers[0].weight, f"{what}[0].weight"), _np(layers[0].bias, f"{what}[0].bias")
        w2, b2 = _np(layers[1].weight, f"{what}[1].weight"), _np(layers[1].bias, f"{what}[1].bias")
        wh, bh = _np(head.weight, f"{what} head weight"), _np(head.bias, f"{what} head bias")
        H = w1.shape[0]
        if H not in HIDDEN_WIDTHS or w1.shape != (H, _capi.OBS_DIM) or b1.shape != (H,) or w2.shape != (H, H) or \
                b2.shape != (H,) or wh.shape != (n_out, H) or bh.shape != (n_out,):
            raise ValueError(f"{what}: unsupported shapes {[w1.shape, w2.shape, wh.shape]}; supported: {SUPPORTED}")
        return H, (w1, b1, w2, b2, wh, bh)

    @classmethod
    def actor_critic(cls, pi_layers, vf_layers, action_net, value_net, log_std, activation="relu", low=ACTION_LOW,
                     high=ACTION_HIGH) -> "PolicySpec":
        H, pi = cls._tower(pi_layers, action_net, 3, "pi")
        Hv, vf = cls._tower(vf_layers, value_net, 1, "vf")
        if Hv != H:
            raise ValueError(f"pi width {H} and vf width {Hv} differ; supported: {SUPPORTED}")
        ls = _np(log_std, "log_std").reshape(-1)
        if ls.shape != (3,):
            raise ValueError(f"log_std must hold 3 values (state-independent), got shape {ls.shape}")
        names = ("w1", "b1", "w2", "b2", "wh", "bh")
        w = {f"pi_{k}": v for k, v in zip(names, pi)}
        w.update({f"vf_{k}": v for k, v in zip(names, vf)})
        w["log_std_or_sigma"] = ls
        return cls(KIND_ACTOR_CRITIC, H, _activation(activation), w, _np(low, "low"), _np(high, "high"))

    @classmethod
    def deterministic(cls, layers, mu, activation="relu", sigma=None, low=ACTION_LOW, high=ACTION_HIGH) -> "PolicySpec":
        H, pi = cls._tower(layers, mu, 3, "actor")
        w = {f"pi_{k}": v for k, v in zip(("w1", "b1", "w2", "b2", "wh", "bh"), pi)}
        w.update({f"vf_{k}": None for k in ("w1", "b1", "w2", "b2", "wh", "bh")})
        w["log_std_or_sigma"] = cls._sigma(sigma)
        return cls(KIND_DETERMINISTIC, H, _activation(activation), w, _np(low, "low"), _np(high, "high"))

    @staticmethod
    def _sigma(sigma):
        """NormalActionNoise's sigma as a [3] float32 vector, or None (no action noise)."""
        if sigma is None:
            return None
        s = _np(sigma, "sigma")
        s = np.broadcast_to(s, (3,)).astype(np.float32).copy() if s.size in (1, 3) else s
        if s.shape != (3,) or (s < 0).any():
            raise ValueError(f"sigma must be a non-negative scalar or [3] vector, got {sigma!r}")
        return s

    @classmethod
    def ddpg(cls, layers, mu, sigma=None, low=ACTION_LOW, high=ACTION_HIGH) -> "PolicySpec":
        """DDPG's actor: ReLU [400, 300], ``layers`` = [Linear(18, 400), Linear(400, 300)], ``mu`` = Linear(300, 3)."""
        layers = list(layers)
        what = "actor"
        if len(layers) != 2:
            raise ValueError(f"{what}: {len(layers)} hidden layers; supported: {DDPG_SUPPORTED}")
        t = [_np(layers[0].weight, f"{what}[0].weight"), _np(layers[0].bias, f"{what}[0].bias"),
             _np(layers[1].weight, f"{what}[1].weight"), _np(layers[1].bias, f"{what}[1].bias"),
             _np(mu.weight, f"{what} head weight"), _np(mu.bias, f"{what} head bias")]
        H1, H2 = N.DDPG_WIDTHS
        if [a.shape for a in t] != [(H1, _capi.OBS_DIM), (H1,), (H2, H1), (H2,), (3, H2), (3,)]:
            raise ValueError(f"{what}: unsupported shapes {[t[0].shape, t[2].shape, t[4].shape]}; supported: {DDPG_SUPPORTED}")
        w = {f"pi_{k}": v for k, v in zip(("w1", "b1", "w2", "b2", "wh", "bh"), t)}
        w.update({f"vf_{k}": None for k in ("w1", "b1", "w2", "b2", "wh", "bh")})
        w["log_std_or_sigma"] = cls._sigma(sigma)
        return cls(KIND_DETERMINISTIC, H1, "relu", w, _np(low, "low"), _np(high, "high"), hidden2=H2)

    @classmethod
    def from_sb3(cls, policy, sigma=None, low=ACTION_LOW, high=ACTION_HIGH) -> "PolicySpec":
        """Duck-typed on SB3 2.x: ``ActorCriticPolicy`` (mlp_extractor.policy_net / .value_net, action_net, value_net,
        log_std) or ``TD3Policy`` (actor.mu = Sequential(Linear, act, Linear, act, Linear, Tanh)).  An algorithm object
        (``PPO(...)``) is unwrapped through its ``.policy``.  sigma: TD3's NormalActionNoise sigma (deterministic kind).
        A DDPG model (``sb3_nets.is_ddpg``: actor.mu [400, 300] beside one [400, 300] critic) gives ``PolicySpec.ddpg``."""
        if not hasattr(policy, "mlp_extractor") and not hasattr(policy, "actor") and hasattr(policy, "policy"):
            policy = policy.policy
        for attr in ("features_extractor", "pi_features_extractor", "vf_features_extractor"):
            fe = getattr(policy, attr, None)
            if fe is not None and type(fe).__name__ != "FlattenExtractor":
                raise ValueError(f"{attr} is {type(fe).__name__}; only the MLP policies' FlattenExtractor is supported")
        if hasattr(policy, "mlp_extractor"):
            if getattr(policy, "use_sde", False) or getattr(policy, "squash_output", False):
                raise ValueError("gSDE / squashed actor-critic policies are not supported; " + SUPPORTED)
            ext = policy.mlp_extractor
            pi, pi_acts = _sequential(ext.policy_net)
            vf, vf_acts = _sequential(ext.value_net)
            acts = pi_acts | vf_acts
            if len(acts) != 1:
                raise ValueError(f"activations {sorted(acts)}; supported: {SUPPORTED}")
            return cls.actor_critic(pi, vf, policy.action_net, policy.value_net, policy.log_std, activation=acts.pop(),
                                    low=low, high=high)
        if hasattr(policy, "actor") and hasattr(policy.actor, "mu"):
            mods = list(policy.actor.mu)
            if not mods or type(mods[-1]).__name__ != "Tanh":
                raise ValueError("actor.mu must end in Tanh (SB3 TD3 / DDPG actor); " + SUPPORTED)
            linears, acts = _sequential(mods[:-1])
            if len(acts) != 1 or len(linears) != 3:
                raise ValueError(f"actor.mu: {len(linears) - 1} hidden layers, activations {sorted(acts)}; supported: {SUPPORTED}")
            if N.is_ddpg(policy, "actor", "critic"):
                if acts != {"relu"}:
                    raise ValueError(f"actor.mu: activations {sorted(acts)}; supported: {SUPPORTED}")
                return cls.ddpg(linears[:2], linears[2], sigma=sigma, low=low, high=high)
            return cls.deterministic(linears[:2], linears[2], activation=acts.pop(), sigma=sigma, low=low, high=high)
        raise ValueError("not an SB3 ActorCriticPolicy (mlp_extractor) or TD3Policy (actor.mu)")

    def load_args(self):
        """Host pointers in the order of meshenv_policy_load (the arrays stay referenced by self.weights); with two widths, of
        meshenv_policy_load_widths."""
        if self.hidden2 is not None:
            w = self.weights
            ptrs = [w[k].ctypes.data if w.get(k) is not None else None
                    for k in ("pi_w1", "pi_b1", "pi_w2", "pi_b2", "pi_wh", "pi_bh", "log_std_or_sigma")]
            return ptrs + [self.low.ctypes.data, self.high.ctypes.data]
        w = self.weights
        order = ("pi_w1", "pi_b1", "pi_w2", "pi_b2", "pi_wh", "pi_bh", "vf_w1", "vf_b1", "vf_w2", "vf_b2", "vf_wh", "vf_bh",
                 "log_std_or_sigma")
        ptrs = [w[k].ctypes.data if w.get(k) is not None else None for k in order]
        return ptrs + [self.low.ctypes.data, self.high.ctypes.data]


def live_deterministic(model):
    """(first hidden width, activation, the six live tensors w1 b1 w2 b2 w3 b3) of the LIVE actor of an SB3 TD3 ([256, 256]) or
    DDPG ([400, 300]) model, TD3Policy or Actor, through ``sb3_nets.td3_live_actor`` (its refusals: a SAC model, no Tanh tail,
    other widths, non-float32 parameters)."""
    if not hasattr(model, "actor") and hasattr(model, "mu"):
        import types
        model = types.SimpleNamespace(actor=model)
    widths, params = N.deterministic_live_params(model)
    return widths[0], "relu", params


class FusedPolicy(Handle):
    """A PolicySpec loaded on one GPU.  forward / sample / value return dicts of float32 CUDA tensors."""
    PREFIX = "meshenv_policy"
    LAST_ERROR = "meshenv_last_error"

    def __init__(self, spec: PolicySpec, device: int = 0):
        self.spec = spec
        super().__init__(device)
        if spec.hidden2 is not None:
            rc = self._L.meshenv_policy_load_widths(self._h, spec.kind, spec.hidden, spec.hidden2, ACTIVATIONS[spec.activation],
                                                    *spec.load_args())
            self._check(rc, "meshenv_policy_load_widths")
            return
        rc = self._L.meshenv_policy_load(self._h, spec.kind, spec.hidden, ACTIVATIONS[spec.activation], *spec.load_args())
        self._check(rc, "meshenv_policy_load")

    @property
    def kind(self) -> str:
        return self.spec.kind_name

    @classmethod
    def actor_critic(cls, pi_layers, vf_layers, action_net, value_net, log_std, activation="relu", device: int = 0,
                     low=ACTION_LOW, high=ACTION_HIGH):
        return cls(PolicySpec.actor_critic(pi_layers, vf_layers, action_net, value_net, log_std, activation, low, high), device)

    @classmethod
    def deterministic(cls, layers, mu, activation="relu", sigma=None, device: int = 0, low=ACTION_LOW, high=ACTION_HIGH):
        return cls(PolicySpec.deterministic(layers, mu, activation, sigma, low, high), device)

    @classmethod
    def ddpg(cls, layers, mu, sigma=None, device: int = 0, low=ACTION_LOW, high=ACTION_HIGH):
        return cls(PolicySpec.ddpg(layers, mu, sigma, low, high), device)

    @classmethod
    def from_sb3(cls, policy, sigma=None, device: int = 0, low=ACTION_LOW, high=ACTION_HIGH):
        return cls(PolicySpec.from_sb3(policy, sigma, low, high), device)

    # ---------------------------------------------------------------- live parameters
    def bind_live(self, policy) -> None:
        """Record the LIVE parameters of ``policy`` (an SB3 ActorCriticPolicy, or a PPO / A2C object through ``.policy``; for
        the deterministic kind an SB3 TD3 model, TD3Policy or Actor: ``actor.mu``) so that refresh() can carry them into this
        object's packed weights: what SB3 does implicitly when collect_rollouts reads the parameters
        ``policy.optimizer.step()`` has just written.  The shapes and the activation must be the loaded ones and the tensors
        on this device.  Again after anything that reallocates the parameters (``.to()``)."""
        if self.spec.kind != KIND_ACTOR_CRITIC:
            # the deterministic kind: the live actor of an SB3 TD3 or DDPG model (``model.actor``, ReLU [256, 256] or
            # [400, 300], six tensors); sigma, low and high stay as loaded
            _, act, params = live_deterministic(policy)
            widths = (int(params[0].shape[0]), int(params[2].shape[0]))
        else:
            H, act, params = N.actor_critic_live(policy, widths=HIDDEN_WIDTHS)
            widths = (H, H)
        if tuple(widths) != self.spec.widths or act != self.spec.activation:
            raise ValueError(f"the live policy is {act} {list(widths)}; this FusedPolicy was loaded as {self.spec.activation} "
                             f"{list(self.spec.widths)}")
        N.check_device(params, self.device, "FusedPolicy.bind_live")
        rc = self._L.meshenv_policy_bind(self._h, self._ptrs(params), len(params))
        self._check(rc, "meshenv_policy_bind")
        self._live = params      # keeps the storages alive

    def refresh(self) -> None:
        """The bound parameters, as they are now, into the packed weights: one launch on the current stream, no host copy, no
        synchronisation.  Launches that follow on the same stream see the new weights."""
        if getattr(self, "_live", None) is None:
            raise ValueError("refresh() needs bind_live(policy) first")
        self._bind_stream()
        self._check(self._L.meshenv_policy_refresh(self._h), "meshenv_policy_refresh")

    def _obs(self, obs):
        t = self._torch
        if obs.dtype != t.float32 or not obs.is_contiguous() or obs.device != self.device:
            obs = obs.to(device=self.device, dtype=t.float32).contiguous()
        if obs.dim() != 2 or obs.shape[1] != _capi.OBS_DIM or obs.shape[0] == 0:
            raise ValueError(f"obs must have shape (n, {_capi.OBS_DIM}), got {tuple(obs.shape)}")
        return obs

    def _outputs(self, n, eps: bool):
        t = self._torch
        out = dict(actions=t.empty((n, 3), dtype=t.float32, device=self.device),
                   buffer_actions=t.empty((n, 3), dtype=t.float32, device=self.device))
        if self.spec.kind == KIND_ACTOR_CRITIC:
            out["log_prob"] = t.empty(n, dtype=t.float32, device=self.device)
            out["value"] = t.empty(n, dtype=t.float32, device=self.device)
        if eps:
            out["eps"] = t.empty((n, 3), dtype=t.float32, device=self.device)
        return out

    def _launch(self, obs, noise, sample, seed, counter, out):
        ptr = lambda k: out[k].data_ptr() if k in out else None   # noqa: E731
        self._bind_stream()
        rc = self._L.meshenv_policy_forward(self._h, obs.shape[0], obs.data_ptr(), noise.data_ptr() if noise is not None else None,
                                            1 if sample else 0, C.c_uint64(seed & (2 ** 64 - 1)),
                                            C.c_uint64(counter & (2 ** 64 - 1)), ptr("actions"), ptr("buffer_actions"),
                                            ptr("log_prob"), ptr("value"), ptr("eps"))
        self._check(rc, "meshenv_policy_forward")
        return out

    # ---------------------------------------------------------------- public
    def forward(self, obs, noise=None, deterministic: bool = False):
        """obs float32 CUDA [n, 18]; noise float32 CUDA [n, 3] of N(0, 1) draws, or None / deterministic=True for eps = 0
        (the mean action).  Returns {actions, buffer_actions[, log_prob, value]}."""
        t = self._torch
        obs = self._obs(obs)
        if deterministic:
            noise = None
        if noise is not None:
            noise = noise.to(device=self.device, dtype=t.float32).contiguous()
            if tuple(noise.shape) != (obs.shape[0], 3):
                raise ValueError(f"noise must have shape ({obs.shape[0]}, 3), got {tuple(noise.shape)}")
        return self._launch(obs, noise, False, 0, 0, self._outputs(obs.shape[0], False))

    def sample(self, obs, seed: int, counter: int):
        """Stochastic outputs with eps drawn in the kernel (Philox4x32-10 keyed by seed, counter (env, counter): pass a fresh
        counter every rollout step).  The dict also holds eps: forward(obs, eps) reproduces the outputs bit for bit."""
        obs = self._obs(obs)
        return self._launch(obs, None, True, seed, counter, self._outputs(obs.shape[0], True))

    def value(self, obs):
        """V(obs) by the vf tower alone (actor-critic kind).  float32 CUDA [n]."""
        if self.spec.kind != KIND_ACTOR_CRITIC:
            raise ValueError("the deterministic kind has no value head")
        obs = self._obs(obs)
        out = dict(value=self._torch.empty(obs.shape[0], dtype=self._torch.float32, device=self.device))
        return self._launch(obs, None, False, 0, 0, out)["value"]
