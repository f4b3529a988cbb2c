"""TD targets of SAC and TD3 on the GPU (include/meshenv.h: meshenv_target_*, csrc/meshenv_target.h): the
``with th.no_grad():`` block of SB3 2.x's ``SAC.train`` / ``TD3.train`` that turns a sampled batch into ``target_q_values``,
one launch from the tensors ``DeviceReplayBuffer.sample`` returns.

Two kinds, the networks the reference trains (rl/baselines/RL_Mesh.py:179-222):

* SAC: actor ReLU [128, 128, 128] with ``mu`` / ``log_std`` heads, twin critics ReLU [128, 128, 128];
* TD3: ``actor_target`` ReLU [256, 256] + tanh, twin critics ReLU [256, 256].

The weights are the LIVE torch parameters on the device: ``FusedTDTarget`` records their pointers once and ``refresh()``
copies them into the kernel's layout in one launch on the current stream (no host copy, no synchronisation), so a training
loop calls ``refresh()`` after its optimiser / Polyak steps and ``target(...)`` after ``sample``.  ``TDTargetSpec`` is the
host half (kind, constants, the parameter tensors and every refusal; no device needed).  Layers are ``torch.nn.Linear``-like
objects (``.weight [out][in]``, ``.bias``)."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import List, Optional

from . import _capi
from .policy import _sequential

KIND_SAC, KIND_TD3 = 0, 1
OBS_DIM, ACT_DIM = _capi.OBS_DIM, _capi.ACT_DIM
Q_IN = OBS_DIM + ACT_DIM
HIDDEN = {KIND_SAC: (128, 3), KIND_TD3: (256, 2)}     # width, hidden layers
SUPPORTED = ("SAC: ReLU [128, 128, 128] actor (mu and log_std heads) with twin ReLU [128, 128, 128] critics; "
             "TD3: ReLU [256, 256] tanh actor with twin ReLU [256, 256] critics; 18 observations, 3 actions, "
             "critic input cat(obs, action) = 21")


def _param(x, what, shape):
    """A live parameter: float32, contiguous, of the expected shape (a torch tensor: its storage is what gets bound)."""
    if not hasattr(x, "data_ptr") or not hasattr(x, "is_contiguous"):
        raise ValueError(f"{what} is {type(x).__name__}, not a torch tensor")
    if str(x.dtype) != "torch.float32":
        raise ValueError(f"{what} has dtype {x.dtype}; parameters must be float32")
    if tuple(x.shape) != tuple(shape):
        raise ValueError(f"{what} has shape {tuple(x.shape)}, expected {tuple(shape)}; supported: {SUPPORTED}")
    if not x.is_contiguous():
        raise ValueError(f"{what} is not contiguous")
    return x


def _mlp(layers, head_layers, n_in, kind, what):
    """[w1, b1, ..., head_w, head_b, ...] of an MLP of the kind's width and depth; each head has (n_out, layer)."""
    H, NL = HIDDEN[kind]
    layers = list(layers)
    widths = [tuple(getattr(l.weight, "shape", ())) for l in layers]
    if len(layers) != NL or any(w[:1] != (H,) for w in widths):
        raise ValueError(f"{what}: hidden layers {[w[0] if w else None for w in widths]}; supported: {SUPPORTED}")
    out, k = [], n_in
    for i, l in enumerate(layers):
        out += [_param(l.weight, f"{what}[{i}].weight", (H, k)), _param(l.bias, f"{what}[{i}].bias", (H,))]
        k = H
    for name, n_out, l in head_layers:
        out += [_param(l.weight, f"{what} {name}.weight", (n_out, H)), _param(l.bias, f"{what} {name}.bias", (n_out,))]
    return out


def _critic(q, kind, what):
    """A q_network: an nn.Sequential(Linear, ReLU, ..., Linear) or a list of its Linear layers."""
    linears, acts = _sequential(q)
    if acts - {"relu"}:
        raise ValueError(f"{what}: activations {sorted(acts)}; supported: {SUPPORTED}")
    if len(linears) < 2:
        raise ValueError(f"{what}: {len(linears)} Linear layers; supported: {SUPPORTED}")
    return _mlp(linears[:-1], [("output", 1, linears[-1])], Q_IN, kind, what)


def _flatten_only(owner, what, shared=False):
    fe = getattr(owner, "features_extractor", None)
    if fe is not None and type(fe).__name__ != "FlattenExtractor":
        how = " (share_features_extractor=True)" if shared else ""
        raise ValueError(f"{what}.features_extractor{how} is {type(fe).__name__}; only the MLP policies' FlattenExtractor is "
                         "supported")


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
        return "sac" if self.kind == KIND_SAC else "td3"

    @property
    def hidden(self) -> int:
        return HIDDEN[self.kind][0]

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
        if (log_ent_coef is None) == (ent_coef is None):
            raise ValueError("SAC needs exactly one of log_ent_coef (the learned tensor) and ent_coef (a fixed float)")
        actor = _mlp(actor_layers, [("mu", ACT_DIM, mu), ("log_std", ACT_DIM, log_std)], OBS_DIM, KIND_SAC, "actor")
        spec = cls(KIND_SAC, cls._gamma(gamma), actor, _critic(q1, KIND_SAC, "q_networks[0]"), _critic(q2, KIND_SAC, "q_networks[1]"))
        if log_ent_coef is not None:
            if not hasattr(log_ent_coef, "numel") or log_ent_coef.numel() != 1:
                raise ValueError(f"log_ent_coef must be a tensor of one element, got {log_ent_coef!r}")
            spec.log_ent_coef = _param(log_ent_coef, "log_ent_coef", tuple(log_ent_coef.shape))
        else:
            spec.ent_coef = float(ent_coef)
            if not spec.ent_coef == spec.ent_coef or abs(spec.ent_coef) == float("inf"):
                raise ValueError(f"ent_coef must be finite, got {ent_coef!r}")
        return spec

    @classmethod
    def td3(cls, actor_layers, mu, q1, q2, gamma, policy_noise=0.2, noise_clip=0.5) -> "TDTargetSpec":
        pn, nc = float(policy_noise), float(noise_clip)
        if not (0.0 <= pn < float("inf")) or not (0.0 <= nc < float("inf")):
            raise ValueError(f"policy_noise and noise_clip must be finite and >= 0, got {policy_noise!r}, {noise_clip!r}")
        actor = _mlp(actor_layers, [("mu", ACT_DIM, mu)], OBS_DIM, KIND_TD3, "actor")
        return cls(KIND_TD3, cls._gamma(gamma), actor, _critic(q1, KIND_TD3, "q_networks[0]"), _critic(q2, KIND_TD3, "q_networks[1]"),
                   policy_noise=pn, noise_clip=nc)

    @classmethod
    def from_sb3(cls, model) -> "TDTargetSpec":
        """Duck-typed on SB3 2.x's SAC (``actor.latent_pi / .mu / .log_std``, ``critic_target.q_networks``, ``gamma``,
        ``log_ent_coef`` or ``ent_coef_tensor``) and TD3 (``actor_target.mu``, ``critic_target.q_networks``, ``gamma``,
        ``target_policy_noise``, ``target_noise_clip``)."""
        critic = getattr(model, "critic_target", None)
        if critic is None or not hasattr(critic, "q_networks"):
            raise ValueError(f"{type(model).__name__} has no critic_target.q_networks: not an SB3 SAC or TD3 model")
        qs = list(critic.q_networks)
        n_critics = int(getattr(critic, "n_critics", len(qs)))
        is_sac = hasattr(getattr(model, "actor", None), "latent_pi")
        is_td3 = not is_sac and hasattr(getattr(model, "actor_target", None), "mu")
        if not is_sac and not is_td3:
            raise ValueError(f"{type(model).__name__} has neither SAC's actor.latent_pi nor TD3's actor_target.mu")
        if n_critics != 2 or len(qs) != 2:
            ddpg = " (DDPG: one critic, no twin minimum)" if is_td3 and n_critics == 1 else ""
            raise ValueError(f"n_critics = {n_critics}{ddpg}; the twin critics of SAC / TD3 (n_critics = 2) are supported")
        _flatten_only(critic, "critic_target", shared=bool(getattr(critic, "share_features_extractor", False)))
        if is_sac:
            actor = model.actor
            _flatten_only(actor, "actor")
            if getattr(actor, "use_sde", False):
                raise ValueError("use_sde=True (gSDE actor) is not supported; " + SUPPORTED)
            linears, acts = _sequential(actor.latent_pi)
            if acts - {"relu"}:
                raise ValueError(f"actor.latent_pi: activations {sorted(acts)}; supported: {SUPPORTED}")
            if type(actor.log_std).__name__ != "Linear":
                raise ValueError(f"actor.log_std is {type(actor.log_std).__name__}, not a Linear head (gSDE?); " + SUPPORTED)
            lec = getattr(model, "log_ent_coef", None)
            if lec is not None:
                return cls.sac(linears, actor.mu, actor.log_std, qs[0], qs[1], model.gamma, log_ent_coef=lec)
            fixed = getattr(model, "ent_coef_tensor", None)
            if fixed is None:
                raise ValueError("the SAC model has neither log_ent_coef nor ent_coef_tensor")
            return cls.sac(linears, actor.mu, actor.log_std, qs[0], qs[1], model.gamma, ent_coef=float(fixed))
        actor = model.actor_target
        _flatten_only(actor, "actor_target")
        mods = list(actor.mu)
        if not mods or type(mods[-1]).__name__ != "Tanh":
            raise ValueError("actor_target.mu must end in Tanh (SB3's TD3 actor); " + SUPPORTED)
        linears, acts = _sequential(mods[:-1])
        if acts - {"relu"}:
            raise ValueError(f"actor_target.mu: activations {sorted(acts)}; supported: {SUPPORTED}")
        if len(linears) < 2:
            raise ValueError(f"actor_target.mu: {len(linears)} Linear layers; supported: {SUPPORTED}")
        return cls.td3(linears[:-1], linears[-1], qs[0], qs[1], model.gamma, model.target_policy_noise, model.target_noise_clip)

    def check_device(self, device) -> None:
        """Every bound tensor lives on `device` (a torch.device): the kernel reads them through raw pointers."""
        for x in self.tensors():
            if x.device != device:
                raise ValueError(f"a parameter of shape {tuple(x.shape)} is on {x.device}; FusedTDTarget binds float32 "
                                 f"contiguous CUDA tensors on {device}")


class FusedTDTarget:
    """A TDTargetSpec bound on one GPU.  target() returns target_q_values [B, 1] as a float32 CUDA tensor."""

    def __init__(self, spec: TDTargetSpec, device: int = 0):
        import torch
        self._torch = torch
        self._L = _capi.load()
        if not torch.cuda.is_available():
            raise _capi.MeshEnvError("FusedTDTarget needs a ROCm GPU")
        self.spec = spec
        self.device = torch.device("cuda", device)
        spec.check_device(self.device)
        self._h = C.c_void_p()
        stream = torch.cuda.current_stream(self.device).cuda_stream
        rc = self._L.meshenv_target_create(device, C.c_void_p(stream), spec.kind, spec.gamma, spec.ent_coef, spec.policy_noise,
                                           spec.noise_clip, C.byref(self._h))
        if rc != 0:
            raise _capi.MeshEnvError(f"meshenv_target_create failed ({rc}): {self._L.meshenv_target_last_error(None).decode()}")
        self._stream = stream
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
    def from_sb3(cls, model, device: int = 0):
        return cls(TDTargetSpec.from_sb3(model), device)

    # ---------------------------------------------------------------- plumbing
    def _check(self, rc, what):
        if rc != 0:
            msg = self._L.meshenv_target_last_error(self._h)
            raise _capi.MeshEnvError(f"{what} failed (code {rc}): {msg.decode() if msg else ''}")

    def _bind_stream(self):
        stream = self._torch.cuda.current_stream(self.device).cuda_stream
        if stream != self._stream:
            self._check(self._L.meshenv_target_set_stream(self._h, C.c_void_p(stream)), "meshenv_target_set_stream")
            self._stream = stream

    def bind(self) -> None:
        """Record the parameters' device pointers again: after anything that reallocates them (``.to()``; SB3's optimisers,
        ``polyak_update`` and ``load_state_dict`` write in place and need no new bind).  Follow with refresh()."""
        s = self.spec
        s.check_device(self.device)
        arr = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])   # noqa: E731
        lec = s.log_ent_coef.data_ptr() if s.log_ent_coef is not None else None
        rc = self._L.meshenv_target_bind(self._h, arr(s.actor), len(s.actor), arr(s.q1), arr(s.q2), len(s.q1), lec)
        self._check(rc, "meshenv_target_bind")

    def refresh(self) -> None:
        """Snapshot the live parameters (and log_ent_coef) into the kernel's layout: one launch on the current stream, no
        synchronisation.  target() uses the values of the last refresh."""
        self._bind_stream()
        self._check(self._L.meshenv_target_refresh(self._h), "meshenv_target_refresh")

    def _f32(self, x, name, shape):
        t = self._torch
        if x.dtype != t.float32 or not x.is_contiguous() or x.device != self.device:
            x = x.to(device=self.device, dtype=t.float32).contiguous()
        if tuple(x.shape) not in shape:
            raise ValueError(f"{name} must have shape {' or '.join(str(s) for s in shape)}, got {tuple(x.shape)}")
        return x

    # ---------------------------------------------------------------- public
    def target(self, samples=None, *, next_observations=None, rewards=None, dones=None, noise=None, seed=None,
               counter: int = 0, return_parts: bool = False):
        """target_q_values [B, 1] of a batch: ``samples`` (a ReplayBufferSamples: next_observations, rewards, dones are
        read) or the three tensors by keyword.  eps is ``noise`` ([B, 3] of N(0, 1) draws), drawn in the kernel when ``seed``
        is given (Philox4x32-10 at (seed, counter, sample index), a stream of its own: pass a fresh counter every batch), or
        0 with neither.  return_parts: also a dict of next_actions [B, 3] (in [-1, 1]), next_log_prob [B] (SAC), q1, q2 [B]
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
            parts = dict(next_actions=t.empty((B, ACT_DIM), **f32), q1=t.empty(B, **f32), q2=t.empty(B, **f32))
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

    def close(self):
        if self._h:
            self._L.meshenv_target_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
