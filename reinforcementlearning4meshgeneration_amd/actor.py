"""Fused SAC actor forward on the GPU (include/meshenv.h: meshenv_actor_*): the policy side of the rollout loop,
so that observation -> action -> step is two kernel launches with nothing leaving HBM.

Architecture = the reference's policy (rl/baselines/RL_Mesh.py:183-196: SB3 SAC, MlpPolicy, ReLU, [128, 128, 128]).
``FusedActor.from_torch(trunk, mu, log_std)`` takes the five ``torch.nn.Linear`` modules of an SB3 actor
(``actor.latent_pi`` layers 0/2/4, ``actor.mu``, ``actor.log_std``)."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi, sb3_nets
from ._handle import Handle
from .vec_env import ACTION_HIGH, ACTION_LOW


class FusedActor(Handle):
    PREFIX = "meshenv_actor"
    LAST_ERROR = "meshenv_last_error"
    HAS_LAST_ERROR = False

    def __init__(self, device: int = 0):
        super().__init__(device)

    @classmethod
    def from_torch(cls, linears, mu, log_std, device: int = 0, low=ACTION_LOW, high=ACTION_HIGH):
        """linears: the three hidden torch.nn.Linear layers (18->128, 128->128, 128->128)."""
        self = cls(device)
        arrs = []
        for lin in list(linears) + [mu, log_std]:
            arrs.append(np.ascontiguousarray(lin.weight.detach().cpu().numpy(), np.float32))
            arrs.append(np.ascontiguousarray(lin.bias.detach().cpu().numpy(), np.float32))
        shapes = [a.shape for a in arrs]
        assert shapes == [(128, 18), (128,), (128, 128), (128,), (128, 128), (128,), (3, 128), (3,), (3, 128), (3,)], shapes
        arrs += [np.ascontiguousarray(low, np.float32), np.ascontiguousarray(high, np.float32)]
        self._check(self._L.meshenv_actor_load(self._h, *[a.ctypes.data for a in arrs]), "meshenv_actor_load")
        return self

    @classmethod
    def from_sb3(cls, policy, device: int = 0, low=ACTION_LOW, high=ACTION_HIGH):
        """An SB3 2.x SAC model, SACPolicy or Actor (duck-typed, SB3 is not imported): the modules INTEGRATION.md section 3
        passes to from_torch by hand -- actor.latent_pi[0, 2, 4] (Linear, ReLU x 3, net_arch [128, 128, 128]), actor.mu,
        actor.log_std.  gSDE actors and other architectures are refused."""
        actor = policy
        if not hasattr(actor, "latent_pi"):
            if not hasattr(actor, "actor") and hasattr(actor, "policy"):
                actor = actor.policy
            actor = getattr(actor, "actor", actor)
        if not hasattr(actor, "latent_pi") or not hasattr(actor, "mu") or not hasattr(actor, "log_std"):
            raise ValueError("not an SB3 SAC actor (latent_pi, mu, log_std)")
        linears = sb3_nets.sac_actor(actor)
        if len(linears) != 3:
            raise ValueError(f"actor.latent_pi has {len(linears)} Linear layers; the fused actor is MlpPolicy's ReLU [128, 128, 128] "
                             "(rl/baselines/RL_Mesh.py:183-196)")
        return cls.from_torch(linears, actor.mu, actor.log_std, device=device, low=low, high=high)

    # ---------------------------------------------------------------- live parameters
    @staticmethod
    def live_params(policy):
        """The ten LIVE tensors of an SB3 SAC model, SACPolicy or Actor in bind order (w1 b1 w2 b2 w3 b3 mu_w mu_b log_std_w
        log_std_b), with the refusals of ``sb3_nets.sac_actor`` / ``sac_actor_params``.  No device is needed."""
        actor = policy
        if not hasattr(actor, "latent_pi"):
            if not hasattr(actor, "actor") and hasattr(actor, "policy"):
                actor = actor.policy
            actor = getattr(actor, "actor", actor)
        if not hasattr(actor, "latent_pi") or not hasattr(actor, "mu") or not hasattr(actor, "log_std"):
            raise ValueError("not an SB3 SAC actor (latent_pi, mu, log_std)")
        return sb3_nets.sac_actor_params(sb3_nets.sac_actor(actor), actor.mu, actor.log_std)

    def _check_live(self, rc, what):
        if rc != 0:
            msg = self._L.meshenv_actor_last_error(self._h)
            raise _capi.MeshEnvError(f"{what} failed (code {rc}): {msg.decode() if msg else ''}")

    def bind_live(self, policy) -> None:
        """Record the LIVE parameters of ``policy`` (an SB3 SAC model, SACPolicy or Actor) so that refresh() can carry them
        into this object's packed weights: what SB3 does implicitly when collect_rollouts reads the parameters
        ``actor.optimizer.step()`` has just written.  The object must have been loaded (from_torch / from_sb3 lay the packed
        buffer out) and the tensors must be on this device.  Again after anything that reallocates the parameters."""
        params = self.live_params(policy)
        sb3_nets.check_device(params, self.device, "FusedActor.bind_live")
        self._check_live(self._L.meshenv_actor_bind(self._h, self._ptrs(params), len(params)), "meshenv_actor_bind")
        self._live = params      # keeps the storages alive

    def refresh(self) -> None:
        """The bound parameters, as they are now, into the packed weights: one launch on the current stream, no host copy, no
        synchronisation.  Launches that follow on the same stream see the new weights."""
        if getattr(self, "_live", None) is None:
            raise ValueError("refresh() needs bind_live(model) first")
        self._bind_stream()
        self._check_live(self._L.meshenv_actor_refresh(self._h), "meshenv_actor_refresh")

    def forward(self, obs, noise=None, out=None):
        """obs: float32 CUDA [n, 18]; noise: float32 CUDA [n, 3] of N(0,1) samples or None (deterministic).
        Returns actions float32 CUDA [n, 3] inside the action Box."""
        t = self._torch
        n = obs.shape[0]
        if out is None:
            out = t.empty((n, 3), dtype=t.float32, device=self.device)
        self._bind_stream()
        rc = self._L.meshenv_actor_forward(self._h, n, obs.data_ptr(), noise.data_ptr() if noise is not None else None,
                                           out.data_ptr())
        self._check(rc, "meshenv_actor_forward")
        return out

    def sample(self, obs, seed: int, counter: int, out=None, eps_out=None):
        """Stochastic action with the N(0,1) exploration noise drawn inside the kernel (Philox4x32-10 keyed by `seed`,
        counter (env, `counter`)): pass a fresh `counter` every rollout step.  eps_out (float32 CUDA [n,3], optional)
        receives the noise used, so that forward(obs, eps_out) reproduces the actions exactly."""
        t = self._torch
        n = obs.shape[0]
        if out is None:
            out = t.empty((n, 3), dtype=t.float32, device=self.device)
        self._bind_stream()
        rc = self._L.meshenv_actor_sample(self._h, n, obs.data_ptr(), C.c_uint64(seed & (2 ** 64 - 1)),
                                          C.c_uint64(counter & (2 ** 64 - 1)), out.data_ptr(),
                                          eps_out.data_ptr() if eps_out is not None else None)
        self._check(rc, "meshenv_actor_sample")
        return out
