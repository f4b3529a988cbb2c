"""Policy evaluation on the device: SB3 2.x's ``evaluate_policy`` for the fused policies and ``MeshVecEnv.evaluate``'s
result type.

The reference evaluates in three places, each stepping a policy deterministically until every episode ends and reading
the return, the length, ``info['is_complete']``, ``len(env.generated_meshes)`` and the elements' quality:

* ``rl/baselines/CustomizeCallback.py:27-141`` every 1000 training steps, to pick ``best_model``;
* ``rl/baselines/testbed.py:150-212`` per domain, with the mean / std of ``get_quality(e, 4)``;
* ``v2/src/mesh_rl/evaluation/eval_loop.py:80-103``, which writes ``{"completed": [...], "n_elements": [...]}``.

``MeshVecEnv.evaluate(policy, ...)`` runs that loop in one C call (``meshenv_evaluate``: policy, step and a ``k_eval_tally``
launch per vector step, csrc/meshenv_eval.h) and returns an ``EvalResult``; ``evaluate_policy(model, env, ...)`` is SB3's
function on top of it.  Nothing here needs a GPU except the calls that run one."""
from __future__ import annotations

import warnings
from dataclasses import dataclass
from typing import Optional

import numpy as np

QUALITY_MEASURES = ("min_angle_deg", "max_angle_deg", "scaled_jacobian", "stretch", "taper", "robust", "area", "default")
FLAG_COMPLETE, FLAG_OVERFLOW = 1, 2
# the 16 words of a topology report (include/meshenv_topology.h)
TOPOLOGY_FIELDS = ("status", "n_elements", "n_vertices", "singularity", "valence_1", "valence_2", "valence_3", "valence_4",
                   "valence_5", "valence_6", "valence_7", "valence_8_or_more", "n_edges", "boundary_edges", "nonmanifold_edges",
                   "front_edges")


def topology_report(reports) -> dict:
    """The topology column of the reference's results table (general/post_processing.py:93-161: Singularity, num_vertices,
    num_elements per mesh) over a batch of reports [n, 16] (MeshVecEnv.mesh_topology, EvalResult.topology).

    Counted: the rows with status 0 and n_elements > 0.  meshes, elements, vertices (sums); singularity = dict(average, std,
    min, max, total) over the meshes (std: numpy's population value); singular_fraction = total singular / total vertices;
    valence_histogram = the summed bins (1 .. 7, >= 8 elements per vertex); closed = meshes with front_edges == 0;
    nonmanifold = meshes with nonmanifold_edges > 0; euler = [V - E + F per mesh]; skipped = {status: rows} of the rows with
    a status other than 0."""
    r = np.asarray(reports, dtype=np.int64).reshape(-1, len(TOPOLOGY_FIELDS))
    live = (r[:, 0] == 0) & (r[:, 1] > 0)
    m = r[live]
    sing = m[:, 3]
    have = len(m) > 0
    verts = int(m[:, 2].sum())
    bad, counts = np.unique(r[r[:, 0] != 0, 0], return_counts=True)
    return {"meshes": int(live.sum()), "elements": int(m[:, 1].sum()), "vertices": verts,
            "singularity": dict(average=float(sing.mean()) if have else float("nan"),
                                std=float(sing.std()) if have else float("nan"),
                                min=int(sing.min()) if have else 0, max=int(sing.max()) if have else 0, total=int(sing.sum())),
            "singular_fraction": float(sing.sum()) / verts if verts else float("nan"),
            "valence_histogram": [int(x) for x in m[:, 4:12].sum(axis=0)],
            "closed": int((m[:, 15] == 0).sum()), "nonmanifold": int((m[:, 14] > 0).sum()),
            "euler": [int(x) for x in m[:, 2] - m[:, 12] + m[:, 1]],
            "skipped": {int(k): int(c) for k, c in zip(bad, counts)}}


def episode_targets(n_envs: int, n_eval_episodes: Optional[int] = None, episodes_per_env=None) -> np.ndarray:
    """Episodes to record per env, int32 [n_envs]: SB3's ``(n_eval_episodes + i) // n_envs`` (evaluate_policy), an explicit
    int or [n_envs] array, or one episode per env when neither is given."""
    if n_eval_episodes is not None and episodes_per_env is not None:
        raise ValueError("give n_eval_episodes or episodes_per_env, not both")
    if episodes_per_env is None:
        if n_eval_episodes is None:
            return np.ones(n_envs, np.int32)
        if isinstance(n_eval_episodes, bool) or int(n_eval_episodes) != n_eval_episodes or n_eval_episodes < 0:
            raise ValueError(f"n_eval_episodes must be a non-negative integer, got {n_eval_episodes!r}")
        return np.array([(int(n_eval_episodes) + i) // n_envs for i in range(n_envs)], np.int32)
    t = np.asarray(episodes_per_env)
    if t.ndim == 0:
        t = np.full(n_envs, t)
    if t.shape != (n_envs,) or not np.issubdtype(t.dtype, np.integer) or (t < 0).any() or (t > 2 ** 24).any():
        raise ValueError(f"episodes_per_env must be a non-negative integer or an integer array of shape ({n_envs},), "
                         f"got {episodes_per_env!r}")
    if int(t.sum()) >= 2 ** 31:
        raise ValueError("too many episodes in one evaluation")
    return t.astype(np.int32)


@dataclass
class EvalResult:
    """The recorded episodes, sorted by (step, env): the order of SB3's ``episode_rewards`` / ``episode_lengths``.

    env, domain, step (0-based vector step at which the episode ended), length; reward = SB3's return (float64 sum of the
    float32 rewards), reward_raw = float64 sum of the float64 rewards; complete, overflow (the element log outgrew
    log_capacity); n_elements (0: the episode ended without an element; -1: no element log); archive = the
    ``get_last_episode(env)["episodes"]`` value of the finished mesh (0: none); quality [N, 8, 4] min / mean / max / variance
    of the QUALITY_MEASURES (None when not requested).  steps = vector steps run; finished = every env reached its target.
    topology [N, 16] int32: the TOPOLOGY_FIELDS of each finished mesh, scored at the tally like quality (None when not
    requested; 16 zeros for an episode without elements)."""
    env: np.ndarray
    domain: np.ndarray
    step: np.ndarray
    length: np.ndarray
    reward: np.ndarray
    reward_raw: np.ndarray
    complete: np.ndarray
    overflow: np.ndarray
    n_elements: np.ndarray
    archive: np.ndarray
    quality: Optional[np.ndarray]
    targets: np.ndarray
    steps: int
    finished: bool
    topology: Optional[np.ndarray] = None

    @classmethod
    def from_records(cls, rec: dict, targets, steps: int, finished: bool) -> "EvalResult":
        """rec: per-episode arrays in any order (keys env, domain, step, length, return, return_raw, flags, n_elements and
        optionally archive, quality, topology); sorted here by (step, env)."""
        order = np.lexsort((np.asarray(rec["env"]), np.asarray(rec["step"])))
        take = lambda k, dt: np.asarray(rec[k])[order].astype(dt)   # noqa: E731
        flags = take("flags", np.int32)
        n = len(order)
        q = rec.get("quality")
        tp = rec.get("topology")
        return cls(env=take("env", np.int32), domain=take("domain", np.int32), step=take("step", np.int64),
                   length=take("length", np.int64), reward=take("return", np.float64),
                   reward_raw=take("return_raw", np.float64), complete=(flags & FLAG_COMPLETE) != 0,
                   overflow=(flags & FLAG_OVERFLOW) != 0, n_elements=take("n_elements", np.int32),
                   archive=take("archive", np.int32) if rec.get("archive") is not None else np.zeros(n, np.int32),
                   quality=None if q is None else np.asarray(q, np.float64).reshape(-1, 8, 4)[order],
                   targets=np.asarray(targets, np.int32), steps=int(steps), finished=bool(finished),
                   topology=None if tp is None else np.asarray(tp, np.int32).reshape(-1, len(TOPOLOGY_FIELDS))[order])

    def __len__(self):
        return len(self.env)

    @property
    def episode_rewards(self) -> list:
        return [float(r) for r in self.reward]

    @property
    def episode_lengths(self) -> list:
        return [int(x) for x in self.length]

    @property
    def mean_reward(self) -> float:
        return float(np.mean(self.reward)) if len(self) else float("nan")

    @property
    def std_reward(self) -> float:
        return float(np.std(self.reward)) if len(self) else float("nan")

    def summary(self, by: Optional[str] = "domain") -> dict:
        """eval_loop.py's ``{"completed": [...], "n_elements": [...]}`` (v2/src/mesh_rl/evaluation/eval_loop.py:80-103), in
        record order: one such dict per domain (by="domain"), per env (by="env"), or a single one (by=None)."""
        def one(sel):
            return {"completed": [int(c) for c in self.complete[sel]], "n_elements": [int(x) for x in self.n_elements[sel]]}
        if by is None:
            return one(slice(None))
        if by not in ("domain", "env"):
            raise ValueError(f"by must be 'domain', 'env' or None, got {by!r}")
        keys = self.domain if by == "domain" else self.env
        return {int(k): one(keys == k) for k in np.unique(keys)}

    def quality_report(self) -> dict:
        """Per measure: the mean over the scored meshes of (average, standard deviation) and the overall range -- the
        aggregation of MeshVecEnv.quality_report; episodes without elements are skipped."""
        if self.quality is None:
            raise ValueError("this evaluation ran with quality=False")
        live = self.n_elements > 0
        out = {"meshes": int(live.sum()), "elements": int(self.n_elements[live].sum())}
        for k, name in enumerate(QUALITY_MEASURES):
            if live.any():
                st = self.quality[live, k]
                out[name] = dict(average=float(st[:, 1].mean()), std=float(np.sqrt(np.abs(st[:, 3])).mean()),
                                 min=float(st[:, 0].min()), max=float(st[:, 2].max()))
        return out

    def topology_report(self) -> dict:
        """evaluation.topology_report over the recorded meshes: Singularity / vertices / elements as the reference tabulates
        them, the valence histogram, closed and non-manifold meshes; episodes without elements are skipped."""
        if self.topology is None:
            raise ValueError("this evaluation ran with topology=False")
        return topology_report(self.topology)


def as_fused(model, device: int = 0):
    """A FusedPolicy / FusedActor as it is; an SB3 model or policy converted: SAC (actor.latent_pi) through
    FusedActor.from_sb3, PPO / A2C / TD3 through FusedPolicy.from_sb3."""
    from .actor import FusedActor
    from .policy import FusedPolicy
    if isinstance(model, (FusedPolicy, FusedActor)):
        return model, False
    pol = model
    if not hasattr(pol, "actor") and not hasattr(pol, "mlp_extractor") and hasattr(pol, "policy"):
        pol = pol.policy
    if hasattr(pol, "actor") and hasattr(pol.actor, "latent_pi"):
        return FusedActor.from_sb3(pol, device=device), True
    return FusedPolicy.from_sb3(pol, device=device), True


def evaluate_policy(model, env, n_eval_episodes: int = 10, deterministic: bool = True, return_episode_rewards: bool = False,
                    reward_threshold: Optional[float] = None, warn: bool = True, callback=None, render: bool = False):
    """SB3 2.x's ``stable_baselines3.common.evaluation.evaluate_policy`` on a MeshVecEnv, run on the device.

    Same signature and return values: (mean_reward, std_reward), or (episode_rewards, episode_lengths) with
    return_episode_rewards, in SB3's order; the rewards are SB3's sums of the float32 rewards.  model: a FusedPolicy /
    FusedActor, or an SB3 model or policy (converted once per call).  Episodes are split over the envs as SB3 does:
    (n_eval_episodes + i) // n_envs for env i.  callback and render=True would need the host inside the loop and are
    refused; warn=False silences the warning of an evaluation that hit max_steps."""
    if callback is not None:
        raise ValueError("evaluate_policy: callback is not supported: the episodes run inside one device loop with no "
                         "host code per step (use MeshVecEnv.step_tensor for a host-side loop)")
    if render:
        raise ValueError("evaluate_policy: render=True is not supported: the episodes run inside one device loop")
    if not hasattr(env, "evaluate"):
        raise TypeError(f"env must be a MeshVecEnv / SB3MeshVecEnv, got {type(env).__name__}")
    fused, owned = as_fused(model, device=env.device.index or 0)
    try:
        with warnings.catch_warnings():
            if not warn:
                warnings.simplefilter("ignore", RuntimeWarning)
            res = env.evaluate(fused, n_eval_episodes=n_eval_episodes, deterministic=deterministic,
                               quality=env.log_capacity > 0)
    finally:
        if owned:
            fused.close()
    if reward_threshold is not None:
        assert res.mean_reward > reward_threshold, \
            f"Mean reward below threshold: {res.mean_reward:.2f} < {reward_threshold:.2f}"
    if return_episode_rewards:
        return res.episode_rewards, res.episode_lengths
    return res.mean_reward, res.std_reward
