"""The hand-written twin loops the GPU tests of the two device learn loops compare ``learn()`` with for EQUAL BITS, shared by
tests/test_gpu_offpolicy_learn.py, tests/test_gpu_onpolicy_learn.py and their ``_range`` modules.  Both sides of every
comparison run the same kernels on the same inputs in the same order, so no tolerance appears anywhere.

OffPolicyTwin   SB3's OffPolicyAlgorithm.learn over step_tensor / step_actor_T / collect_rollout / add_rollout and the train
                composition of tests/offpolicy_train_ref.py.  It stays independent of ``FusedOffPolicyLearn`` where it matters:
                the warm-up actions are the numpy restatement ``offpolicy_learn_ref.uniform_actions`` uploaded and stepped one
                ``step_tensor`` at a time, the behaviour actor is REBUILT THROUGH THE HOST before every collect, the Monitor is
                ``offpolicy_learn_ref.MonitorRef`` applied to the histories.
OnPolicyTwin    the loop of examples/ppo_train.py by hand: collect_rollout -> EpisodeStats.update -> num_timesteps ->
                FusedOnPolicyTrain.train (the path with a read-back per train() when there is a ``target_kl``).
Learner         FusedOnPolicyLearn on a model, an env and (optionally) handles of the test's own.

The shapes (n_envs, train_freq / n_steps, buffer_size through the model, window, fail_limit) and the starting values of the
step and draw counters are parameters; the defaults are the shapes of the two first test modules."""
from dataclasses import dataclass

import numpy as np

import offpolicy_learn_ref as LR
import offpolicy_train_ref as TR
import on_policy_stubs as S
import onpolicy_train_ref as OTR

SIGMA = np.array([0.1, 0.2, 0.05], np.float32)               # TD3's NormalActionNoise(0, sigma)
LOW = np.array([-1.0, -1.5, 0.0], np.float32)
HIGH = np.array([1.0, 1.5, 1.5], np.float32)
_CACHE = {}


def bits(x):
    import torch
    return x.contiguous().view(torch.int64 if x.dtype == torch.float64 else torch.int32 if x.dtype == torch.float32 else x.dtype)


def make_env(n, fail_limit=100, reset=False):
    from reinforcementlearning4meshgeneration_amd import MeshVecEnv, boundary
    env = MeshVecEnv([boundary(0)], n_envs=n, fail_limit=fail_limit)
    if reset:
        env.reset()
    return env


# ------------------------------------------------------------------------------------------------------------ off-policy
def offpolicy_model(kind, n_envs, train_freq, **attrs):
    base = dict(learning_starts=50, train_freq=train_freq, gradient_steps=2, batch_size=16, buffer_size=64 * n_envs, num_timesteps=0)
    base.update(attrs)
    if kind == "td3":
        base.setdefault("policy_delay", 2)
    return TR.model(kind, **base)


class OffPolicyTwin:
    """SB3's loop by hand over step_tensor / step_actor_T / collect_rollout / add_rollout / the train composition.

    Kept per collect in ``collects``: its kind ("uniform" / "behaviour"), the counter of its first vector step, the replay
    position it was stored at, the rollout dict with ``obs_after`` [T, n, 18] (the env's observation after each step, post-reset
    where an episode ended) and the number of episodes that finished in it; per iteration ``positions`` (pos, full) after its
    collects.  With ``record`` also, from launches of their own that change no state: the behaviour noise ``eps`` [P, n, 3]
    (vector step j of the collect at ``counter + j``) and per train() call ``sampled`` = (pos, full, the row indices of
    ``sample(..., return_indices=True)`` at the (seed, counter) of each of its gradient steps)."""

    def __init__(self, model, kind, n_envs=33, train_freq=3, seed=6, window=100, fail_limit=100, steps=0, draws=0, record=False):
        from reinforcementlearning4meshgeneration_amd import DeviceReplayBuffer
        self.m, self.kind = model, kind
        self.n, self.T, self.seed, self.record = n_envs, train_freq, seed, record
        self.env = make_env(n_envs, fail_limit)
        self.buf = DeviceReplayBuffer(self.env, model.buffer_size)
        self.comp = TR.Composition(model, self.buf)
        self.monitor = LR.MonitorRef(n_envs, window)
        self.steps, self.draws = steps, draws
        self.rebuilds = self.trains = self.uniform_calls = 0
        self.collects, self.positions, self.sampled = [], [], []

    def close(self):
        self.comp.close()
        self.env.close()

    def episodes(self, kind):
        return sum(c["episodes"] for c in self.collects if c["kind"] == kind)

    def _note(self, out, kind, counter, pos, obs_after, eps=None):
        done = out["done"].cpu().numpy()
        self.monitor.update(out["reward"].cpu().numpy(), done, out["complete"].cpu().numpy())
        self.collects.append(dict(kind=kind, counter=counter, pos=pos, out=out, obs_after=obs_after, eps=eps, episodes=int(done.sum())))

    def _warmup(self, W):
        import torch
        env, n = self.env, self.n
        a, b = LR.uniform_actions(self.seed, self.steps, W, n, LOW, HIGH)
        actions, buffer_actions = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
        obs = [env.obs.clone()]
        hist = dict(reward=[], done=[], complete=[], terminal_obs=[])
        for t in range(W):
            o, r, d, c = env.step_tensor(actions[t])
            obs.append(o.clone())
            hist["reward"].append(r.clone()); hist["done"].append(d.clone()); hist["complete"].append(c.clone())
            hist["terminal_obs"].append(torch.where(d[:, None] != 0, env.terminal_obs, torch.zeros_like(env.terminal_obs)))
        out = {k: torch.stack(v) for k, v in hist.items()}
        out.update(obs=torch.stack(obs[:W]), obs_after=torch.stack(obs[1:]), actions=actions, buffer_actions=buffer_actions)
        pos = self.buf.pos
        self.buf.add_rollout(out)
        self._note(out, "uniform", self.steps, pos, out["obs_after"])
        self.uniform_calls += 1

    def _behave(self, P, counter):
        import torch

        from reinforcementlearning4meshgeneration_amd import FusedActor, FusedPolicy
        env, seed = self.env, self.seed
        self.rebuilds += 1
        pos, eps = self.buf.pos, None
        if self.kind == "sac":
            actor = FusedActor.from_sb3(self.m)                          # through the host, every time
            try:
                obs0 = env.obs.clone()
                first = actor.sample(obs0, seed, counter)
                if self.record:                                          # the same draws again, into buffers of their own
                    eps0 = torch.empty((self.n, 3), dtype=torch.float32, device=env.device)
                    actor.sample(obs0, seed, counter, out=torch.empty_like(eps0), eps_out=eps0)
                out = env.step_actor_T(actor, first, P, seed=seed, counter=counter + 1, want_terminal_obs=True, want_eps=self.record)
                self.buf.add_rollout(out, obs0=obs0)
                if self.record:
                    eps = torch.cat([eps0[None], out["eps"][:P - 1]])   # out["eps"][t] chose the action of step t + 1
            finally:
                actor.close()
            obs_after = out["obs"]
        else:
            policy = FusedPolicy.from_sb3(self.m, sigma=SIGMA)
            try:
                out = env.collect_rollout(policy, P, seed=seed, counter=counter)
                self.buf.add_rollout(out)
            finally:
                policy.close()
            eps = out["eps"]
            obs_after = torch.cat([out["obs"][1:], env.obs[None]])
        self._note(out, "behaviour", counter, pos, obs_after, eps)

    def _train(self, K):
        if self.record:
            rows = [self.buf.sample(self.m.batch_size, seed=self.seed, counter=self.draws + k, return_indices=True)[1] for k in range(K)]
            self.sampled.append((self.buf.pos, self.buf.full, rows))
        self.comp.train(K, seed=self.seed, counter=self.draws)
        self.draws += K
        self.trains += 1

    def learn(self, total_timesteps):
        m, T, N = self.m, self.T, self.n
        total = total_timesteps + m.num_timesteps
        while m.num_timesteps < total:
            flags = []
            nt = m.num_timesteps
            for _ in range(T):                                            # SB3 tests before each step's increment
                flags.append(nt < m.learning_starts)
                nt += N
            W = sum(flags)
            assert flags == [True] * W + [False] * (T - W)
            if W:
                self._warmup(W)
            if T - W:
                self._behave(T - W, self.steps + W)
            self.positions.append((self.buf.pos, self.buf.full))
            self.steps += T
            m.num_timesteps = nt
            m._current_progress_remaining = 1.0 - float(nt) / float(total)
            if nt > 0 and nt > m.learning_starts and m.gradient_steps != 0:
                self._train(m.gradient_steps if m.gradient_steps > 0 else T)


def assert_offpolicy_equal(learn, twin, m, tw):
    import torch
    assert TR.differing(m, tw) == []                                      # parameters, moments, steps, targets, _n_updates
    assert m.num_timesteps == tw.num_timesteps and m._current_progress_remaining == tw._current_progress_remaining
    a, b = learn.buffer, twin.buf
    assert (a.pos, a.full, a.size()) == (b.pos, b.full, b.size())
    assert torch.equal(a.store.view(torch.int32), b.store.view(torch.int32))
    assert torch.equal(learn.venv.obs.view(torch.int32), twin.env.obs.view(torch.int32))
    assert torch.equal(learn.venv.done, twin.env.done)
    stats, ref = learn.stats, twin.monitor
    assert int(stats.count.cpu().numpy().view(np.uint64)[0]) == ref.count
    assert np.array_equal(stats.ring.cpu().numpy().view(np.int64), ref.ring().view(np.int64))
    cr, cl = ref.carries()
    assert np.array_equal(stats.carry_return.cpu().numpy().view(np.int64), cr.view(np.int64))
    assert np.array_equal(stats.carry_len.cpu().numpy(), cl)


# ------------------------------------------------------------------------------------------------------------- on-policy
@dataclass(frozen=True)
class OnPolicyShape:
    """n envs x T steps per collect; PPO: ``batch`` rows per minibatch and ``epochs`` epochs (A2C: one minibatch of all rows)."""
    n: int = 11
    T: int = 3
    batch: int = 8
    epochs: int = 3
    seed: int = 5
    window: int = 100
    fail_limit: int = 100

    @property
    def rows(self):
        return self.n * self.T

    @property
    def K(self):
        """Minibatches of one PPO train()."""
        return self.epochs * -(-self.rows // self.batch)


DEFAULT_SHAPE = OnPolicyShape()


def onpolicy_model(kind, variant="plain", target_kl=None, shape=DEFAULT_SHAPE):
    model, params = S.model(kind, "cuda")
    model.n_steps, model.num_timesteps, model._n_updates = shape.T, 0, 0
    if kind == "ppo":
        model.n_epochs, model.batch_size, model.target_kl = shape.epochs, shape.batch, target_kl
        if variant == "scheduled":
            model.lr_schedule = lambda progress: 1.0e-4 + 4.0e-4 * progress
            model.clip_range = lambda progress: 0.1 + 0.1 * progress
    return model, params


def onpolicy_perms(kind, iterations, seed=3, shape=DEFAULT_SHAPE):
    import torch
    rng = np.random.default_rng(seed)
    n_epochs = shape.epochs if kind == "ppo" else 1
    return torch.from_numpy(np.stack([[rng.permutation(shape.rows) for _ in range(n_epochs)] for _ in range(iterations)]).astype(np.int64)).cuda()


def fixed_obs():
    import torch
    if "obs" not in _CACHE:
        rng = np.random.default_rng(17)
        _CACHE["obs"] = (torch.from_numpy(rng.uniform(-1, 1, (16, 18)).astype(np.float32)).cuda(),
                         torch.from_numpy(rng.standard_normal((16, 3)).astype(np.float32)).cuda())
    return _CACHE["obs"]


class OnPolicyTwin:
    """Side B: the loop of examples/ppo_train.py by hand, with EpisodeStats.update and SB3's bookkeeping.  ``keep``: the rollout
    dict of every collect stays in ``outs``, with the counter of its first vector step in ``counters``."""

    def __init__(self, kind, variant="plain", target_kl=None, shape=DEFAULT_SHAPE, steps=0, keep=False):
        from reinforcementlearning4meshgeneration_amd import EpisodeStats, FusedOnPolicyTrain, FusedPolicy
        self.kind, self.shape, self.keep = kind, shape, keep
        self.model, self.params = onpolicy_model(kind, variant, target_kl, shape)
        self.opt = self.model.policy.optimizer
        self.env = make_env(shape.n, shape.fail_limit, reset=True)
        self.fp = FusedPolicy.from_sb3(self.model)
        self.fp.bind_live(self.model)
        self.tr = FusedOnPolicyTrain.from_sb3(self.model, self.fp)
        self.stats = EpisodeStats(shape.n, shape.window)
        self.steps = steps
        self.rows, self.applied, self.kls = [], [], []
        self.outs, self.counters = [], []

    def close(self):
        for h in (self.tr, self.stats, self.fp, self.env):
            h.close()

    def loop(self, total_timesteps, perms, cb=None, record=False):
        from reinforcementlearning4meshgeneration_amd.onpolicy_train import update_learning_rate
        m, T, N, seed = self.model, self.shape.T, self.shape.n, self.shape.seed
        total = total_timesteps + m.num_timesteps
        i = 0
        while m.num_timesteps < total:
            if cb is not None:                           # SB3 would evaluate during the collect; the parameters change only in train()
                for j in range(1, T + 1):
                    cb.n_calls += 1
                    if cb.n_calls % cb.eval_freq == 0:
                        cb.evaluate_now(self.fp, m.num_timesteps + j * N)
            out = self.env.collect_rollout(self.fp, T, seed=seed, counter=self.steps, gamma=m.gamma, gae_lambda=m.gae_lambda)
            self.stats.update(out)
            if self.keep:
                self.outs.append(out)
                self.counters.append(self.steps)
            self.steps += T
            m.num_timesteps += T * N
            m._current_progress_remaining = 1.0 - float(m.num_timesteps) / float(total)
            if record:                                   # the composition: approx_kl per minibatch, read on the host
                update_learning_rate(m, self.opt)
                ref = OTR.compose(m, self.tr.pg, self.tr.fo, self.tr.rb, self.fp, out, perms[i])
                self.kls.append([float(r["approx_kl"]) for r in ref["records"]])
            else:
                logs = self.tr.train(out, perms[i])
                self.rows.append(logs.device.clone())
                if m.target_kl is not None:
                    self.applied.append(logs.values()["steps_applied"])
            i += 1


class Learner:
    """Side A: FusedOnPolicyLearn on a model, an env and (optionally) handles of the test's own."""

    def __init__(self, kind, variant="plain", target_kl=None, own_handles=False, shape=DEFAULT_SHAPE):
        from reinforcementlearning4meshgeneration_amd import FusedOnPolicyLearn, FusedOnPolicyTrain, FusedPolicy
        self.shape = shape
        self.model, self.params = onpolicy_model(kind, variant, target_kl, shape)
        self.opt = self.model.policy.optimizer
        self.env = make_env(shape.n, shape.fail_limit, reset=True)
        self.fp = self.tr = None
        if own_handles:
            self.fp = FusedPolicy.from_sb3(self.model)
            self.fp.bind_live(self.model)
            self.tr = FusedOnPolicyTrain.from_sb3(self.model, self.fp)
        self.learn = FusedOnPolicyLearn.from_sb3(self.model, self.env, policy=self.fp, train=self.tr, window=shape.window)
        self.stats = self.learn.stats

    def close(self):
        self.learn.close()
        for h in (self.tr, self.fp, self.env):
            if h is not None:
                h.close()


def assert_onpolicy_equal(a, b, what, rows=None, want=None):
    """All 13 parameters, every optimiser state tensor and step, the refreshed policy's forward, _n_updates, num_timesteps,
    the EpisodeStats state, the env, and (rows: A's history) every history row against B's per-iteration logs.device (want:
    those rows when B is a Learner too)."""
    import torch
    want = getattr(b, "rows", None) if want is None else want
    b_policy = b.learn.policy if isinstance(b, Learner) else b.fp
    for i, (p, q) in enumerate(zip(a.params, b.params)):
        assert torch.equal(bits(p.detach()), bits(q.detach())), (what, "parameter", i)
        sa, sb = a.opt.state[p], b.opt.state[q]
        assert set(sa) == set(sb) and len(sa) >= 2, (what, i)
        for k in sa:
            if k == "step":
                assert float(sa[k]) == float(sb[k]), (what, "step", i, float(sa[k]), float(sb[k]))
            else:
                assert torch.equal(bits(sa[k]), bits(sb[k])), (what, k, i)
    assert a.model._n_updates == b.model._n_updates, (what, a.model._n_updates, b.model._n_updates)
    assert a.model.num_timesteps == b.model.num_timesteps, what
    assert a.model._current_progress_remaining == b.model._current_progress_remaining, what
    obs, eps = fixed_obs()
    fa, fb = a.learn.policy.forward(obs, eps), b_policy.forward(obs, eps)
    for k in ("actions", "log_prob", "value"):
        assert torch.equal(bits(fa[k]), bits(fb[k])), (what, "refreshed policy", k)
    for name in ("state", "carry_return", "carry_len"):
        assert torch.equal(bits(getattr(a.stats, name)), bits(getattr(b.stats, name))), (what, "EpisodeStats", name)
    assert torch.equal(bits(a.env.obs), bits(b.env.obs)) and torch.equal(a.env.done, b.env.done), (what, "env")
    if rows is not None:
        assert tuple(rows.shape) == (len(want), 12) and rows.dtype == torch.float64, (what, tuple(rows.shape), len(want))
        for i, row in enumerate(want):
            assert torch.equal(bits(rows[i]), bits(row)), (what, "history row", i, rows[i].tolist(), row.tolist())


def onpolicy_target(variant, iterations, perms, shape=DEFAULT_SHAPE, key=None):
    """(target_kl, the recorded approx_kl per iteration and minibatch, i*) from the twin's side alone: the hand loop is run
    without a target_kl through tests/onpolicy_train_ref.compose, which records approx_kl per minibatch.  With M_i the largest
    approx_kl of iteration i, the limit 1.5 x target_kl is set just under M_i* for the first i* >= 1 whose M exceeds every
    earlier iteration's: iterations before i* then apply all K steps on the recorded trajectory, and iteration i* stops inside
    (minibatch 0 of a train() has an approx_kl of rounding size: the parameters are the rollout's).  Without such an i* the
    limit goes just under M_0.  ``key``: what the result is cached under (None: not cached)."""
    if key is None or key not in _CACHE:
        import torch
        rec = OnPolicyTwin("ppo", variant, shape=shape)
        rec.loop(iterations * shape.rows, perms, record=True)
        torch.cuda.synchronize()
        rec.close()
        kls = rec.kls
        assert len(kls) == iterations and all(len(k) == shape.K for k in kls), kls
        M = [max(k) for k in kls]
        star = next((i for i in range(1, iterations) if M[i] * (1 - 2.0 ** -10) > max(M[:i])), 0)
        target = M[star] * (1 - 2.0 ** -10) / 1.5
        assert target > 0.0 and all(x <= 1.5 * target for k in kls[:star] for x in k) and M[star] > 1.5 * target
        print(f"\n{variant}: max approx_kl per iteration {M}; i* = {star}; target_kl = {target!r}")
        if key is None:
            return target, kls, star
        _CACHE[key] = (target, kls, star)
    return _CACHE[key]
