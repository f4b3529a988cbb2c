"""GPU: ``FusedOffPolicyLearn.learn`` against a hand-written loop over the pieces that were public before it, on a deep-copied
twin model with its own env and replay buffer and the same seeds and counters.  The twin's behaviour actor is REBUILT THROUGH
THE HOST from the twin's parameters before every collect (the path ``bind_live`` + ``refresh()`` replaces), its warm-up
actions are the numpy restatement uploaded, stepped one ``step_tensor`` at a time, and its ``train()`` is the composition of
tests/offpolicy_train_ref.py.  Afterwards everything is EQUAL: parameters, Adam moments, steps, targets, ``_n_updates``,
``num_timesteps``, the replay store with ``pos`` / ``full``, the env's obs / done; the episode statistics equal the Monitor
restatement applied to the twin's histories.

n = 33, train_freq = 3, learning_starts = 50: the first collect is two warm-up steps and one policy step, and training starts
after it (99 > 50)."""
import numpy as np
import pytest

import offpolicy_learn_ref as LR
import offpolicy_train_ref as TR

pytestmark = pytest.mark.gpu

N, T, LS, GS, BATCH, SEED = 33, 3, 50, 2, 16, 6
SIGMA = np.array([0.1, 0.2, 0.05], np.float32)
LOW = np.array([-1.0, -1.5, 0.0], np.float32)
HIGH = np.array([1.0, 1.5, 1.5], np.float32)


def _env():
    from reinforcementlearning4meshgeneration_amd import MeshVecEnv, boundary
    return MeshVecEnv([boundary(0)], n_envs=N)


def _model(kind, **attrs):
    base = dict(learning_starts=LS, train_freq=T, gradient_steps=GS, batch_size=BATCH, buffer_size=64 * N, num_timesteps=0)
    base.update(attrs)
    if kind == "td3":
        base.setdefault("policy_delay", 2)
    return TR.model(kind, **base)


class Twin:
    """SB3's loop by hand over step_tensor / step_actor_T / collect_rollout / add_rollout / the train composition."""

    def __init__(self, model, kind):
        from reinforcementlearning4meshgeneration_amd import DeviceReplayBuffer
        self.m, self.kind = model, kind
        self.env = _env()
        self.buf = DeviceReplayBuffer(self.env, model.buffer_size)
        self.comp = TR.Composition(model, self.buf)
        self.monitor = LR.MonitorRef(N, 100)
        self.steps = self.draws = 0
        self.rebuilds = self.trains = self.uniform_calls = 0

    def close(self):
        self.comp.close()
        self.env.close()

    def _note(self, out):
        self.monitor.update(out["reward"].cpu().numpy(), out["done"].cpu().numpy(), out["complete"].cpu().numpy())

    def _warmup(self, W):
        import torch
        env = self.env
        a, b = LR.uniform_actions(SEED, self.steps, W, N, LOW, HIGH)
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
        self.buf.add_rollout(out)
        self._note(out)
        self.uniform_calls += 1

    def _behave(self, P, counter):
        from reinforcementlearning4meshgeneration_amd import FusedActor, FusedPolicy
        env = self.env
        self.rebuilds += 1
        if self.kind == "sac":
            actor = FusedActor.from_sb3(self.m)                          # through the host, every time
            try:
                obs0 = env.obs.clone()
                first = actor.sample(obs0, SEED, counter)
                out = env.step_actor_T(actor, first, P, seed=SEED, counter=counter + 1, want_terminal_obs=True)
                self.buf.add_rollout(out, obs0=obs0)
            finally:
                actor.close()
        else:
            policy = FusedPolicy.from_sb3(self.m, sigma=SIGMA)
            try:
                out = env.collect_rollout(policy, P, seed=SEED, counter=counter)
                self.buf.add_rollout(out)
            finally:
                policy.close()
        self._note(out)

    def learn(self, total_timesteps):
        m = self.m
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
            self.steps += T
            m.num_timesteps = nt
            m._current_progress_remaining = 1.0 - float(nt) / float(total)
            if nt > 0 and nt > m.learning_starts and m.gradient_steps != 0:
                K = m.gradient_steps if m.gradient_steps > 0 else T
                self.comp.train(K, seed=SEED, counter=self.draws)
                self.draws += K
                self.trains += 1


def _assert_equal(learn, twin, m, tw):
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


@pytest.mark.parametrize("kind", ["sac", "td3"])
def test_learn_equals_the_host_rebuilt_loop_and_a_second_learn_continues(kind):
    from reinforcementlearning4meshgeneration_amd import FusedOffPolicyLearn
    m = _model(kind)
    tw = TR.twin(m)
    env = _env()
    learn = FusedOffPolicyLearn.from_sb3(m, env, action_noise_sigma=SIGMA if kind == "td3" else None)
    twin = Twin(tw, kind)
    try:
        logs = learn.learn(3 * 99, seed=SEED)
        twin.learn(3 * 99)
        assert m.num_timesteps == 297 and logs.iterations == 3
        assert learn.collect_calls == {"uniform": 1, "behaviour": 3} and twin.uniform_calls == 1 and twin.rebuilds == 3
        assert learn.train.calls == 3 == twin.trains and m._n_updates == 3 * GS
        _assert_equal(learn, twin, m, tw)
        got = logs.read()
        assert got["time/total_timesteps"] == 297 and got["train/n_updates"] == 6 and got["episodes"] == twin.monitor.count
        assert np.isfinite(got["train/critic_loss"])
        want = twin.monitor.logs()
        for k in ("rollout/ep_rew_mean", "rollout/ep_len_mean"):
            assert (k in got) == (k in want) and got.get(k) == want.get(k)
        # a second learn() continues: num_timesteps, the counters and the replay position go on, nothing is drawn twice
        logs = learn.learn(99, seed=SEED)
        twin.learn(99)
        assert m.num_timesteps == 396 and logs.iterations == 1 and learn.steps == 4 * T and learn.train.counter == 4 * GS
        assert learn.collect_calls["uniform"] == 1                          # past learning_starts: no second warm-up
        assert learn.buffer.pos == 4 * T
        _assert_equal(learn, twin, m, tw)
    finally:
        learn.close()
        twin.close()
        env.close()


def test_learning_starts_zero_launches_no_warmup_and_minus_one_trains_T_steps():
    from reinforcementlearning4meshgeneration_amd import FusedOffPolicyLearn
    m = _model("sac", learning_starts=0, gradient_steps=-1)
    tw = TR.twin(m)
    env = _env()
    learn = FusedOffPolicyLearn.from_sb3(m, env)
    twin = Twin(tw, "sac")
    try:
        learn.learn(99, seed=SEED)
        twin.learn(99)
        assert learn.collect_calls == {"uniform": 0, "behaviour": 1} and twin.uniform_calls == 0
        assert m._n_updates == T == tw._n_updates
        _assert_equal(learn, twin, m, tw)
    finally:
        learn.close()
        twin.close()
        env.close()


def test_learning_starts_beyond_total_never_trains():
    import torch
    from reinforcementlearning4meshgeneration_amd import FusedOffPolicyLearn
    m = _model("td3", learning_starts=10_000)
    before = {k: v.detach().clone() for k, v in TR.state(m).items()}
    env = _env()
    learn = FusedOffPolicyLearn.from_sb3(m, env, action_noise_sigma=SIGMA)
    try:
        logs = learn.learn(2 * 99, seed=SEED)
        assert learn.train.calls == 0 and m._n_updates == 0 and m.num_timesteps == 198
        assert learn.collect_calls == {"uniform": 2, "behaviour": 0}
        after = TR.state(m)
        assert set(after) == set(before)
        assert all(torch.equal(after[k].detach().view(torch.int32), before[k].view(torch.int32)) for k in before)
        got = logs.read()
        assert "train/critic_loss" not in got and got["time/total_timesteps"] == 198
        assert learn.buffer.pos == 2 * T
    finally:
        learn.close()
        env.close()
