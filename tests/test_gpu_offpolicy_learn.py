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

import learn_twins as LT
import offpolicy_train_ref as TR

pytestmark = pytest.mark.gpu

N, T, LS, GS, BATCH, SEED = 33, 3, 50, 2, 16, 6
SIGMA = LT.SIGMA


def _env():
    from reinforcementlearning4meshgeneration_amd import MeshVecEnv, boundary
    return MeshVecEnv([boundary(0)], n_envs=N)


def _model(kind, **attrs):
    base = dict(learning_starts=LS, train_freq=T, gradient_steps=GS, batch_size=BATCH, buffer_size=64 * N, num_timesteps=0)
    base.update(attrs)
    if kind == "td3":
        base.setdefault("policy_delay", 2)
    return TR.model(kind, **base)


class Twin(LT.OffPolicyTwin):
    """tests/learn_twins.py's hand loop at this module's shape."""

    def __init__(self, model, kind):
        super().__init__(model, kind, n_envs=N, train_freq=T, seed=SEED)


_assert_equal = LT.assert_offpolicy_equal


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
