"""GPU: ``FusedOnPolicyLearn.learn`` against the hand loop of tests/learn_twins.py (collect_rollout -> EpisodeStats.update ->
num_timesteps -> FusedOnPolicyTrain.train) for EQUAL BITS, at the shapes the first module (tests/test_gpu_onpolicy_learn.py:
11 envs x 3 steps, no episode needs to end) leaves out: 1025 envs x 2 steps (more envs than one workgroup of k_episode_stats,
2050 rows: more than 1024 per train(), PPO's last minibatch of 2 rows) without and with a ``target_kl``, episodes that end
and feed the ``terminal_value`` bootstrap into GAE, and a noise counter that carries into its high word inside a collect under
a seed whose high word is set.

The models are tests/on_policy_stubs.py's.  Both sides run the same kernels on the same inputs in the same order; the two
independent restatements used on top are tests/gae_ref.py (numpy float32, equal bits) and ``policy_ref.philox_normal`` (fp64,
``policy_ref.assert_within``'s bound).  Every test prints what keeps it from passing on empty data."""
import numpy as np
import pytest

import gae_ref
import learn_twins as LT
import offpolicy_learn_ref as LR
import on_policy_stubs as S
import policy_ref as R

pytestmark = pytest.mark.gpu

WIDE_SEED = (0x5EED << 32) | 77                              # both words of the key are non-zero
WIDE = LT.OnPolicyShape(n=1025, T=2, batch=512, epochs=2, fail_limit=2)     # PPO: 5 minibatches per epoch, the last of 2 rows
ENDING = LT.OnPolicyShape(n=33, T=3, window=4, fail_limit=3)
CARRY = LT.OnPolicyShape(n=33, T=3, seed=WIDE_SEED)


def _episodes(twin, first_env=0):
    """Episodes finished per collect of the twin's kept rollouts, in the envs from ``first_env`` on."""
    return [int(out["done"][:, first_env:].sum()) for out in twin.outs]


def _count(stats):
    return int(stats.count.cpu()[0])


# ------------------------------------------------------------------------------------------------- 8. past one workgroup
@pytest.mark.parametrize("kind", ["ppo", "a2c"])
def test_1025_envs_and_2050_rows_have_the_hand_loops_bits(kind):
    """Two iterations of 1025 envs x 2 steps.  PPO: batch_size 512 (minibatches of 512, 512, 512, 512 and 2 rows), 2 epochs, no
    target_kl; A2C: its one minibatch of all 2050 rows.  fail_limit = 2: under the initial policies (fp64 restatement, CPU
    oracle) env 1024 is refused at both steps of the first collect, so its episode ends at vector step 1."""
    import torch
    a, b = LT.Learner(kind, shape=WIDE), LT.OnPolicyTwin(kind, shape=WIDE, keep=True)
    perms = LT.onpolicy_perms(kind, 2, shape=WIDE)
    logs = a.learn.learn(2 * WIDE.rows, seed=WIDE.seed, perms=perms)
    b.loop(2 * WIDE.rows, perms)
    last = _episodes(b, 1024)
    print(f"\n{kind}: episodes finished per collect {_episodes(b)}, in env 1024 {last}")
    assert sum(last) >= 1 and _count(b.stats) == sum(_episodes(b)) > 100           # the ring of 100 wraps, too
    assert a.model.num_timesteps == 2 * WIDE.rows and logs.iterations == 2 and a.learn.readbacks == 0 and a.learn.steps == 4
    LT.assert_onpolicy_equal(a, b, f"{kind} 1025 envs", logs.device)
    per_train = WIDE.K if kind == "ppo" else 1
    assert all(float(a.opt.state[p]["step"]) == float(2 * per_train) for p in a.params)
    assert a.model._n_updates == 2 * (WIDE.epochs if kind == "ppo" else 1)
    assert not any(torch.equal(p, q) for p, q in zip(a.params, S.policy(kind, "cuda")[1]))      # it did train
    assert logs.read()["episodes"] == _count(b.stats)
    a.close(); b.close()


# ------------------------------------------------------------------------------------------------- 9. the same with a target_kl
def test_1025_envs_with_a_target_kl_stop_early_and_run_through_with_one_read_back():
    """The counted path at 2050 rows.  The limit comes from the twin's composition alone (learn_twins.onpolicy_target, the rule
    of tests/test_gpu_onpolicy_learn.py): an early stop and a full iteration must both occur."""
    perms = LT.onpolicy_perms("ppo", 2, shape=WIDE)
    target, kls, star = LT.onpolicy_target("plain", 2, perms, shape=WIDE)
    a, b = LT.Learner("ppo", "plain", target, shape=WIDE), LT.OnPolicyTwin("ppo", "plain", target, shape=WIDE)
    logs = a.learn.learn(2 * WIDE.rows, seed=WIDE.seed, perms=perms)
    b.loop(2 * WIDE.rows, perms)
    K = WIDE.K
    print(f"\nsteps applied per iteration {b.applied} of K = {K}: early stops after minibatch "
          f"{[s for s in b.applied if s < K]} of their train(); i* = {star}")
    assert any(0 < s < K for s in b.applied), ("no iteration stops strictly inside its train()", b.applied, kls)
    assert any(s == K for s in b.applied), ("no iteration applies all K steps", b.applied, kls)
    assert a.learn.readbacks == 1 and a.learn.counter is not None and logs.iterations == 2
    LT.assert_onpolicy_equal(a, b, "1025 envs, target_kl", logs.device)
    assert all(float(a.opt.state[p]["step"]) == float(sum(b.applied)) for p in a.params)
    assert a.learn.counter.words[:3].cpu().tolist() == [a.model._n_updates, 0, sum(b.applied)]
    assert [int(v) for v in logs.history()[:, 8]] == b.applied
    a.close(); b.close()


# ------------------------------------------------------------------------------------------------- 10. episodes end, bootstrap
@pytest.mark.parametrize("kind", ["ppo", "a2c"])
def test_episodes_end_and_the_terminal_value_bootstrap_feeds_gae(kind):
    """fail_limit = 3, window = 4, five iterations of 33 envs x 3 steps.

    The CPU oracle (oracle/ref_lib.RefEnv, an episode cut when ``failed_num`` reaches 3) stepped on the initial policy's
    actions (tests/policy_ref.policy_forward in fp64 on the oracle's observations with ``philox_normal(5, t, envs)``) finishes
    0, 0, 28 episodes in the three steps of the first collect for PPO and 0, 0, 27 for A2C: more than window before the first
    train(), every one truncated (done && !complete), which is the branch that bootstraps."""
    a, b = LT.Learner(kind, shape=ENDING), LT.OnPolicyTwin(kind, shape=ENDING, keep=True)
    perms = LT.onpolicy_perms(kind, 5, shape=ENDING)
    logs = a.learn.learn(5 * ENDING.rows, seed=ENDING.seed, perms=perms)
    b.loop(5 * ENDING.rows, perms)
    episodes = _episodes(b)
    boots, monitor = 0, LR.MonitorRef(ENDING.n, ENDING.window)
    for i, out in enumerate(b.outs):
        h = {k: out[k].cpu().numpy() for k in ("reward", "value", "done", "complete", "last_value", "terminal_value", "advantages", "returns")}
        monitor.update(h["reward"], h["done"], h["complete"])
        need = (h["done"] != 0) & (h["complete"] == 0)
        assert (h["terminal_value"][~need] == 0.0).all()
        boots += int((h["terminal_value"][need] != 0.0).sum())
        ref = gae_ref.gae_ref(h["reward"], h["value"], h["done"], h["last_value"], h["terminal_value"], b.model.gamma, b.model.gae_lambda)
        for k in ("advantages", "returns"):
            assert gae_ref.same_bits(h[k], ref[k]) and np.isfinite(h[k]).all(), (kind, "collect", i, k)
    print(f"\n{kind}: episodes finished per collect {episodes}; {boots} truncated rows with a non-zero terminal_value")
    assert sum(episodes) > ENDING.window and _count(b.stats) == sum(episodes)
    assert boots >= 1
    LT.assert_onpolicy_equal(a, b, f"{kind} ending episodes", logs.device)
    got, want = logs.read(), monitor.logs()                                # the Monitor restatement on the twin's histories
    assert got["episodes"] == sum(episodes) == monitor.count
    for k in ("rollout/ep_rew_mean", "rollout/ep_len_mean"):
        assert got[k] == want[k], (k, got[k], want[k])
    assert np.array_equal(a.stats.ring.cpu().numpy().view(np.int64), monitor.ring().view(np.int64))
    a.close(); b.close()


# ------------------------------------------------------------------------------------------------- 11. counter carry
@pytest.mark.parametrize("kind", ["ppo", "a2c"])
def test_the_noise_counter_carries_into_its_high_word_inside_a_collect(kind):
    """steps start at 2^32 - 2 under a seed with a high word: the first collect draws at 2^32 - 2, 2^32 - 1, 2^32, the two that
    follow from 2^32 + 1 on."""
    s0 = 2 ** 32 - 2
    a, b = LT.Learner(kind, shape=CARRY), LT.OnPolicyTwin(kind, shape=CARRY, steps=s0, keep=True)
    a.learn.steps = s0                                                     # a plain attribute: the counter of the next collect
    perms = LT.onpolicy_perms(kind, 3, shape=CARRY)
    logs = a.learn.learn(3 * CARRY.rows, seed=WIDE_SEED, perms=perms)
    b.loop(3 * CARRY.rows, perms)
    assert a.learn.steps == s0 + 9 == b.steps and b.counters == [s0, s0 + 3, s0 + 6]
    LT.assert_onpolicy_equal(a, b, f"{kind} counter carry", logs.device)
    envs, worst = np.arange(CARRY.n, dtype=np.uint64), 0.0
    for out, counter in zip(b.outs, b.counters):
        eps = out["eps"].cpu().numpy()
        assert eps.shape == (3, CARRY.n, 3)
        for t in range(3):
            worst = max(worst, R.assert_within(eps[t], R.philox_normal(WIDE_SEED, counter + t, envs), f"{kind} eps at {counter + t}"))
            if counter + t >= 2 ** 32:                                     # the counter's high word reaches the draw
                assert R.ratio(eps[t], R.philox_normal(WIDE_SEED, (counter + t) & 0xFFFFFFFF, envs))[1].any()
    print(f"\n{kind}: rollout eps against the host Philox at counters {s0} .. {s0 + 8}: max |kernel - fp64| / bound {worst:.4f}")
    a.close(); b.close()
