"""CPU: tests/gae_ref.py (the host restatement meshenv_gae is held to) is the float32 loop users run today -- a literal
transcription of SB3's RolloutBuffer.compute_returns_and_advantage with collect_rollouts' truncation bootstrap, and
examples/ppo_rollout.py::gae on CPU torch tensors -- bit for bit, plus hand-worked and limiting cases."""
import numpy as np
import pytest

import gae_ref as R


def sb3_gae(reward, value, done, complete, last_value, terminal_value, gamma, gae_lambda):
    """SB3 2.x, literally: OnPolicyAlgorithm.collect_rollouts (rewards[idx] += gamma * terminal_value where
    TimeLimit.truncated; RolloutBuffer.add stores float32, episode_starts = the previous step's dones) and
    RolloutBuffer.compute_returns_and_advantage(last_values, dones)."""
    T, n = reward.shape
    rewards = np.zeros((T, n), np.float32)
    episode_starts = np.zeros((T, n), np.float32)
    values = np.zeros((T, n), np.float32)
    last_episode_starts = np.zeros(n, dtype=bool)
    for t in range(T):
        rewards_t = reward[t].copy()
        for idx in range(n):
            if done[t, idx] and not complete[t, idx]:           # infos[idx]["TimeLimit.truncated"]
                rewards_t[idx] = np.float32(rewards_t[idx]) + gamma * terminal_value[t, idx]
        rewards[t] = np.array(rewards_t)
        episode_starts[t] = np.array(last_episode_starts)
        values[t] = value[t]
        last_episode_starts = done[t].astype(bool)
    dones = last_episode_starts
    advantages = np.zeros((T, n), np.float32)
    last_values = last_value.flatten()
    last_gae_lam = 0
    with np.errstate(all="ignore"):
        for step in reversed(range(T)):
            if step == T - 1:
                next_non_terminal = 1.0 - dones.astype(np.float32)
                next_values = last_values
            else:
                next_non_terminal = 1.0 - episode_starts[step + 1]
                next_values = values[step + 1]
            delta = rewards[step] + gamma * next_values * next_non_terminal - values[step]
            last_gae_lam = delta + gamma * gae_lambda * next_non_terminal * last_gae_lam
            advantages[step] = last_gae_lam
        returns = advantages + values
    return advantages, returns, rewards


COEFFS = [(0.99, 0.95), (0.99, 1.0), (1.0, 1.0), (0.9, 0.0), (0.0, 0.95), (0.95, 0.0), (0.95, 1.0)]


@pytest.mark.parametrize("gamma,gae_lambda", COEFFS)
@pytest.mark.parametrize("T,n,seed", [(1, 5, 1), (7, 33, 2), (300, 1000, 3)])
def test_restatement_equals_sb3_transcription(T, n, seed, gamma, gae_lambda):
    h = R.synthetic(T, n, seed, special=False)
    ref = R.gae_ref(h["reward"], h["value"], h["done"], h["last_value"], h["terminal_value"], gamma, gae_lambda)
    adv, ret, rew = sb3_gae(h["reward"], h["value"], h["done"], h["complete"], h["last_value"], h["terminal_value"],
                            gamma, gae_lambda)
    assert R.same_bits(ref["rewards"], rew)
    assert R.same_bits(ref["advantages"], adv)
    assert R.same_bits(ref["returns"], ret)


@pytest.mark.parametrize("gamma,gae_lambda", COEFFS)
@pytest.mark.parametrize("T,n,seed", [(1, 5, 4), (7, 33, 5), (300, 1000, 6)])
def test_restatement_equals_the_examples_torch_loop(T, n, seed, gamma, gae_lambda):
    torch = pytest.importorskip("torch")
    h = R.synthetic(T, n, seed)
    ref = R.gae_ref(h["reward"], h["value"], h["done"], h["last_value"], h["terminal_value"], gamma, gae_lambda)
    out = {k: torch.from_numpy(h[k]) for k in ("reward", "value", "done", "last_value", "terminal_value")}
    adv, ret = R.example_gae()(torch, out, gamma, gae_lambda)
    assert R.same_bits(ref["advantages"], adv.numpy())
    assert R.same_bits(ref["returns"], ret.numpy())
    assert np.isnan(ref["advantages"][:, 2]).any() and (ref["advantages"][:, 1] != 0).any()


def test_hand_worked_T3():
    """gamma = lambda = 0.5 (g = 0.5, gl = 0.25) on small integers: every intermediate is exact."""
    reward = np.array([[1, 1], [2, 2], [3, 3]], np.float64)
    value = np.array([[1, 1], [2, 2], [4, 4]], np.float32)
    done = np.array([[0, 0], [0, 1], [0, 0]], np.uint8)
    tv = np.array([[0, 0], [0, 6], [0, 0]], np.float32)    # env 1 truncated at t = 1, V(terminal obs) = 6
    last_value = np.array([8, 8], np.float32)
    out = R.gae_ref(reward, value, done, last_value, tv, 0.5, 0.5)
    # env 0: delta = 3, 2, 1; adv = 3, 2 + 0.25 * 3, 1 + 0.25 * 2.75
    # env 1: t = 1 r = 2 + 0.5 * 6 = 5, nnt = 0: delta = 5 - 2 = 3, adv = 3; t = 0: 1 + 0.25 * 3
    np.testing.assert_array_equal(out["advantages"], np.array([[1.6875, 1.75], [2.75, 3], [3, 3]], np.float32))
    np.testing.assert_array_equal(out["returns"], np.array([[2.6875, 2.75], [4.75, 5], [7, 7]], np.float32))
    np.testing.assert_array_equal(out["rewards"], np.array([[1, 1], [2, 5], [3, 3]], np.float32))


def test_gamma_zero_is_the_one_step_advantage():
    h = R.synthetic(50, 64, 7, special=False)
    out = R.gae_ref(h["reward"], h["value"], h["done"], h["last_value"], h["terminal_value"], 0.0, 0.95)
    r = h["reward"].astype(np.float32)    # g * terminal_value = 0
    assert R.same_bits(out["rewards"], r + np.float32(0.0))
    assert R.same_bits(out["advantages"], r - h["value"])


def test_lambda_zero_is_the_td_error():
    h = R.synthetic(50, 64, 8, special=False)
    g = np.float32(0.99)
    out = R.gae_ref(h["reward"], h["value"], h["done"], h["last_value"], h["terminal_value"], 0.99, 0.0)
    next_v = np.concatenate([h["value"][1:], h["last_value"][None]])
    nnt = np.float32(1) - h["done"].astype(np.float32)
    assert R.same_bits(out["advantages"], (out["rewards"] + (g * next_v) * nnt) - h["value"])


def test_lambda_one_without_dones_is_the_discounted_return_minus_value():
    """lambda = 1, no episode end: returns = r_t + g r_{t+1} + ... + g^(T-t) last_value (to float32 rounding)."""
    h = R.synthetic(20, 16, 9, with_terminal=False, special=False)
    done = np.zeros_like(h["done"])
    out = R.gae_ref(h["reward"], h["value"], done, h["last_value"], None, 0.9, 1.0)
    r = h["reward"].astype(np.float32).astype(np.float64)
    G = h["last_value"].astype(np.float64)
    for t in reversed(range(20)):
        G = r[t] + np.float64(np.float32(0.9)) * G
        np.testing.assert_allclose(out["returns"][t], G, rtol=1e-4, atol=1e-3)


def test_terminal_value_none_keeps_the_float32_reward():
    h = R.synthetic(9, 10, 10)
    out = R.gae_ref(h["reward"], h["value"], h["done"], h["last_value"], None)
    assert R.same_bits(out["rewards"], h["reward"].astype(np.float32))
