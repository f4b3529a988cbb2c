"""Host restatement of the off-policy learn loop's own pieces (reinforcementlearning4meshgeneration_amd/offpolicy_learn.py,
csrc/meshenv_learn.h) in numpy / pure Python.  Nothing here touches a device.

schedule      SB3's OffPolicyAlgorithm.learn / collect_rollouts with train_freq in vector steps, one env step at a time: a step
              is a warm-up step iff num_timesteps < learning_starts before its increment; train() follows a collect iff
              num_timesteps > 0 and num_timesteps > learning_starts; gradient_steps < 0 is the T just collected.
uniform draw  element (t, env, c) of k_uniform_actions: Philox4x32-10 keyed by seed at counter words
              (env, lo(counter + t), hi(counter + t), 4), output word c; u = float32(word >> 8) * 2^-24;
              buffer = 2 u - 1;  action = low + 0.5 * (buffer + 1) * (high - low), every operation rounded to float32.
monitor       SB3's Monitor per env (rewards appended, ep_rew = sum(rewards) = the sequential float64 sum, ep_len = len) and
              ep_info_buffer = deque(maxlen=window), extended per vector step in env order (flat index t * n + env)."""
from collections import deque

import numpy as np

import policy_ref

UNIFORM_TAG = 4
MASK = 0xFFFFFFFF
MASK64 = 2 ** 64 - 1


# ----------------------------------------------------------------------------------------------------------------- schedule
def sb3_schedule(num_timesteps, total_timesteps, n_envs, T, learning_starts, gradient_steps):
    """[(per-step warm-up flags of the collect, num_timesteps after it, gradient steps of its train() or 0)], stepping
    num_timesteps one env step at a time as collect_rollouts does.  total_timesteps is the absolute target."""
    out = []
    while num_timesteps < total_timesteps:
        flags = []
        for _ in range(T):
            flags.append(num_timesteps < learning_starts)
            num_timesteps += n_envs
        K = 0
        if num_timesteps > 0 and num_timesteps > learning_starts:
            K = gradient_steps if gradient_steps >= 0 else T
        out.append((flags, num_timesteps, K))
    return out


# ------------------------------------------------------------------------------------------------------------- uniform draw
def uniform_words(seed, counter, T, n):
    """uint32 [T, n, 3]: output words 0..2 of step t, env e."""
    out = np.empty((T, n, 3), np.uint32)
    env = np.arange(n, dtype=np.uint64)
    for t in range(T):
        c = (counter + t) & MASK64                      # the 64-bit sum carries into the high word
        w = policy_ref.philox4x32(env, c & MASK, (c >> 32) & MASK, UNIFORM_TAG, seed & MASK, (seed >> 32) & MASK)
        for k in range(3):
            out[t, :, k] = w[k]
    return out


def unscale_action(s, low, high):
    """low + 0.5 * (s + 1) * (high - low) in float32, one rounding per operation (k_policy_forward's expression)."""
    s, low, high = (np.asarray(x, np.float32) for x in (s, low, high))
    return (low + np.float32(0.5) * (s + np.float32(1.0)) * (high - low)).astype(np.float32)


def uniform_actions(seed, counter, T, n, low, high):
    """(actions, buffer_actions) float32 [T, n, 3]."""
    w = uniform_words(seed, counter, T, n)
    u = (w >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    buf = (np.float32(2.0) * u - np.float32(1.0)).astype(np.float32)
    return unscale_action(buf, low, high), buf


# ------------------------------------------------------------------------------------------------------------------ monitor
class MonitorRef:
    """n Monitors and SB3's ep_info_buffer.  order: "t_env" (SB3: per vector step, envs ascending) or "env_t" (the wrong
    order a column-major traversal would give; kept so that a test can show it tells the two apart)."""

    def __init__(self, n_envs, window=100, order="t_env"):
        self.n, self.window, self.order = n_envs, window, order
        self.rewards = [[] for _ in range(n_envs)]
        self.buffer = deque(maxlen=window)
        self.count = 0

    def update(self, reward, done, complete):
        reward, done, complete = np.asarray(reward, np.float64), np.asarray(done), np.asarray(complete)
        T, n = done.shape
        assert n == self.n
        finished = []
        for t in range(T):
            for e in range(n):
                self.rewards[e].append(float(reward[t, e]))
                if done[t, e]:
                    ret = 0.0
                    for r in self.rewards[e]:           # sum(rewards) of Python <= 3.11: left to right from 0.0
                        ret += r
                    finished.append(((t, e), (ret, float(len(self.rewards[e])), 1.0 if complete[t, e] else 0.0)))
                    self.rewards[e] = []
        if self.order == "env_t":
            finished.sort(key=lambda x: (x[0][1], x[0][0]))
        for _, ep in finished:
            self.buffer.append(ep)
        self.count += len(finished)

    def carries(self):
        """(carry_return float64 [n], carry_len int32 [n]) of the episodes in flight."""
        ret = np.zeros(self.n, np.float64)
        for e, rs in enumerate(self.rewards):
            acc = 0.0
            for r in rs:
                acc += r
            ret[e] = acc
        return ret, np.array([len(rs) for rs in self.rewards], np.int32)

    def ring(self):
        """float64 [window, 3] as the device lays it out: episode k (0-based, over the run) at slot k % window; zeros where
        nothing was written yet."""
        out = np.zeros((self.window, 3), np.float64)
        first = self.count - len(self.buffer)
        for k, ep in enumerate(self.buffer):
            out[(first + k) % self.window] = ep
        return out

    def logs(self):
        d = {"episodes": self.count}
        if self.buffer:
            eps = np.array(self.buffer, np.float64)
            d["rollout/ep_rew_mean"] = float(np.mean(eps[:, 0]))
            d["rollout/ep_len_mean"] = float(np.mean(eps[:, 1]))
            d["complete_rate"] = float(np.mean(eps[:, 2]))
        return d


def synthetic_history(T, n, seed, p_done=0.3):
    """reward float64 [T, n] with full mantissas of mixed magnitude (so that the order of a sum shows in its bits), done and
    complete uint8 [T, n]."""
    rng = np.random.default_rng(seed)
    reward = rng.standard_normal((T, n)) * 10.0 ** rng.integers(-6, 7, (T, n))
    done = (rng.random((T, n)) < p_done).astype(np.uint8)
    complete = (done & (rng.random((T, n)) < 0.5)).astype(np.uint8)
    return reward, done, complete
