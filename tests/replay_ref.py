"""Host restatement of the device replay buffer (csrc/meshenv_replay.h, DeviceReplayBuffer) in numpy: SB3 2.x's
ReplayBuffer (optimize_memory_usage=False) fed by OffPolicyAlgorithm._store_transition, one vector step at a time, SB3's
_get_samples, and the device's own index draw.  Nothing here touches a device.

Storage      rows = max(buffer_size // n_envs, 1); observations / next_observations [rows, n, 18], actions [rows, n, 3],
             rewards / dones / timeouts [rows, n], all float32; pos, full; size() = rows if full else pos.
add          next_obs[k] = terminal_obs[k] if done[k] else new_obs[k]; rewards = float32(reward);  dones = done;
             timeouts = done and not complete (infos[k]["TimeLimit.truncated"], which SB3MeshVecEnv sets to not is_complete
             on the envs that are done), 0 everywhere with handle_timeout_termination=False; written at pos; pos += 1; at
             pos == rows: full = True, pos = 0.
scaling      with (low, high): actions = 2.0 * ((a - low) / (high - low)) - 1.0 in float32 (SB3's policy.scale_action).
sample       _get_samples(batch_inds, env_inds) -> (observations, actions, next_observations,
             (dones * (1 - timeouts)).reshape(-1, 1), rewards.reshape(-1, 1)).
index draw   sample i of a batch at (seed, counter): w = Philox4x32-10(counter words (i, counter lo, counter hi, DRAW_TAG),
             key (seed lo, seed hi));  row = (w[0] * size) >> 32,  env = (w[1] * n_envs) >> 32  (multiply-high of a uniform
             32-bit word: in [0, bound) for every bound <= 2^32, each index hit floor or ceil of 2^32 / bound times).
             DRAW_TAG = 1; the exploration noise draws use 0 in that word, so the two streams never meet."""
from collections import namedtuple

import numpy as np

import policy_ref

OBS_DIM, ACT_DIM = 18, 3
DRAW_TAG = 1
MASK = 0xFFFFFFFF

ReplayBufferSamples = namedtuple("ReplayBufferSamples", ["observations", "actions", "next_observations", "dones", "rewards"])


def draw_indices(seed, counter, batch, size, n_envs, first=0):
    """(rows, envs) int32 [batch] of samples first .. first + batch - 1."""
    i = np.arange(first, first + batch, dtype=np.uint64)
    w = policy_ref.philox4x32(i, counter & MASK, (counter >> 32) & MASK, DRAW_TAG, seed & MASK, (seed >> 32) & MASK)
    return map_index(w[0], size), map_index(w[1], n_envs)


def map_index(word, bound):
    """A uniform 32-bit word to [0, bound): the high half of the 64-bit product."""
    return ((np.asarray(word, np.uint64) * np.uint64(bound)) >> np.uint64(32)).astype(np.int32)


def scale_action(a, low, high):
    """SB3 policy.scale_action on float32 arrays: one rounding per operation."""
    a, low, high = (np.asarray(x, np.float32) for x in (a, low, high))
    with np.errstate(all="ignore"):
        return (np.float32(2.0) * ((a - low) / (high - low)) - np.float32(1.0)).astype(np.float32)


class ReplayRef:
    def __init__(self, buffer_size, n_envs, handle_timeout_termination=True, optimize_memory_usage=False):
        if optimize_memory_usage:
            raise ValueError("optimize_memory_usage=True is not supported")
        self.n_envs = int(n_envs)
        self.rows = self.buffer_size = max(int(buffer_size) // self.n_envs, 1)
        self.handle_timeout_termination = bool(handle_timeout_termination)
        r, n = self.rows, self.n_envs
        self.observations = np.zeros((r, n, OBS_DIM), np.float32)
        self.next_observations = np.zeros((r, n, OBS_DIM), np.float32)
        self.actions = np.zeros((r, n, ACT_DIM), np.float32)
        self.rewards = np.zeros((r, n), np.float32)
        self.dones = np.zeros((r, n), np.float32)
        self.timeouts = np.zeros((r, n), np.float32)
        self.pos, self.full = 0, False

    FIELDS = ("observations", "next_observations", "actions", "rewards", "dones", "timeouts")

    def fill(self, pattern):
        """Every stored float32 set to the bits of `pattern` (the state of a freshly filled device store)."""
        for k in self.FIELDS:
            getattr(self, k).view(np.uint32)[...] = np.uint32(pattern)

    def size(self):
        return self.rows if self.full else self.pos

    def add_step(self, obs, new_obs, terminal_obs, action, reward, done, complete, low_high=None):
        """One vector step: obs / new_obs / terminal_obs [n, 18] float32, action [n, 3] float32, reward [n] float64,
        done / complete [n] (0 / 1)."""
        d = np.asarray(done) != 0
        p = self.pos
        self.observations[p] = obs
        self.next_observations[p] = np.where(d[:, None], terminal_obs, new_obs)
        self.actions[p] = action if low_high is None else scale_action(action, low_high[0], low_high[1])
        self.rewards[p] = np.asarray(reward).astype(np.float32)
        self.dones[p] = d
        self.timeouts[p] = (d & (np.asarray(complete) == 0)) if self.handle_timeout_termination else 0
        self.pos += 1
        if self.pos == self.rows:
            self.full, self.pos = True, 0

    def add_rollout(self, obs0, obs_after, terminal_obs, actions, reward, done, complete, low_high=None):
        """T vector steps, one add_step each: obs0 [n, 18] is what step 0 acted on, obs_after[t] the observation after
        step t (and so what step t + 1 acted on)."""
        for t in range(len(obs_after)):
            self.add_step(obs0 if t == 0 else obs_after[t - 1], obs_after[t], terminal_obs[t], actions[t], reward[t], done[t],
                          complete[t], low_high)

    def add_sb3(self, obs, next_obs, action, reward, done, infos):
        """SB3's ReplayBuffer.add signature (next_obs already holds the terminal observation of finished envs)."""
        trunc = np.array([bool(i.get("TimeLimit.truncated", False)) for i in infos])
        self.add_step(obs, next_obs, next_obs, action, reward, done, ~trunc)

    def get_samples(self, batch_inds, env_inds):
        b, e = np.asarray(batch_inds), np.asarray(env_inds)
        with np.errstate(all="ignore"):
            dones = (self.dones[b, e] * (np.float32(1.0) - self.timeouts[b, e])).reshape(-1, 1)
        return ReplayBufferSamples(self.observations[b, e], self.actions[b, e], self.next_observations[b, e], dones,
                                   self.rewards[b, e].reshape(-1, 1))

    def sample(self, batch_size, seed=0, counter=0):
        if self.size() < 1:
            raise ValueError("sample from an empty buffer")
        rows, envs = draw_indices(seed, counter, batch_size, self.size(), self.n_envs)
        return self.get_samples(rows, envs), rows, envs


def synthetic(T, n, seed, special=True):
    """A seeded history of T vector steps shaped like the rollout calls': float32 observations and Box actions with full
    mantissas, float64 rewards, ~8 % done of which half complete, with steps 0..2 of env 0 forced to not-done /
    done-complete / done-truncated where T allows (otherwise spread over the first envs), terminal observations only where
    done.  With special (and n >= 4): env 1 carries subnormals, env 2 NaNs (observations and reward), env 3 +-inf."""
    rng = np.random.default_rng(seed)
    obs0 = rng.standard_normal((n, OBS_DIM)).astype(np.float32)
    obs_after = rng.standard_normal((T, n, OBS_DIM)).astype(np.float32)
    terminal_obs = rng.standard_normal((T, n, OBS_DIM)).astype(np.float32)
    actions = rng.uniform([-1, -1.5, 0], [1, 1.5, 1.5], size=(T, n, 3)).astype(np.float32)
    reward = rng.standard_normal((T, n)) * rng.uniform(0.1, 20.0, (T, n))
    done = (rng.random((T, n)) < 0.08).astype(np.uint8)
    complete = (done & (rng.random((T, n)) < 0.5)).astype(np.uint8)
    flat_d, flat_c = done.reshape(-1), complete.reshape(-1)     # [T * n] views: the first three transitions hold all kinds
    if T * n >= 3:
        flat_d[:3] = (0, 1, 1)
        flat_c[:3] = (0, 1, 0)
    terminal_obs[done == 0] = 0.0
    if special and n >= 4:
        obs_after[:, 1] = (np.float32(1e-39) * rng.uniform(-1, 1, (T, OBS_DIM))).astype(np.float32)
        reward[:, 1] = rng.uniform(-1, 1, T) * 1e-39
        obs_after[:, 2, ::3] = np.nan
        terminal_obs[:, 2, 1] = np.nan
        reward[T // 2, 2] = np.nan
        obs_after[:, 3, 0], obs_after[:, 3, 1] = np.inf, -np.inf
        reward[(T - 1) // 3, 3] = -np.inf
    return dict(obs0=obs0, obs_after=obs_after, terminal_obs=terminal_obs, actions=actions, reward=reward, done=done,
                complete=complete)


def kinds_present(done, complete):
    """Does a history hold all of not-done, done-complete and done-truncated?"""
    d, c = np.asarray(done) != 0, np.asarray(complete) != 0
    return bool((~d).any() and (d & c).any() and (d & ~c).any())


def same_bits(a, b):
    """float32 arrays equal bit for bit, NaN payloads included."""
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == np.float32 and b.dtype == np.float32 and a.shape == b.shape and \
        np.array_equal(np.ascontiguousarray(a).view(np.int32), np.ascontiguousarray(b).view(np.int32))
