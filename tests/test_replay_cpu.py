"""CPU: tests/replay_ref.py (the host restatement the device replay buffer is held to) is SB3 2.x's ReplayBuffer fed by
OffPolicyAlgorithm._store_transition -- a literal step-by-step transcription of both written out below -- bit for bit, plus
hand-worked cases, the Philox words behind the index draw against the Random123 known answers, and the index mapping's range
and uniformity."""
import copy
import math

import numpy as np
import pytest

import policy_ref
import replay_ref as R


# ------------------------------------------------------------------------------------------------ SB3, literally
class Sb3ReplayBuffer:
    """stable_baselines3.common.buffers.ReplayBuffer (2.x, optimize_memory_usage=False, Box spaces), its statements kept."""

    def __init__(self, buffer_size, n_envs, handle_timeout_termination=True):
        self.buffer_size = max(buffer_size // n_envs, 1)
        self.n_envs = n_envs
        self.pos, self.full = 0, False
        self.observations = np.zeros((self.buffer_size, n_envs, 18), dtype=np.float32)
        self.next_observations = np.zeros((self.buffer_size, n_envs, 18), dtype=np.float32)
        self.actions = np.zeros((self.buffer_size, n_envs, 3), dtype=np.float32)
        self.rewards = np.zeros((self.buffer_size, n_envs), dtype=np.float32)
        self.dones = np.zeros((self.buffer_size, n_envs), dtype=np.float32)
        self.handle_timeout_termination = handle_timeout_termination
        self.timeouts = np.zeros((self.buffer_size, n_envs), dtype=np.float32)

    def size(self):
        if self.full:
            return self.buffer_size
        return self.pos

    def add(self, obs, next_obs, action, reward, done, infos):
        action = action.reshape((self.n_envs, 3))
        self.observations[self.pos] = np.array(obs)
        self.next_observations[self.pos] = np.array(next_obs)
        self.actions[self.pos] = np.array(action)
        self.rewards[self.pos] = np.array(reward)
        self.dones[self.pos] = np.array(done)
        if self.handle_timeout_termination:
            self.timeouts[self.pos] = np.array([info.get("TimeLimit.truncated", False) for info in infos])
        self.pos += 1
        if self.pos == self.buffer_size:
            self.full = True
            self.pos = 0

    def _get_samples(self, batch_inds, env_indices):
        next_obs = self.next_observations[batch_inds, env_indices, :]
        return (self.observations[batch_inds, env_indices, :], self.actions[batch_inds, env_indices, :], next_obs,
                (self.dones[batch_inds, env_indices] * (1 - self.timeouts[batch_inds, env_indices])).reshape(-1, 1),
                self.rewards[batch_inds, env_indices].reshape(-1, 1))


def sb3_store_transition(replay_buffer, buffer_action, new_obs, reward, dones, infos, last_obs):
    """OffPolicyAlgorithm._store_transition without VecNormalize; returns the new _last_obs."""
    next_obs = copy.deepcopy(new_obs)
    for i, done in enumerate(dones):
        if done and infos[i].get("terminal_observation") is not None:
            next_obs[i] = infos[i]["terminal_observation"]
    replay_buffer.add(last_obs, next_obs, buffer_action, reward, dones, infos)
    return new_obs


def vec_env_infos(done, complete, terminal_obs):
    """What SB3MeshVecEnv._build_infos hands out for one vector step."""
    infos = [{"is_complete": bool(c)} for c in complete]
    for k in np.nonzero(done)[0]:
        infos[k] = {"is_complete": bool(complete[k]), "terminal_observation": terminal_obs[k].copy(),
                    "TimeLimit.truncated": not bool(complete[k])}
    return infos


def sb3_feed(buf, h, low_high=None):
    last_obs = h["obs0"]
    for t in range(len(h["obs_after"])):
        done = h["done"][t] != 0
        infos = vec_env_infos(done, h["complete"][t], h["terminal_obs"][t])
        a = h["actions"][t]
        if low_high is not None:          # SAC._sample_action: buffer_action = self.policy.scale_action(unscaled_action)
            low, high = np.asarray(low_high[0], np.float32), np.asarray(low_high[1], np.float32)
            a = 2.0 * ((a - low) / (high - low)) - 1.0
        reward = h["reward"][t].astype(np.float32)       # the VecEnv's step_wait returns float32 rewards
        last_obs = sb3_store_transition(buf, a, h["obs_after"][t], reward, done, infos, last_obs)


def assert_same_state(ref, sb3, what=""):
    assert (ref.pos, ref.full, ref.size(), ref.rows) == (sb3.pos, sb3.full, sb3.size(), sb3.buffer_size), what
    for k in R.ReplayRef.FIELDS:
        assert R.same_bits(getattr(ref, k), getattr(sb3, k)), (what, k)


LOW_HIGH = ([-1.0, -1.5, 0.0], [1.0, 1.5, 1.5])


@pytest.mark.parametrize("handle", [True, False])
@pytest.mark.parametrize("scale", [False, True])
@pytest.mark.parametrize("T,n,buffer_size,seed", [(1, 5, 50, 1), (7, 33, 33 * 4, 2), (12, 4, 48, 3), (40, 17, 17 * 9 + 5, 4),
                                                  (5, 8, 3, 5)])
def test_restatement_equals_sb3_transcription(T, n, buffer_size, seed, scale, handle):
    h = R.synthetic(T, n, seed, special=not scale)
    assert R.kinds_present(h["done"], h["complete"])
    lh = LOW_HIGH if scale else None
    ref = R.ReplayRef(buffer_size, n, handle_timeout_termination=handle)
    sb3 = Sb3ReplayBuffer(buffer_size, n, handle_timeout_termination=handle)
    for call in range(2):                                  # the second call continues where the first stopped
        ref.add_rollout(**h, low_high=lh)
        sb3_feed(sb3, h, lh)
        assert_same_state(ref, sb3, f"call {call}")
    rng = np.random.default_rng(seed)
    b, e = rng.integers(0, ref.size(), 200), rng.integers(0, n, 200)
    got, want = ref.get_samples(b, e), sb3._get_samples(b, e)
    assert got._fields == ("observations", "actions", "next_observations", "dones", "rewards")
    for g, w in zip(got, want):
        assert R.same_bits(g, w)
    assert got.dones.shape == (200, 1) and got.rewards.shape == (200, 1) and got.actions.shape == (200, 3)
    if handle:
        trunc = (ref.dones != 0) & (ref.timeouts != 0)
        assert not got.dones[trunc[b, e]].any()            # a truncated episode is not terminal for the critic target


def test_sb3_signature_add_equals_sb3():
    h = R.synthetic(6, 9, 11, special=True)
    ref, sb3 = R.ReplayRef(9 * 4, 9), Sb3ReplayBuffer(9 * 4, 9)
    last = h["obs0"]
    for t in range(6):
        done = h["done"][t] != 0
        infos = vec_env_infos(done, h["complete"][t], h["terminal_obs"][t])
        next_obs = np.where(done[:, None], h["terminal_obs"][t], h["obs_after"][t])
        rew = h["reward"][t].astype(np.float32)
        ref.add_sb3(last, next_obs, h["actions"][t], rew, done, infos)
        sb3.add(last, next_obs, h["actions"][t], rew, done, infos)
        last = h["obs_after"][t]
        assert_same_state(ref, sb3, f"step {t}")


# ------------------------------------------------------------------------------------------------ hand-worked cases
def _step(n, v, done=0, complete=0):
    o = np.full((n, 18), v, np.float32)
    return dict(obs=o, new_obs=o + 1, terminal_obs=o + 100, action=np.full((n, 3), v, np.float32), reward=np.full(n, float(v)),
                done=np.full(n, done, np.uint8), complete=np.full(n, complete, np.uint8))


def test_full_flips_exactly_at_rows_and_the_write_wraps():
    b = R.ReplayRef(buffer_size=6, n_envs=2)         # 3 rows
    assert (b.rows, b.size(), b.full) == (3, 0, False)
    for v in (1, 2):
        b.add_step(**_step(2, v))
    assert (b.pos, b.full, b.size()) == (2, False, 2)
    b.add_step(**_step(2, 3))
    assert (b.pos, b.full, b.size()) == (0, True, 3)
    b.add_step(**_step(2, 4))                          # overwrites row 0
    assert (b.pos, b.full, b.size()) == (1, True, 3)
    assert b.rewards[:, 0].tolist() == [4.0, 2.0, 3.0]
    assert b.observations[0, 1, 0] == 4.0 and b.next_observations[0, 1, 0] == 5.0


def test_buffer_smaller_than_n_envs_keeps_one_row():
    b = R.ReplayRef(buffer_size=3, n_envs=8)
    assert b.rows == 1
    b.add_step(**_step(8, 1))
    assert (b.pos, b.full, b.size()) == (0, True, 1)
    b.add_step(**_step(8, 2))
    assert b.rewards[0].tolist() == [2.0] * 8


def test_done_complete_against_done_truncated():
    b = R.ReplayRef(buffer_size=8, n_envs=2)
    s = _step(2, 1)
    s["done"], s["complete"] = np.array([1, 1], np.uint8), np.array([1, 0], np.uint8)
    b.add_step(**s)
    assert b.dones[0].tolist() == [1.0, 1.0] and b.timeouts[0].tolist() == [0.0, 1.0]
    assert b.next_observations[0, :, 0].tolist() == [101.0, 101.0]       # the terminal observation, not the reset one
    got = b.get_samples([0, 0], [0, 1])
    assert got.dones.tolist() == [[1.0], [0.0]]
    b.add_step(**_step(2, 5))
    assert b.next_observations[1, :, 0].tolist() == [6.0, 6.0] and b.timeouts[1].tolist() == [0.0, 0.0]


def test_handle_timeout_termination_false_keeps_timeouts_zero():
    b = R.ReplayRef(buffer_size=8, n_envs=2, handle_timeout_termination=False)
    s = _step(2, 1, done=1, complete=0)
    b.add_step(**s)
    assert b.timeouts[0].tolist() == [0.0, 0.0] and b.get_samples([0], [1]).dones.tolist() == [[1.0]]


def test_optimize_memory_usage_is_refused_by_name():
    with pytest.raises(ValueError, match="optimize_memory_usage"):
        R.ReplayRef(10, 2, optimize_memory_usage=True)


def test_scale_action_is_the_float32_expression():
    a = np.array([[-1.0, -1.5, 0.0], [1.0, 1.5, 1.5], [0.3, 0.7, 0.2]], np.float32)
    s = R.scale_action(a, *LOW_HIGH)
    assert s.dtype == np.float32 and s[0].tolist() == [-1.0] * 3 and s[1].tolist() == [1.0] * 3
    low, high = np.float32(-1.5), np.float32(1.5)
    x = np.float32(0.7)
    assert s[2, 1] == np.float32(np.float32(2.0) * np.float32(np.float32(x - low) / np.float32(high - low))) - np.float32(1.0)


# ------------------------------------------------------------------------------------------------ the index draw
@pytest.mark.parametrize("ctr, key, want", [          # the Random123 known answers of tests/test_policy_ref_cpu.py
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_the_draws_philox_reproduces_the_known_answers(ctr, key, want):
    got = policy_ref.philox4x32(*[np.array([c], np.uint64) for c in ctr], *key)
    assert tuple(int(w[0]) for w in got) == want


def test_draw_uses_the_known_answer_philox_with_its_own_tag():
    seed, counter = (7 << 32) | 12345, (3 << 32) | 99
    i = np.arange(5, dtype=np.uint64)
    w = policy_ref.philox4x32(i, 99, 3, R.DRAW_TAG, 12345, 7)
    rows, envs = R.draw_indices(seed, counter, 5, 1000, 4096)
    assert rows.tolist() == [(int(x) * 1000) >> 32 for x in w[0]] and envs.tolist() == [(int(x) * 4096) >> 32 for x in w[1]]
    noise = policy_ref.philox_words(seed, counter, i)            # the exploration noise of env i at the same (seed, counter)
    assert R.DRAW_TAG != 0 and not np.array_equal(noise[0], w[0])
    r2, e2 = R.draw_indices(seed, counter, 3, 1000, 4096, first=2)   # sample i depends on i alone, not on the batch size
    assert r2.tolist() == rows[2:].tolist() and e2.tolist() == envs[2:].tolist()


@pytest.mark.parametrize("bound", [1, 2, 3, 244, 2 ** 20, 2 ** 31 - 1])
def test_mapped_indices_are_in_range(bound):
    edge = np.array([0, 1, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 2, 2 ** 32 - 1], np.uint64)
    got = R.map_index(edge, bound)
    assert got.dtype == np.int32 and got.min() >= 0 and got.max() < bound
    assert got[0] == 0 and got[-1] == bound - 1
    rows, envs = R.draw_indices(5, 6, 100000, bound, bound)
    for x in (rows, envs):
        assert x.dtype == np.int32 and x.min() >= 0 and x.max() < bound
    if bound <= 3:
        assert set(rows.tolist()) == set(range(bound))


def chi2_quantile_999(dof):
    """The 99.9 % quantile of chi-square with dof degrees of freedom by Wilson-Hilferty (relative error below 1e-3 for
    dof >= 100, which is far less than the distance between a uniform and a broken mapping)."""
    z = 3.090232306167813
    return dof * (1.0 - 2.0 / (9.0 * dof) + z * math.sqrt(2.0 / (9.0 * dof))) ** 3


@pytest.mark.parametrize("seed", [1, 20261016, (0xDEADBEEF << 32) | 0x12345678])
@pytest.mark.parametrize("bound", [244, 1000, 2 ** 20, 2 ** 31 - 1])
def test_draws_are_uniform_by_chi_square(seed, bound):
    N = 10 ** 6
    rows, envs = R.draw_indices(seed, seed ^ 0x5555, N, bound, bound)
    cells = min(bound, 1000)
    for name, x in (("rows", rows), ("envs", envs)):
        cell = x.astype(np.int64) * cells // bound
        counts = np.bincount(cell, minlength=cells).astype(np.float64)
        # expected count of a cell: the share of [0, bound) that maps to it
        edges = -(-np.arange(cells + 1, dtype=np.int64) * bound // cells)    # ceil(c * bound / cells)
        expect = np.diff(edges) / bound * N
        stat = float(((counts - expect) ** 2 / expect).sum())
        limit = chi2_quantile_999(cells - 1)
        print(f"seed {seed:#x} bound {bound} {name}: chi2 = {stat:.1f}, 99.9 % quantile {limit:.1f} ({cells} cells)")
        assert stat < limit
    # the two indices of a sample come from different words: not the same number twice
    assert (rows != envs).mean() > 0.9


# ------------------------------------------------------------------------------------------------ the C-ABI's names
def test_capi_exports_name_the_replay_entries():
    from reinforcementlearning4meshgeneration_amd import _capi
    for name in ("meshenv_replay_add", "meshenv_replay_sample", "meshenv_replay_record_floats"):
        assert name in _capi.EXPORTS
    L = _capi.load()
    R_ = L.meshenv_replay_record_floats()
    assert R_ >= 42 and R_ % 4 == 0          # 42 payload floats, whole 16-byte pieces
