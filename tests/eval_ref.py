"""Host restatements of policy evaluation over recorded [T, n] reward / done / complete streams (numpy only).

sb3_evaluate: a transcription of SB3 2.x's evaluate_policy loop (stable_baselines3/common/evaluation.py, the branch without
a Monitor wrapper) with env.step replaced by the recorded rows; per recorded episode it also keeps env, step, the float64
return and is_complete.  device_layout: the bookkeeping of k_eval_tally (csrc/meshenv_eval.h) restated -- one slot range per
env, filled lane by lane, sorted by (step, env) afterwards.  The two must agree bit for bit."""
import numpy as np


def sb3_targets(n_eval_episodes, n_envs):
    return np.array([(n_eval_episodes + i) // n_envs for i in range(n_envs)], dtype="int")


def sb3_evaluate(reward, done, complete, targets, max_steps=None):
    """reward [T, n] float64 as the env returns it (handed to SB3 as float32, as SB3MeshVecEnv does), done / complete
    [T, n].  Returns dict of per-episode lists in SB3's append order plus steps (vector steps consumed) and finished."""
    T, n_envs = reward.shape
    max_steps = T if max_steps is None else min(T, max_steps)
    episode_rewards, episode_lengths = [], []
    rec = dict(env=[], step=[], return_raw=[], complete=[])
    episode_counts = np.zeros(n_envs, dtype="int")
    episode_count_targets = np.asarray(targets, dtype="int")
    current_rewards = np.zeros(n_envs)
    current_raw = np.zeros(n_envs)
    current_lengths = np.zeros(n_envs, dtype="int")
    t = 0
    while (episode_counts < episode_count_targets).any() and t < max_steps:
        rewards = reward[t].astype(np.float32)   # SB3MeshVecEnv.step_wait: float32 rewards
        dones = done[t].astype(bool)
        current_rewards += rewards
        current_raw += reward[t]
        current_lengths += 1
        for i in range(n_envs):
            if episode_counts[i] < episode_count_targets[i]:
                if dones[i]:
                    episode_rewards.append(current_rewards[i])
                    episode_lengths.append(current_lengths[i])
                    episode_counts[i] += 1
                    rec["env"].append(i); rec["step"].append(t); rec["return_raw"].append(current_raw[i])
                    rec["complete"].append(bool(complete[t, i]))
                    current_rewards[i] = 0
                    current_lengths[i] = 0
            if dones[i]:
                current_raw[i] = 0
        t += 1
    return dict(episode_rewards=episode_rewards, episode_lengths=episode_lengths, steps=t,
                finished=bool((episode_counts >= episode_count_targets).all()), **rec)


def device_layout(reward, done, complete, targets, max_steps=None):
    """k_eval_tally's layout: per-env accumulators, record k of env e in slot offset[e] + k, then sorted by (step, env)."""
    T, n = reward.shape
    max_steps = T if max_steps is None else min(T, max_steps)
    targets = np.asarray(targets, np.int64)
    offset = np.concatenate([[0], np.cumsum(targets)[:-1]]).astype(np.int64)
    total = int(targets.sum())
    slots = dict(env=np.zeros(total, np.int64), step=np.zeros(total, np.int64), length=np.zeros(total, np.int64),
                 ret=np.zeros(total), raw=np.zeros(total), complete=np.zeros(total, bool))
    count = np.zeros(n, np.int64)
    length = np.zeros(n, np.int64)
    ret = np.zeros(n)
    raw = np.zeros(n)
    short = int((targets > 0).sum())
    t = 0
    while short > 0 and t < max_steps:
        for e in range(n):   # one lane per env
            r = reward[t, e]
            length[e] += 1
            ret[e] = ret[e] + np.float64(np.float32(r))
            raw[e] = raw[e] + r
            if done[t, e]:
                if count[e] < targets[e]:
                    s = offset[e] + count[e]
                    slots["env"][s], slots["step"][s], slots["length"][s] = e, t, length[e]
                    slots["ret"][s], slots["raw"][s], slots["complete"][s] = ret[e], raw[e], bool(complete[t, e])
                    count[e] += 1
                    short -= int(count[e] == targets[e])
                length[e], ret[e], raw[e] = 0, 0.0, 0.0
        t += 1
    keep = (np.arange(total) - offset[np.repeat(np.arange(n), targets)]) < count[np.repeat(np.arange(n), targets)]
    order = np.lexsort((slots["env"][keep], slots["step"][keep]))
    out = {k: v[keep][order] for k, v in slots.items()}
    return dict(episode_rewards=list(out["ret"]), episode_lengths=list(out["length"]), env=list(out["env"]),
                step=list(out["step"]), return_raw=list(out["raw"]), complete=list(out["complete"]), steps=t,
                finished=short == 0)


def synthetic(T, n, seed, p_done=0.05, burst=None):
    """Reward / done / complete streams: float64 rewards with low bits (float32 rounding matters), done with probability
    p_done; burst = a step at which every env is done at once."""
    rng = np.random.default_rng(seed)
    reward = rng.normal(0, 1, (T, n)) * np.exp(rng.uniform(-3, 3, (T, n)))
    done = rng.random((T, n)) < p_done
    if burst is not None:
        done[burst] = True
    complete = done & (rng.random((T, n)) < 0.4)
    return reward, done.astype(np.uint8), complete.astype(np.uint8)


def sb3_evaluate_fast(reward, done, complete, targets, max_steps=None):
    """sb3_evaluate with the loop over envs vectorised (the envs of one step are visited in increasing order, as there):
    the form the GPU tests use on [T, 4096] streams.  Equal to sb3_evaluate (tests/test_eval_cpu.py)."""
    T, n_envs = reward.shape
    max_steps = T if max_steps is None else min(T, max_steps)
    targets = np.asarray(targets, dtype="int")
    counts = np.zeros(n_envs, dtype="int")
    cur = np.zeros(n_envs)
    raw = np.zeros(n_envs)
    length = np.zeros(n_envs, dtype="int")
    out = dict(episode_rewards=[], episode_lengths=[], env=[], step=[], return_raw=[], complete=[])
    t = 0
    while (counts < targets).any() and t < max_steps:
        cur += reward[t].astype(np.float32)
        raw += reward[t]
        length += 1
        d = done[t].astype(bool)
        idx = np.nonzero(d & (counts < targets))[0]
        out["episode_rewards"] += list(cur[idx]); out["episode_lengths"] += list(length[idx])
        out["env"] += idx.tolist(); out["step"] += [t] * len(idx); out["return_raw"] += list(raw[idx])
        out["complete"] += [bool(c) for c in complete[t, idx]]
        counts[idx] += 1
        cur[d] = 0; raw[d] = 0; length[d] = 0
        t += 1
    return dict(out, steps=t, finished=bool((counts >= targets).all()))
