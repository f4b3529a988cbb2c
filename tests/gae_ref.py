"""Host restatement of meshenv_gae (csrc/meshenv_gae.h) in numpy float32: SB3's RolloutBuffer.compute_returns_and_advantage
(GAE, SB3 2.x) with the TimeLimit.truncated bootstrap of collect_rollouts in front, evaluated in the order SB3's numpy code and
examples/ppo_rollout.py::gae evaluate it.  numpy 2 rounds a Python-float scalar to float32 before an elementwise op with a
float32 array, as torch does, so this is the float32 loop the kernel must match bit for bit.

Also the seeded synthetic histories the CPU and GPU tests share, and the example's torch loop loaded from its file."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def gae_ref(reward, value, done, last_value, terminal_value=None, gamma=0.99, gae_lambda=0.95):
    """reward [T, n] float64, value [T, n] float32, done [T, n] uint8, last_value [n] float32, terminal_value [T, n]
    float32 or None -> dict(advantages, returns, rewards) [T, n] float32."""
    g = np.float32(gamma)
    gl = np.float32(gamma * gae_lambda)
    T, n = reward.shape
    adv = np.empty((T, n), np.float32)
    ret = np.empty((T, n), np.float32)
    rew = np.empty((T, n), np.float32)
    last = np.zeros(n, np.float32)
    with np.errstate(all="ignore"):
        for t in reversed(range(T)):
            r = reward[t].astype(np.float32)
            if terminal_value is not None:
                r = r + g * terminal_value[t]
            nnt = np.float32(1.0) - (done[t] != 0).astype(np.float32)
            next_v = last_value if t == T - 1 else value[t + 1]
            delta = (r + (g * next_v) * nnt) - value[t]
            last = delta + (gl * nnt) * last
            adv[t] = last
            ret[t] = last + value[t]
            rew[t] = r
    return dict(advantages=adv, returns=ret, rewards=rew)


def synthetic(T, n, seed, with_terminal=True, special=True):
    """Seeded histories shaped like collect_rollout's: float64 rewards with full mantissas, ~5 % done, terminal values only
    where done and not complete.  With special (and n >= 3): env 1 holds subnormal values and rewards, env 2 a NaN value and
    an inf reward."""
    rng = np.random.default_rng(seed)
    reward = rng.standard_normal((T, n)) * rng.uniform(0.1, 20.0, (T, n))
    value = (rng.standard_normal((T, n)) * 5.0).astype(np.float32)
    done = (rng.random((T, n)) < 0.05).astype(np.uint8)
    complete = done & (rng.random((T, n)) < 0.5).astype(np.uint8)
    last_value = (rng.standard_normal(n) * 5.0).astype(np.float32)
    tv = None
    if with_terminal:
        tv = np.where((done != 0) & (complete == 0), rng.standard_normal((T, n)) * 5.0, 0.0).astype(np.float32)
    if special and n >= 3:
        tiny = np.float32(1e-39)   # f32 subnormal
        value[:, 1] = tiny * rng.uniform(-1.0, 1.0, T).astype(np.float32)
        reward[:, 1] = rng.uniform(-1.0, 1.0, T) * 1e-39
        last_value[1] = tiny
        done[:, 1] = 0
        if tv is not None:
            tv[:, 1] = 0.0
        value[T // 2, 2] = np.nan
        reward[(T - 1) // 3, 2] = np.inf
    return dict(reward=reward, value=value, done=done, complete=complete, last_value=last_value, terminal_value=tv)


def example_gae():
    """examples/ppo_rollout.py::gae (the torch loop the device path replaces)."""
    spec = importlib.util.spec_from_file_location("ppo_rollout_example", os.path.join(ROOT, "examples", "ppo_rollout.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.gae


def same_bits(a, b):
    """float32 arrays equal bit for bit, except that NaNs are compared by position only (payloads may differ)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    if not np.array_equal(na, nb):
        return False
    return np.array_equal(a.view(np.int32)[~na], b.view(np.int32)[~nb])
