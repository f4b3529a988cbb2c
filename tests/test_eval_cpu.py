"""CPU: the device layout of policy evaluation (per-env slots + the step index, sorted afterwards) equals SB3's
evaluate_policy loop bit for bit on recorded streams; EvalResult's ordering, summaries and quality report; the argument
checks of evaluate_policy / episode_targets that run before any launch."""
import numpy as np
import pytest

import eval_ref as R
from reinforcementlearning4meshgeneration_amd.evaluation import EvalResult, episode_targets, evaluate_policy


def _same(a, b):
    for k in ("episode_rewards", "episode_lengths", "env", "step", "return_raw", "complete"):
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.shape == y.shape, k
        if x.dtype.kind == "f":
            assert np.array_equal(x.view(np.int64), y.astype(np.float64).view(np.int64)), k
        else:
            assert np.array_equal(x, y), k
    assert a["steps"] == b["steps"] and a["finished"] == b["finished"]


CASES = [   # (T, n, n_eval_episodes, max_steps, burst)
    (200, 8, 3, None, None),       # below n_envs: targets of 0
    (200, 8, 8, None, None),       # equal
    (400, 8, 21, None, None),      # not a multiple
    (300, 16, 40, None, 5),        # every env done at the same step
    (300, 16, 64, 60, None),       # max_steps cut
    (50, 4, 0, None, None),        # nothing to record
]


@pytest.mark.parametrize("T,n,n_eval,max_steps,burst", CASES)
def test_device_layout_equals_sb3_loop(T, n, n_eval, max_steps, burst):
    for seed in range(3):
        reward, done, complete = R.synthetic(T, n, seed=seed, p_done=0.08, burst=burst)
        targets = R.sb3_targets(n_eval, n)
        a = R.sb3_evaluate(reward, done, complete, targets, max_steps)
        b = R.device_layout(reward, done, complete, targets, max_steps)
        _same(a, b)
        assert len(a["episode_rewards"]) <= n_eval
        if max_steps is not None:
            assert not a["finished"] and a["steps"] == max_steps
        if burst is not None:
            assert len(set(zip(a["step"], a["env"]))) == len(a["step"]) and a["step"].count(burst) > 1


def test_float32_rounding_of_the_return_is_sb3s():
    reward = np.array([[0.1], [0.2], [1e-9]], np.float64)
    done = np.array([[0], [0], [1]], np.uint8)
    a = R.sb3_evaluate(reward, done, done, [1])
    assert a["episode_rewards"][0] == np.float64(np.float32(0.1)) + np.float64(np.float32(0.2)) + np.float64(np.float32(1e-9))
    assert a["episode_rewards"][0] != a["return_raw"][0]


def test_episode_targets():
    assert episode_targets(4, 10).tolist() == [2, 2, 3, 3] == R.sb3_targets(10, 4).tolist()
    assert episode_targets(4, 3).tolist() == [0, 1, 1, 1]
    assert episode_targets(3).tolist() == [1, 1, 1]
    assert episode_targets(3, episodes_per_env=2).tolist() == [2, 2, 2]
    assert episode_targets(3, episodes_per_env=np.array([0, 5, 1])).tolist() == [0, 5, 1]
    for bad in (dict(n_eval_episodes=-1), dict(n_eval_episodes=2.5), dict(episodes_per_env=-1),
                dict(episodes_per_env=[1, 2]), dict(episodes_per_env=np.array([1.0, 2.0, 3.0])),
                dict(n_eval_episodes=3, episodes_per_env=1)):
        with pytest.raises(ValueError):
            episode_targets(3, **bad)


def _records(seed=0):
    rng = np.random.default_rng(seed)
    N = 12
    rec = {"env": rng.integers(0, 5, N), "step": rng.integers(0, 4, N), "domain": rng.integers(0, 2, N),
           "length": rng.integers(1, 50, N), "return": rng.normal(size=N), "return_raw": rng.normal(size=N),
           "flags": rng.integers(0, 4, N), "n_elements": rng.integers(0, 30, N), "archive": rng.integers(0, 3, N),
           "quality": rng.normal(size=(N, 8, 4))}
    rec["n_elements"][:3] = 0
    return rec


def test_eval_result_order_and_summaries():
    rec = _records()
    res = EvalResult.from_records(rec, targets=np.ones(5, np.int32), steps=4, finished=True)
    order = sorted(range(len(rec["env"])), key=lambda i: (rec["step"][i], rec["env"][i]))
    assert res.env.tolist() == [int(rec["env"][i]) for i in order]
    assert res.step.tolist() == [int(rec["step"][i]) for i in order]
    assert res.episode_rewards == [float(rec["return"][i]) for i in order]
    assert res.mean_reward == float(np.mean(res.reward)) and res.std_reward == float(np.std(res.reward))
    assert res.complete.tolist() == [bool(rec["flags"][i] & 1) for i in order]
    assert res.overflow.tolist() == [bool(rec["flags"][i] & 2) for i in order]
    assert np.array_equal(res.quality, rec["quality"][order])
    whole = res.summary(by=None)
    assert whole == {"completed": [int(c) for c in res.complete], "n_elements": [int(x) for x in res.n_elements]}
    per = res.summary(by="domain")
    assert sorted(per) == sorted(set(int(d) for d in rec["domain"]))
    assert sum(len(v["completed"]) for v in per.values()) == len(res)
    for d, v in per.items():
        assert v["n_elements"] == [int(x) for x, dd in zip(res.n_elements, res.domain) if dd == d]
    assert sum(len(v["completed"]) for v in res.summary(by="env").values()) == len(res)
    with pytest.raises(ValueError):
        res.summary(by="step")


def test_eval_result_quality_report():
    res = EvalResult.from_records(_records(1), targets=np.ones(5, np.int32), steps=4, finished=True)
    rep = res.quality_report()
    live = res.n_elements > 0
    assert rep["meshes"] == int(live.sum()) and rep["elements"] == int(res.n_elements[live].sum())
    st = res.quality[live, 2]
    assert rep["scaled_jacobian"] == dict(average=float(st[:, 1].mean()), std=float(np.sqrt(np.abs(st[:, 3])).mean()),
                                          min=float(st[:, 0].min()), max=float(st[:, 2].max()))
    empty = EvalResult.from_records({k: v[:0] for k, v in _records().items()}, np.zeros(2, np.int32), 0, True)
    assert len(empty) == 0 and np.isnan(empty.mean_reward) and empty.summary(by=None) == {"completed": [], "n_elements": []}


def test_evaluate_policy_refuses_host_hooks():
    with pytest.raises(ValueError, match="callback"):
        evaluate_policy(object(), object(), callback=lambda *a: None)
    with pytest.raises(ValueError, match="render"):
        evaluate_policy(object(), object(), render=True)
    with pytest.raises(TypeError, match="MeshVecEnv"):
        evaluate_policy(object(), object())


@pytest.mark.parametrize("T,n,n_eval,max_steps,burst", CASES)
def test_vectorised_transcription_equals_the_loop(T, n, n_eval, max_steps, burst):
    reward, done, complete = R.synthetic(T, n, seed=7, p_done=0.08, burst=burst)
    targets = R.sb3_targets(n_eval, n)
    _same(R.sb3_evaluate(reward, done, complete, targets, max_steps), R.sb3_evaluate_fast(reward, done, complete, targets, max_steps))
