"""CPU: the host half of ``DeviceEvalCallback`` (reinforcementlearning4meshgeneration_amd/eval_callback.py) against the
restatements of tests/eval_callback_ref.py: the evaluation schedule against SB3's loop stepped one vector step at a time, the
restated reduce order against np.mean / np.std within the bound of any summation order, the gate (strict, NaN, tie), the
snapshot sets, every refusal in front of any library call, and the packaging."""
import os
import re
import types

import numpy as np
import pytest

import eval_callback_ref as ER
import on_policy_stubs
import rl_stubs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _E():
    from reinforcementlearning4meshgeneration_amd import eval_callback
    return eval_callback


# ----------------------------------------------------------------------------------------------------------- 1. the schedule
N_ENVS, T = 33, 3


@pytest.mark.parametrize("learning_starts", [0, 50])
@pytest.mark.parametrize("eval_freq", [1, 3, T, T + 1, 5 * T])
def test_schedule_is_sb3s_one_vector_step_at_a_time_across_two_learns(eval_freq, learning_starts):
    """learning_starts moves the warm-up split of a collect, never the callback: SB3 calls on_step after every vector step,
    warm-up or not, so the same evaluations precede the same collects with the same stamps."""
    E = _E()
    from reinforcementlearning4meshgeneration_amd import offpolicy_learn as L
    n_calls = num = 0
    ref_calls = ref_num = 0
    for total in (7 * T * N_ENVS - 5, 4 * T * N_ENVS):             # two consecutive learn() calls; the first overshoots its total
        want, ref_calls, ref_after = ER.sb3_eval_schedule(ref_calls, ref_num, ref_num + total, N_ENVS, T, eval_freq)
        got, after_calls = E.schedule(n_calls, num, num + total, N_ENVS, T, eval_freq)
        assert got == want and after_calls == ref_calls
        # the collects are learn()'s own: one per plan() entry, and the callback's per-collect walk gives the same list
        plan = L.plan(num, num + total, N_ENVS, T, learning_starts, 1)
        walked, calls, at = [], n_calls, num
        for i, (_, _, after, _) in enumerate(plan):
            walked += [(i, calls + j, at + j * N_ENVS) for j in E.eval_points(calls, T, eval_freq)]
            calls, at = calls + T, after
        assert walked == want and at == ref_after
        assert all(stamp == c * N_ENVS for _, c, stamp in want)     # start 0: num_timesteps = n_calls * n_envs
        n_calls, num, ref_num = after_calls, at, ref_after
    assert n_calls == 11 * T and num == 11 * T * N_ENVS              # 7 collects (the last overshoots) + 4: n_calls went on across the calls


def test_eval_points_inside_on_and_past_a_collect():
    E = _E()
    assert E.eval_points(0, 3, 1) == [1, 2, 3] and E.eval_points(0, 3, 3) == [3] and E.eval_points(0, 3, 4) == []
    assert E.eval_points(3, 3, 4) == [1] and E.eval_points(2, 3, 15) == [] and E.eval_points(12, 3, 15) == [3]
    assert E.eval_points(5, 4, 2) == [1, 3]


# ----------------------------------------------------------------------------------------------------------- 2. the reduce order
@pytest.mark.parametrize("k", [1, 2, 63, 64, 65, 1000])
def test_restated_order_against_numpy_within_the_bound_of_any_order(k):
    """Two sums of the same k float64 numbers in different orders, each divided by k, differ by at most k * 2^-52 * max|x|: the
    bound of any summation order.  The variance is held to the same bound over the squared deviations, and std = sqrt of it."""
    rng = np.random.default_rng(k)
    n = max(k // 3, 1) + 70                                          # more envs than lanes: lanes walk several envs
    counts = np.zeros(n, np.int32)
    for _ in range(k):
        counts[rng.integers(n)] += 1
    targets = counts + rng.integers(0, 2, n).astype(np.int32)      # some slots stay unrecorded
    b = ER.tally_buffers(targets, counts, seed=100 + k)
    lanes = ER.recorded_slots(b["target"], b["offset"], b["count"])
    slots = np.array(sorted(s for lane in lanes for s in lane))
    x = b["ep_return"][slots]
    assert len(x) == k and np.isfinite(x).all() and (k < 63 or ((x > 0).any() and (x < 0).any()))
    mean, var = ER.mean_var(b["ep_return"], lanes)
    eps = 2.0 ** -52
    assert abs(mean - np.mean(x)) <= k * eps * np.abs(x).max()
    d2 = np.abs(x - np.mean(x)) ** 2                                  # np.std: sqrt(mean(abs(x - mean) ** 2))
    assert abs(var - np.mean(d2)) <= k * eps * d2.max()
    std = ER.mean_std(b["ep_return"], lanes)[1]
    assert std == np.sqrt(var) and abs(std - np.std(x)) <= k * eps * np.sqrt(d2.max())
    row, improved = ER.reduce_row(**b, short=3, num_timesteps=99, best_mean=-np.inf)
    assert improved and row[0] == 99 and row[4] == k and row[5] == 3 and row[8] == 1.0
    assert row[3] == np.mean(b["ep_length"][slots]) and row[6] == np.mean(b["ep_flags"][slots] & 1)
    assert row[7] == np.mean(b["ep_n_elem"][slots])


def test_nothing_recorded_is_nan_and_never_improves_and_a_tie_does_not_improve():
    b = ER.tally_buffers([0, 2, 1, 0], [0, 0, 0, 0], seed=1)
    row, improved = ER.reduce_row(**b, short=2, num_timesteps=5, best_mean=-np.inf)
    assert not improved and row[8] == 0.0 and row[4] == 0
    assert all(ER.bits(row[c])[()] == 0x7FF8000000000000 for c in (1, 2, 3, 6, 7))
    ref = ER.CallbackRef()
    one = ER.tally_buffers([1], [1], seed=2)
    r0, i0 = ref.add(**one, short=0, num_timesteps=1)
    r1, i1 = ref.add(**one, short=0, num_timesteps=2)                 # the same mean again: a tie
    assert i0 and not i1 and ref.best_eval == 0 and r0[1] == r1[1] == ref.best_mean
    _, i2 = ref.add(**b, short=2, num_timesteps=3)                    # NaN after a best
    assert not i2 and ref.best_eval == 0 and ER.bits(ref.last_mean)[()] == 0x7FF8000000000000
    better = dict(one, ep_return=one["ep_return"] + 1.0)
    assert ref.add(**better, short=0, num_timesteps=4)[1] and ref.best_eval == 3
    assert ref.history().shape == (4, 9) and list(ref.state()[[1, 3]]) == [3.0, 4.0]
    # without an element log every n_elements is -1: the mean element count is NaN, the rest is not
    row, _ = ER.reduce_row(**ER.tally_buffers([2, 1], [2, 1], seed=3, log=False), short=0, num_timesteps=0, best_mean=-np.inf)
    assert np.isnan(row[7]) and np.isfinite(row[[1, 2, 3, 6]]).all()


def test_holes_are_never_read():
    a = ER.tally_buffers([2, 0, 3, 1] * 20, [1, 0, 3, 0] * 20, seed=4, nan_holes=True)
    b = ER.tally_buffers([2, 0, 3, 1] * 20, [1, 0, 3, 0] * 20, seed=4, nan_holes=False)
    ra, _ = ER.reduce_row(**a, short=1, num_timesteps=0, best_mean=0.0)
    rb, _ = ER.reduce_row(**b, short=1, num_timesteps=0, best_mean=0.0)
    assert np.array_equal(ER.bits(ra), ER.bits(rb)) and np.isfinite(ra).all() and ra[4] == 80


# ----------------------------------------------------------------------------------------------------------- 3. snapshot sets
def test_snapshot_sets_are_the_live_tensors():
    E = _E()
    sac = rl_stubs.sac_model()
    kind, named = E.snapshot_set(sac)
    assert kind == "sac" and len(named) == 10 + 4 * 8 + 1 and len({k for k, _ in named}) == len(named)
    d = dict(named)
    assert d["actor.0.weight"] is sac.actor.latent_pi[0].weight and d["actor.4.bias"] is sac.actor.log_std.bias
    assert d["critic.q1.3.weight"] is sac.critic.q_networks[1][6].weight
    assert d["critic_target.q0.0.bias"] is sac.critic_target.q_networks[0][0].bias and d["log_ent_coef"] is sac.log_ent_coef
    assert "log_ent_coef" not in dict(E.snapshot_set(rl_stubs.sac_model(learned=False))[1])
    td3 = rl_stubs.td3_model()
    kind, named = E.snapshot_set(td3)
    assert kind == "td3" and len(named) == 6 + 6 + 4 * 6
    d = dict(named)
    assert d["actor.2.weight"] is td3.actor.mu[4].weight and d["actor_target.0.weight"] is td3.actor_target.mu[0].weight
    for k in ("ppo", "a2c"):
        model, params = on_policy_stubs.model(k)
        kind, named = E.snapshot_set(model)
        assert kind == "ac" and [k for k, _ in named] == list(E.AC_NAMES) and all(a is b for (_, a), b in zip(named, params))
    offsets, floats = E.best_layout([("a", types.SimpleNamespace(numel=lambda: 1)), ("b", types.SimpleNamespace(numel=lambda: 3)),
                                     ("c", types.SimpleNamespace(numel=lambda: 2304)), ("d", types.SimpleNamespace(numel=lambda: 5))])
    assert offsets == [0, 4, 8, 2312] and floats == 2320
    with pytest.raises(ValueError, match="hidden layers"):
        E.snapshot_set(rl_stubs.sac_model(H=64))
    with pytest.raises(ValueError, match="n_critics"):
        E.snapshot_set(rl_stubs.td3_model(n_critics=1))


# ----------------------------------------------------------------------------------------------------------- 4. refusals
def _venv(device="cpu", n=33):
    import torch
    return types.SimpleNamespace(num_envs=n, device=torch.device(device), evaluate=lambda *a, **k: None)


def test_every_refusal_comes_before_any_library_call(monkeypatch):
    import torch
    from reinforcementlearning4meshgeneration_amd import _capi, actor, policy
    E = _E()

    def no_library(*a, **k):
        raise AssertionError("the library was loaded before the refusal")
    monkeypatch.setattr(_capi, "load", no_library)
    sac, venv = rl_stubs.sac_model(), _venv()
    for kw, msg in ((dict(eval_freq=0), "eval_freq must be an int >= 1"), (dict(eval_freq=2.5), "eval_freq must be an int >= 1"),
                    (dict(eval_freq=True), "eval_freq must be an int >= 1"), (dict(eval_steps=0), "eval_steps must be an int >= 1"),
                    (dict(eval_steps=-4), "eval_steps must be an int >= 1"), (dict(capacity=0), "capacity must be an int >= 1"),
                    (dict(n_eval_episodes=5, episodes_per_env=1), "not both"), (dict(n_eval_episodes=-1), "non-negative integer")):
        with pytest.raises(ValueError, match=msg):
            E.DeviceEvalCallback(venv, sac, **kw)
    with pytest.raises(TypeError, match="eval_venv must be a MeshVecEnv"):
        E.DeviceEvalCallback(object(), sac)
    with pytest.raises(ValueError, match=r"is on cpu; DeviceEvalCallback \(the eval env's device\) binds"):
        E.DeviceEvalCallback(_venv("cuda:0"), sac)                    # an eval env on another device than the model
    with pytest.raises(ValueError, match="hidden layers"):
        E.DeviceEvalCallback(venv, rl_stubs.sac_model(H=64))
    # a policy kind that does not fit the model
    fa = actor.FusedActor.__new__(actor.FusedActor)
    det = policy.FusedPolicy.__new__(policy.FusedPolicy)
    det.spec = policy.PolicySpec.from_sb3(rl_stubs.td3_model(), sigma=0.1)
    ac = policy.FusedPolicy.__new__(policy.FusedPolicy)
    ac.spec = policy.PolicySpec.from_sb3(on_policy_stubs.model("ppo")[0])
    for kind, good in (("sac", fa), ("td3", det), ("ac", ac)):
        E.check_policy(kind, good)
        for bad in (fa, det, ac, object()):
            if bad is not good:
                with pytest.raises(ValueError, match="the model is evaluated through"):
                    E.check_policy(kind, bad)
    with pytest.raises(ValueError, match=r"evaluated through a FusedActor \(SAC\), got FusedPolicy"):
        E.DeviceEvalCallback(venv, sac, behaviour=det)
    fa.device = torch.device("cuda", 0)
    with pytest.raises(ValueError, match="behaviour is on cuda:0, the eval envs on cpu"):
        E.DeviceEvalCallback(venv, sac, behaviour=fa)


def test_evaluate_now_and_learn_refuse_on_the_host(monkeypatch):
    import torch
    from reinforcementlearning4meshgeneration_amd import _capi, offpolicy_learn, policy
    E = _E()
    cb = E.DeviceEvalCallback.__new__(E.DeviceEvalCallback)           # no device: the checks in front of the C calls
    cb.kind, cb.capacity, cb.evaluations, cb.eval_freq, cb.n_calls = "sac", 2, 2, 3, 0
    cb.device = torch.device("cpu")
    monkeypatch.setattr(_capi, "load", lambda: (_ for _ in ()).throw(AssertionError("library call")))
    with pytest.raises(ValueError, match="2 evaluations made and 1 more asked for; capacity = 2"):
        cb.evaluate_now(object(), 0)
    cb.evaluations = 0
    det = policy.FusedPolicy.__new__(policy.FusedPolicy)
    det.spec = policy.PolicySpec.from_sb3(rl_stubs.td3_model(), sigma=0.1)
    with pytest.raises(ValueError, match="evaluated through a FusedActor"):
        cb.evaluate_now(det, 0)
    # learn(callback=...): the training env itself, another device, another model, a schedule past the capacity
    learn = offpolicy_learn.FusedOffPolicyLearn.__new__(offpolicy_learn.FusedOffPolicyLearn)
    learn.venv, learn.model = _venv(), object()
    with pytest.raises(TypeError, match="callback must be a DeviceEvalCallback"):
        learn._check_callback(object(), 0, 99, 33, 3)
    cb.eval_venv, cb.model = learn.venv, learn.model
    with pytest.raises(ValueError, match="is the training env"):
        learn._check_callback(cb, 0, 99, 33, 3)
    cb.eval_venv = _venv("cuda:0")
    with pytest.raises(ValueError, match="eval envs are on cuda:0, the training envs on cpu"):
        learn._check_callback(cb, 0, 99, 33, 3)
    cb.eval_venv, cb.model = _venv(), object()
    with pytest.raises(ValueError, match="another model"):
        learn._check_callback(cb, 0, 99, 33, 3)
    cb.model = learn.model
    learn._check_callback(cb, 0, 2 * 99, 33, 3)                        # two collects, eval_freq 3: two evaluations fit the capacity
    assert cb.evaluations == 0 and cb.n_calls == 0                    # (checked only; nothing was enqueued or counted)


def test_learn_refuses_a_schedule_past_the_capacity():
    from reinforcementlearning4meshgeneration_amd import offpolicy_learn
    E = _E()
    cb = E.DeviceEvalCallback.__new__(E.DeviceEvalCallback)
    cb.capacity, cb.evaluations, cb.eval_freq, cb.n_calls = 2, 0, 3, 0
    learn = offpolicy_learn.FusedOffPolicyLearn.__new__(offpolicy_learn.FusedOffPolicyLearn)
    learn.venv, learn.model = _venv(), object()
    cb.eval_venv, cb.model = _venv(), learn.model
    learn._check_callback(cb, 0, 2 * 99, 33, 3)                        # two collects of three steps: two evaluations fit
    with pytest.raises(ValueError, match="0 evaluations made and 3 more asked for; capacity = 2"):
        learn._check_callback(cb, 0, 3 * 99, 33, 3)


# ----------------------------------------------------------------------------------------------------------- 5. packaging
def test_exports_declarations_and_header():
    import reinforcementlearning4meshgeneration_amd as pkg
    from reinforcementlearning4meshgeneration_amd import _capi
    E = _E()
    assert "DeviceEvalCallback" in pkg.__all__ and pkg.DeviceEvalCallback is E.DeviceEvalCallback
    assert E.DeviceEvalCallback.PREFIX == "meshenv_eval_callback" and issubclass(E.DeviceEvalCallback, pkg._handle.Handle)
    names = _capi.EXPORTS_EVAL_CALLBACK
    assert len(names) == len(set(names)) == 7
    header = open(os.path.join(ROOT, "include", "meshenv_eval_callback.h")).read()
    defines = dict(re.findall(r"#define\s+(MESHENV_[A-Z_]+)\s+(\d+)", header))
    assert int(defines["MESHENV_EVAL_ROW_DOUBLES"]) == _capi.EVAL_ROW_DOUBLES == len(_capi.EVAL_COLUMNS) == len(ER.COLUMNS) == 9
    assert _capi.EVAL_COLUMNS == ER.COLUMNS
    assert int(defines["MESHENV_EVAL_STATE_DOUBLES"]) == _capi.EVAL_STATE_DOUBLES == 4
    assert int(defines["MESHENV_KEEP_BEST_MAX_ENTRIES"]) == _capi.KEEP_BEST_MAX_ENTRIES == 64
    kernels = open(os.path.join(ROOT, "reinforcementlearning4meshgeneration_amd", "csrc", "meshenv_eval_callback.h")).read()
    assert "k_eval_reduce" in kernels and "k_keep_best" in kernels
    host = open(os.path.join(ROOT, "reinforcementlearning4meshgeneration_amd", "csrc", "meshenv_hip.hip")).read()
    queued = host[host.index("int meshenv_evaluate_queued("):host.index("int meshenv_eval_callback_create(")]
    assert "eval_read_short" not in queued and "eval_host" not in queued and "Synchronize" not in queued and "hipMemcpy" not in queued
    lib = _capi.load()
    assert lib.meshenv_evaluate_queued.argtypes is not None and lib.meshenv_keep_best.restype is not None
    import ctypes
    assert ctypes.sizeof(_capi.MeshKeepEntry) == 24
    import inspect
    from reinforcementlearning4meshgeneration_amd import offpolicy_learn
    assert inspect.signature(offpolicy_learn.FusedOffPolicyLearn.learn).parameters["callback"].default is None
