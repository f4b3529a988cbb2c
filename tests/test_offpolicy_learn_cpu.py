"""CPU: the host half of ``FusedOffPolicyLearn`` / ``EpisodeStats`` (reinforcementlearning4meshgeneration_amd/offpolicy_learn.py)
against the restatements of tests/offpolicy_learn_ref.py: the warm-up split and the train gate against SB3's loop stepped one env
step at a time, the uniform draw's range and counter carry, the episode statistics' summation order, (t, env) order, ring wrap
and carry across calls, every refusal, and the packaging."""
import os
import re
import types

import numpy as np
import pytest

import offpolicy_learn_ref as LR
import policy_ref
import rl_stubs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOW = np.array([-1.0, -1.5, 0.0], np.float32)
HIGH = np.array([1.0, 1.5, 1.5], np.float32)


def _L():
    from reinforcementlearning4meshgeneration_amd import offpolicy_learn
    return offpolicy_learn


# ----------------------------------------------------------------------------------------------------------- 1. the schedule
@pytest.mark.parametrize("num,n,T,ls,want", [
    (0, 33, 3, 50, 2),          # strictly inside: steps at 0 and 33 are below 50, the one at 66 is not
    (0, 33, 3, 0, 0),           # learning_starts = 0: no warm-up
    (0, 33, 3, 1000, 3),        # all of the collect
    (0, 33, 3, 66, 2),          # the step AT learning_starts is a policy step (<, not <=)
    (0, 33, 3, 67, 3),
    (99, 33, 3, 100, 1),
    (99, 33, 3, 99, 0),
    (0, 1, 5, 3, 3),
    (0, 4096, 32, 10000, 3),    # the reference's learning_starts at the bench's env count
])
def test_warmup_split_is_the_prefix_sb3_would_sample_uniformly(num, n, T, ls, want):
    L = _L()
    assert L.warmup_split(num, n, T, ls) == want
    flags = LR.sb3_schedule(num, num + 1, n, T, ls, 1)[0][0]
    assert flags == [True] * want + [False] * (T - want)       # a prefix, of that length


def test_train_gate_is_strictly_past_learning_starts():
    L = _L()
    assert not L.should_train(99, 99) and L.should_train(100, 99) and not L.should_train(0, 0) and L.should_train(1, 0)
    # n = 33, T = 3: after the first collect num_timesteps = 99
    assert L.plan(0, 99, 33, 3, 99, 2) == [(3, 0, 99, 0)]
    assert L.plan(0, 99, 33, 3, 98, 2) == [(3, 0, 99, 2)]


def test_gradient_steps_minus_one_is_the_collect_length():
    L = _L()
    assert L.resolve_gradient_steps(-1, 7) == 7 and L.resolve_gradient_steps(3, 7) == 3 and L.resolve_gradient_steps(0, 7) == 0
    assert [k for _, _, _, k in L.plan(0, 20, 2, 5, 0, -1)] == [5, 5]
    with pytest.raises(ValueError, match="gradient_steps must be an int"):
        L.resolve_gradient_steps(1.5, 7)


@pytest.mark.parametrize("num,total,n,T,ls,gs", [(0, 297, 33, 3, 50, 2), (0, 100, 33, 3, 50, 2), (0, 1, 33, 3, 0, -1),
                                                  (198, 198 + 297, 33, 3, 50, 2), (0, 50, 4, 2, 1000, 1), (0, 0, 4, 2, 0, 1),
                                                  (0, 64, 8, 4, 20, 3)])
def test_plan_is_sb3s_loop_overshoot_included(num, total, n, T, ls, gs):
    L = _L()
    ref = LR.sb3_schedule(num, total, n, T, ls, gs)
    got = L.plan(num, total, n, T, ls, gs)
    assert [(W, P) for W, P, _, _ in got] == [(sum(f), T - sum(f)) for f, _, _ in ref]
    assert [(a, k) for _, _, a, k in got] == [(a, k) for _, a, k in ref]
    if got:
        last = got[-1][2]
        assert last >= total and last - T * n < total          # a collect is never cut short: SB3's overshoot
        assert (last - num) % (T * n) == 0
    else:
        assert num >= total


def test_issue_configuration_first_collect_is_two_warmup_steps_and_one_policy_step():
    L = _L()
    p = L.plan(0, 3 * 99, 33, 3, 50, 2)
    assert p[0] == (2, 1, 99, 2) and all(x[:2] == (0, 3) and x[3] == 2 for x in p[1:]) and len(p) == 3 and p[-1][2] == 297


def test_train_freq_forms():
    L = _L()
    assert L.parse_train_freq(3) == 3 and L.parse_train_freq((4, "step")) == 4
    unit = types.SimpleNamespace(value="step")
    assert L.parse_train_freq(types.SimpleNamespace(frequency=5, unit=unit)) == 5
    with pytest.raises(ValueError, match="episodes is not supported"):
        L.parse_train_freq((1, "episode"))
    with pytest.raises(ValueError, match="episodes is not supported"):
        L.parse_train_freq(types.SimpleNamespace(frequency=1, unit=types.SimpleNamespace(value="episode")))
    for bad in (0, -1, True, 2.0, (1, "minute"), (1, 2, 3)):
        with pytest.raises(ValueError):
            L.parse_train_freq(bad)


# ----------------------------------------------------------------------------------------------------------- 2. the uniform draw
def test_uniform_draw_range_and_box():
    a, b = LR.uniform_actions(7, 0, 64, 257, LOW, HIGH)
    assert a.dtype == np.float32 and b.dtype == np.float32 and a.shape == b.shape == (64, 257, 3)
    assert b.min() >= -1.0 and b.max() < 1.0
    assert (a >= LOW).all() and (a <= HIGH).all()
    assert abs(float(b.mean())) < 0.02 and 0.55 < float(b.std()) < 0.6      # uniform on [-1, 1): std 0.577
    # the extreme words: u = 0 and u = 1 - 2^-24 stay inside, and the maps are exact
    for w, want in ((0, -1.0), (0xFFFFFFFF, 1.0 - 2.0 ** -23)):
        u = np.float32(np.uint32(w) >> np.uint32(8)) * np.float32(2.0 ** -24)
        assert float(np.float32(2.0) * u - np.float32(1.0)) == want
    assert float(LR.unscale_action(np.float32(1.0 - 2.0 ** -23), LOW, HIGH)[1]) <= 1.5
    # the + 0.5f map of philox_normal is NOT the one used: it can round to 1
    assert float((np.float32(0xFFFFFF) + np.float32(0.5)) * np.float32(2.0 ** -24)) == 1.0


def test_uniform_draw_stream_is_its_own_and_the_counter_carries():
    n = 5
    w = LR.uniform_words(3, 2 ** 32 - 1, 3, n)
    env = np.arange(n, dtype=np.uint64)
    for t, (lo, hi) in enumerate(((0xFFFFFFFF, 0), (0, 1), (1, 1))):            # the sum carries into the high word
        ref = policy_ref.philox4x32(env, lo, hi, 4, 3, 0)
        assert all(np.array_equal(w[t, :, k], ref[k]) for k in range(3))
    no_carry = policy_ref.philox4x32(env, 0, 0, 4, 3, 0)
    assert not np.array_equal(w[1, :, 0], no_carry[0])
    for tag in (0, 1, 2, 3):                                                     # the tags that are taken
        other = policy_ref.philox4x32(env, 0xFFFFFFFF, 0, tag, 3, 0)
        assert not np.array_equal(w[0, :, 0], other[0])
    assert np.array_equal(LR.uniform_words(3, 2 ** 64 - 1, 2, n)[1], LR.uniform_words(3, 0, 1, n)[0])   # modulo 2^64
    from reinforcementlearning4meshgeneration_amd import _capi
    assert _capi.UNIFORM_PHILOX_TAG == LR.UNIFORM_TAG == 4
    # the unscale expression is k_policy_forward's: policy_ref restates it in float64 with a bound
    s = np.linspace(-1, 1, 11).astype(np.float32)
    mid, err = policy_ref._rescale(s.astype(np.float64)[:, None], 0.0, LOW, HIGH)
    assert (np.abs(LR.unscale_action(s[:, None], LOW, HIGH).astype(np.float64) - mid) <= err).all()


# ----------------------------------------------------------------------------------------------------------- 3. episode statistics
def test_monitor_return_is_the_sequential_float64_sum():
    rewards = np.array([1e16, 1.0, -1e16, 1.0, 3.0])
    m = LR.MonitorRef(1, window=4)
    done = np.zeros((5, 1), np.uint8)
    done[4, 0] = 1
    m.update(rewards.reshape(5, 1), done, done)
    want = 0.0
    for r in rewards:
        want += r
    assert m.buffer[0] == (want, 5.0, 1.0) and want == 4.0
    assert float(((rewards[0] + rewards[2]) + rewards[1]) + rewards[3] + rewards[4]) == 5.0        # another order, another value


def test_monitor_order_is_step_then_env_and_the_other_order_fails():
    reward, done, complete = LR.synthetic_history(3, 33, 5)
    assert done.sum() > 4 and (done.sum(axis=1) > 1).any() and (done.sum(axis=0) > 1).any()
    good, bad = LR.MonitorRef(33, window=4), LR.MonitorRef(33, window=4, order="env_t")
    good.update(reward, done, complete)
    bad.update(reward, done, complete)
    # by hand: flat index ascending
    eps, acc, ln = [], np.zeros(33), np.zeros(33, int)
    for t in range(3):
        for e in range(33):
            acc[e] += reward[t, e]
            ln[e] += 1
            if done[t, e]:
                eps.append((acc[e], float(ln[e]), float(complete[t, e])))
                acc[e], ln[e] = 0.0, 0
    assert list(good.buffer) == eps[-4:] and good.count == len(eps)
    assert list(bad.buffer) != list(good.buffer) and not np.array_equal(bad.ring(), good.ring())


def test_monitor_ring_wrap_and_carry_across_calls():
    reward, done, complete = LR.synthetic_history(12, 3, 11, p_done=0.25)
    done[5:7] = 0                                                  # an episode spans the call boundary at 6
    complete &= done
    whole, parts = LR.MonitorRef(3, window=4), LR.MonitorRef(3, window=4)
    whole.update(reward, done, complete)
    for a, b in ((0, 6), (6, 7), (7, 12)):
        parts.update(reward[a:b], done[a:b], complete[a:b])
    assert whole.count == parts.count > 4
    assert list(whole.buffer) == list(parts.buffer) and np.array_equal(whole.ring(), parts.ring())
    cr, cl = whole.carries()
    pr, pl = parts.carries()
    assert np.array_equal(cr, pr) and np.array_equal(cl, pl)
    L = _L()
    order = L.ring_order(whole.count, 4)
    assert [tuple(whole.ring()[s]) for s in order] == list(whole.buffer)        # deque order out of the ring
    assert L.ring_order(3, 4) == [0, 1, 2] and L.ring_order(4, 4) == [0, 1, 2, 3] and L.ring_order(6, 4) == [2, 3, 0, 1]
    logs = whole.logs()
    assert logs["rollout/ep_rew_mean"] == float(np.mean([e[0] for e in whole.buffer]))
    assert "rollout/ep_rew_mean" not in LR.MonitorRef(3).logs()


# ----------------------------------------------------------------------------------------------------------- 4. refusals, packaging
def _sac(**kw):
    m = rl_stubs.sac_model()
    m.learning_starts, m.train_freq, m.gradient_steps, m.batch_size, m.buffer_size = 50, 3, 2, 16, 1000
    for k, v in kw.items():
        setattr(m, k, v)
    return m


def test_spec_reads_the_model_and_refuses_by_name():
    L = _L()
    s = L.OffPolicyLearnSpec(_sac(), 33)
    assert s.sac and s.learning_starts == 50 and s.train_freq == 3 and s.gradient_steps == 2 and s.num_timesteps() == 0
    td3 = rl_stubs.td3_model()
    td3.learning_starts, td3.train_freq = 10, (2, "step")
    assert not L.OffPolicyLearnSpec(td3, 4).sac
    with pytest.raises(ValueError, match="use_sde=True"):
        L.OffPolicyLearnSpec(_sac(use_sde=True), 33)
    with pytest.raises(ValueError, match="use_sde_at_warmup=True"):
        L.OffPolicyLearnSpec(_sac(use_sde_at_warmup=True), 33)
    with pytest.raises(ValueError, match="episodes is not supported"):
        L.OffPolicyLearnSpec(_sac(train_freq=(1, "episode")), 33)
    with pytest.raises(ValueError, match="venv.auto_reset is off"):
        L.OffPolicyLearnSpec(_sac(), 33, auto_reset=False)
    with pytest.raises(ValueError, match="learning_starts must be an int >= 0"):
        L.OffPolicyLearnSpec(_sac(learning_starts=-1), 33)
    with pytest.raises(ValueError, match="has no train_freq"):
        m = _sac()
        del m.train_freq
        L.OffPolicyLearnSpec(m, 33)
    with pytest.raises(ValueError, match="action_noise with SAC"):
        L.OffPolicyLearnSpec(_sac(action_noise=object()), 33)
    with pytest.raises(ValueError, match="num_timesteps must be an int >= 0"):
        L.OffPolicyLearnSpec(_sac(num_timesteps=-3), 33).num_timesteps()


def test_from_sb3_refuses_before_any_device_is_touched():
    L = _L()
    venv = types.SimpleNamespace(num_envs=33, auto_reset=True)
    with pytest.raises(ValueError, match="not a DeviceReplayBuffer"):
        L.FusedOffPolicyLearn.from_sb3(_sac(), venv, replay_buffer=object())
    with pytest.raises(ValueError, match="use_sde=True"):
        L.FusedOffPolicyLearn.from_sb3(_sac(use_sde=True), venv)
    with pytest.raises(ValueError, match="venv.auto_reset is off"):
        L.FusedOffPolicyLearn.from_sb3(_sac(), types.SimpleNamespace(num_envs=33, auto_reset=False))
    import torch
    venv.device = torch.device("cuda", 0)                         # the stand-in's parameters are on the CPU
    with pytest.raises(ValueError, match="is on cpu; FusedOffPolicyLearn binds"):
        L.FusedOffPolicyLearn.from_sb3(_sac(), venv)


def test_action_noise_sigma():
    L = _L()
    m = rl_stubs.td3_model()
    assert L.noise_sigma(m, None) is None and L.noise_sigma(m, 0.1) == 0.1
    Normal = type("NormalActionNoise", (), {})
    noise = Normal()
    noise._mu, noise._sigma = np.zeros(3), np.full(3, 0.2)
    m.action_noise = noise
    assert np.array_equal(L.noise_sigma(m, None), np.full(3, 0.2, np.float32))
    noise._mu = np.ones(3)
    with pytest.raises(ValueError, match="non-zero mean"):
        L.noise_sigma(m, None)
    m.action_noise = object()
    with pytest.raises(ValueError, match="NormalActionNoise"):
        L.noise_sigma(m, None)


def test_live_parameter_recognisers_on_the_host():
    from reinforcementlearning4meshgeneration_amd import actor, policy
    sac = rl_stubs.sac_model()
    p = actor.FusedActor.live_params(sac)
    assert [tuple(x.shape) for x in p] == [(128, 18), (128,), (128, 128), (128,), (128, 128), (128,), (3, 128), (3,), (3, 128), (3,)]
    assert p[0] is sac.actor.latent_pi[0].weight and p[8] is sac.actor.log_std.weight          # the live tensors themselves
    assert actor.FusedActor.live_params(sac.actor)[6] is sac.actor.mu.weight
    with pytest.raises(ValueError, match="not an SB3 SAC actor"):
        actor.FusedActor.live_params(rl_stubs.td3_model())
    with pytest.raises(ValueError, match="hidden layers"):
        actor.FusedActor.live_params(rl_stubs.sac_model(H=64))
    # FusedPolicy.bind_live no longer refuses the deterministic kind: its host-side checks take a TD3 stand-in
    td3 = rl_stubs.td3_model()
    H, act, six = policy.live_deterministic(td3)
    assert (H, act) == (256, "relu") and [tuple(x.shape) for x in six] == [(256, 18), (256,), (256, 256), (256,), (3, 256), (3,)]
    assert six[0] is td3.actor.mu[0].weight and six[4] is td3.actor.mu[4].weight
    assert policy.live_deterministic(td3.actor)[2][0] is six[0]
    with pytest.raises(ValueError, match="is a SAC model"):
        policy.live_deterministic(sac)
    fp = policy.FusedPolicy.__new__(policy.FusedPolicy)                 # no device: the checks in front of the C call
    fp.spec = policy.PolicySpec.from_sb3(td3, sigma=0.1)
    fp.device = "cuda:0"
    with pytest.raises(ValueError, match=r"is on cpu; FusedPolicy.bind_live binds"):
        fp.bind_live(td3)
    fp.spec = policy.PolicySpec.from_sb3(rl_stubs.td3_model(H=128), sigma=0.1)
    with pytest.raises(ValueError, match=r"the live policy is relu \[256, 256\]; this FusedPolicy was loaded as relu \[128, 128\]"):
        fp.bind_live(td3)
    fa = actor.FusedActor.__new__(actor.FusedActor)
    with pytest.raises(ValueError, match="bind_live"):
        fa.refresh()


def test_exports_declarations_and_header():
    import reinforcementlearning4meshgeneration_amd as pkg
    from reinforcementlearning4meshgeneration_amd import _capi
    L = _L()
    for k in ("FusedOffPolicyLearn", "OffPolicyLearnSpec", "OffPolicyLearnLogs", "EpisodeStats"):
        assert k in pkg.__all__ and getattr(pkg, k) is getattr(L, k)
    assert L.EpisodeStats.PREFIX == "meshenv_episode_stats"
    names = _capi.EXPORTS_OFFPOLICY_LEARN
    assert len(names) == len(set(names)) == 10
    header = open(os.path.join(ROOT, "include", "meshenv_offpolicy_learn.h")).read()
    defines = dict(re.findall(r"#define\s+(MESHENV_[A-Z_]+)\s+(\d+)", header))
    assert int(defines["MESHENV_UNIFORM_PHILOX_TAG"]) == _capi.UNIFORM_PHILOX_TAG == 4
    assert int(defines["MESHENV_EPISODE_RING_DOUBLES"]) == _capi.EPISODE_RING_DOUBLES == 3
    kernels = open(os.path.join(ROOT, "reinforcementlearning4meshgeneration_amd", "csrc", "meshenv_learn.h")).read()
    assert "kUniformPhiloxTag = 4u" in kernels and "k_uniform_actions" in kernels and "k_episode_stats" in kernels
    lib = _capi.load()
    assert lib.meshenv_uniform_actions.restype is not None and lib.meshenv_episode_stats_update.argtypes is not None
    for cls, attrs in ((pkg.FusedActor, ("bind_live", "refresh")), (pkg.MeshVecEnv, ("collect_uniform", "uniform_actions", "step_actions_T"))):
        assert all(hasattr(cls, a) for a in attrs)
