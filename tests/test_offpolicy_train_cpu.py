"""CPU: the host half of ``FusedOffPolicyTrain`` (reinforcementlearning4meshgeneration_amd/offpolicy_train.py): the two
schedules against the transcription of SB3's loops (tests/offpolicy_train_ref.py), the restatement of ``k_offpolicy_finish``'s
summation order and actor-step selector past 1024 steps, the scalar sets of the critic and the actor
steps against successive ``OptimStepSpec.commit`` preparations, the scheduled learning rate, the hyper-parameters, every
refusal, the draw counter, and the packaging."""
import math
import os
import re
import types

import numpy as np
import pytest

import offpolicy_train_ref as TR
import rl_stubs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _T():
    from reinforcementlearning4meshgeneration_amd import offpolicy_train
    return offpolicy_train


# ----------------------------------------------------------------------------------------------------------- 1. schedules
@pytest.mark.parametrize("K,interval", [(1, 1), (5, 1), (5, 2), (7, 3), (3, 8)])
def test_sac_polyak_schedule_is_the_index_inside_the_call(K, interval):
    T = _T()
    want = [u for _, u in TR.sac_steps(K, interval)]
    assert T.sac_polyak_schedule(K, interval) == want and want[0]
    from reinforcementlearning4meshgeneration_amd.optim_step import PROGRAMS
    for n_updates in (0, 5):                                 # _n_updates does not enter
        progs = T.actor_programs(True, K, dict(target_update_interval=interval, n_updates=n_updates))
        assert [PROGRAMS[p] for p in progs] == ["actor_polyak" if u else "actor" for u in want]


@pytest.mark.parametrize("K,delay,n_updates", [(3, 2, 0), (3, 2, 3), (1, 2, 0), (1, 2, 1), (4, 1, 0), (4, 1, 7), (7, 3, 4), (2, 5, 0)])
def test_td3_actor_schedule_tests_the_incremented_n_updates(K, delay, n_updates):
    T = _T()
    steps, after = TR.td3_steps(K, delay, n_updates)
    want = [u for _, u in steps]
    assert after == n_updates + K
    assert T.td3_actor_schedule(K, delay, n_updates) == want
    from reinforcementlearning4meshgeneration_amd.optim_step import PROGRAMS
    progs = T.actor_programs(False, K, dict(policy_delay=delay, n_updates=n_updates))
    assert [PROGRAMS[p] if p >= 0 else None for p in progs] == ["actor_polyak" if u else None for u in want]
    if delay == 1:
        assert all(want)
    if (K, delay) == (1, 2):
        assert want == [n_updates % 2 == 1]                  # from an even _n_updates: no actor step


def test_td3_two_calls_of_three_step_the_actor_at_updates_2_4_6():
    T = _T()
    first = T.td3_actor_schedule(3, 2, 0)
    second = T.td3_actor_schedule(3, 2, 3)
    assert first == [False, True, False] and second == [True, False, True]


FINISH_K = (1, 5, 1024, 1025, 1027, 2050)


def _slots(K, seed=0):
    """[K][4] float32 of the sizes the four logged values have: critic_loss, actor_loss, ent_coef_loss, ent_coef."""
    rng = np.random.default_rng(seed + K)
    x = rng.standard_normal((K, 4)) * [0.3, 2.0, 0.5, 0.05] + [1.0, -3.0, 0.2, 0.9]
    return x.astype(np.float32)


@pytest.mark.parametrize("K", FINISH_K)
def test_k_offpolicy_finishs_order_keeps_the_sum_bound_for_every_phase_and_the_first_1024_steps_alone_do_not(K):
    """finish_order_means against math.fsum of the same float32 values within mean_and_bound, TD3 with policy_delay 1, 2, 3 and
    every _n_updates that gives another phase, SAC with a learned and a fixed coefficient.  The selected steps are those of
    SB3's schedules.  A kernel that read steps 0 .. 1023 only misses the bound at every K above 1024."""
    T = _T()
    slots = _slots(K)
    critic = [float(v) for v in slots[:, 0]]
    for delay in (1, 2, 3):
        phases = set()
        for n_updates in range(delay):
            steps, _ = TR.td3_steps(K, delay, n_updates)
            flags = [u for _, u in steps]
            assert flags == T.td3_actor_schedule(K, delay, n_updates)
            want = [k for k, u in enumerate(flags) if u]
            phase, period = TR.phase_period(flags)
            assert phase == ((delay - 1 - n_updates) % delay if want else K)
            phases.add(phase)
            for ph, per in {(phase, period), (phase, delay) if want else (phase, period)}:
                got = TR.finish_order_means(slots, K, ph, per, TR.TD3)
                assert got["steps"] == want, (K, delay, n_updates)
                mean, bound = TR.mean_and_bound(critic)
                assert abs(got["critic_loss"] - mean) <= bound
                if want:
                    mean, bound = TR.mean_and_bound([float(slots[k, 1]) for k in want])
                    assert abs(got["actor_loss"] - mean) <= bound
                else:
                    assert math.isnan(got["actor_loss"])
                assert math.isnan(got["ent_coef_loss"]) and math.isnan(got["ent_coef"]) and got["last_critic_loss"] == critic[-1]
        assert phases == (set(range(delay)) if K >= delay else set(range(K)) | {K})          # every phase below the period
    for interval in (1, 2):
        flags = [True for _ in TR.sac_steps(K, interval)]                             # SAC steps the actor at every step
        phase, period = TR.phase_period(flags)
        assert phase == 0 and period == (1 if K > 1 else K)
        got = TR.finish_order_means(slots, K, phase, period, TR.SAC_LEARNED)
        assert got["steps"] == [k for k, _ in TR.sac_steps(K, interval)]
        for key, col in (("critic_loss", 0), ("actor_loss", 1), ("ent_coef_loss", 2), ("ent_coef", 3)):
            mean, bound = TR.mean_and_bound([float(v) for v in slots[:, col]])
            assert abs(got[key] - mean) <= bound, key
    fixed = TR.finish_order_means(slots, K, 0, 1, TR.SAC_FIXED, ent_coef=0.1)
    assert fixed["ent_coef"] == float(np.float32(0.1)) and math.isnan(fixed["ent_coef_loss"])
    # the counter-example
    first = TR.finish_order_means(slots, K, 1 % K, 3, TR.TD3, trips=1)
    whole = TR.finish_order_means(slots, K, 1 % K, 3, TR.TD3)
    if K <= TR.FINISH_THREADS:
        assert all(first[key] == whole[key] or (math.isnan(first[key]) and math.isnan(whole[key])) for key in whole)
    else:
        for key, vals in (("critic_loss", critic), ("actor_loss", [float(slots[k, 1]) for k in whole["steps"]])):
            mean, bound = TR.mean_and_bound(vals)
            assert abs(first[key] - mean) > 1e-4 > bound, (key, first[key], mean)


def test_a_phase_at_or_past_k_selects_nothing():
    slots = _slots(5)
    for phase, period in ((5, 1), (5, 3), (7, 2)):
        got = TR.finish_order_means(slots, 5, phase, period, TR.TD3)
        assert got["steps"] == [] and math.isnan(got["actor_loss"]) and not math.isnan(got["critic_loss"])
        got = TR.finish_order_means(slots, 5, phase, period, TR.SAC_LEARNED)
        assert math.isnan(got["actor_loss"]) and math.isnan(got["ent_coef_loss"]) and not math.isnan(got["ent_coef"])
    assert TR.phase_period([False] * 5) == (5, 1) and TR.phase_period([False, False, True, False]) == (2, 4)
    # delay 3 over three calls of four: phases 2, 1, 0
    T = _T()
    assert [TR.phase_period(T.td3_actor_schedule(4, 3, n)) for n in (0, 4, 8)] == [(2, 4), (1, 4), (0, 3)]
    assert TR.phase_period(T.td3_actor_schedule(1027, 3, 4)) == (1, 3) and sum(T.td3_actor_schedule(1027, 3, 4)) == 342
    assert sum(T.sac_polyak_schedule(1027, 2)) == 514


# ----------------------------------------------------------------------------------------------------------- 2. scalar sets
def _ready(kind, loaded=None, **attrs):
    """A CPU model with a gradient on every stepped parameter and, with ``loaded``, an Adam state at that step."""
    import torch
    m = TR.model(kind, device="cpu", **attrs)
    for _, opt in TR.optimizers(m):
        for p in opt.param_groups[0]["params"]:
            p.grad = torch.ones_like(p)
            if loaded is not None:
                opt.state[p] = {"step": torch.tensor(float(loaded), dtype=torch.float32), "exp_avg": torch.full_like(p, 0.25),
                                "exp_avg_sq": torch.full_like(p, 0.5)}
    return m


@pytest.mark.parametrize("kind", ["sac", "td3"])
@pytest.mark.parametrize("loaded", [None, 1234])
def test_scalar_sets_equal_successive_commits_bit_for_bit(kind, loaded):
    T = _T()
    from reinforcementlearning4meshgeneration_amd.optim_step import OptimStepSpec
    K = 9
    m = _ready(kind, loaded)
    spec = OptimStepSpec.from_sb3(m)
    hp = T.hyper(m, kind == "sac")
    progs = T.actor_programs(kind == "sac", K, hp)
    n_actor = sum(p >= 0 for p in progs)
    assert n_actor == (K if kind == "sac" else 4)            # TD3 from _n_updates = 0, delay 2: updates 2, 4, 6, 8
    critic_sets, critic_values = T.scalar_sets(spec, spec.prepare("critic"), K)
    actor_sets, actor_values = T.scalar_sets(spec, spec.prepare("actor_polyak"), n_actor)
    start = float(loaded or 0)
    assert all(float(opt.state[p]["step"]) == start for _, opt in TR.optimizers(m) for p in opt.param_groups[0]["params"])
    assert critic_values == [[start + k for k in range(K + 1)]]
    assert actor_values == [[start + k for k in range(n_actor + 1)]] * (2 if kind == "sac" else 1)
    # what the composition does: a commit per critic step, and per ACTOR step only
    want_critic, want_actor = [], []
    for p in progs:
        want_critic.append(bytes(spec.commit(spec.prepare("critic"))))
        if p >= 0:
            want_actor.append(bytes(spec.commit(spec.prepare("actor_polyak"))))
    assert [bytes(critic_sets[k]) for k in range(K)] == want_critic
    assert [bytes(actor_sets[k]) for k in range(n_actor)] == want_actor
    assert float(m.actor.optimizer.state[m.actor.optimizer.param_groups[0]["params"][0]]["step"]) == start + n_actor
    # "actor" and "actor_polyak" step the same optimisers: one run of sets serves both
    m2 = _ready(kind, loaded)
    spec2 = OptimStepSpec.from_sb3(m2)
    other, _ = T.scalar_sets(spec2, spec2.prepare("actor"), n_actor)
    assert [bytes(other[k]) for k in range(n_actor)] == want_actor


@pytest.mark.parametrize("kind", ["sac", "td3"])
def test_the_scheduled_lr_is_in_every_set_of_every_optimiser(kind):
    T = _T()
    from reinforcementlearning4meshgeneration_amd.optim_step import OptimStepSpec, adam_scalars
    m = _ready(kind, lr_schedule=lambda progress: 1e-3 * progress, _current_progress_remaining=0.25)
    spec = T.OffPolicyTrainSpec(m)
    for opt in spec.optimizers():
        T.update_learning_rate(m, opt)
    assert len(spec.optimizers()) == (3 if kind == "sac" else 2)
    assert all(opt.param_groups[0]["lr"] == 2.5e-4 for opt in spec.optimizers())
    ospec = spec.optim
    for program, blocks in (("critic", 1), ("actor_polyak", 2 if kind == "sac" else 1)):
        sets, _ = T.scalar_sets(ospec, ospec.prepare(program), 4)
        for k in range(4):
            for b in range(blocks):
                assert sets[k].step_size[b] == np.float32(adam_scalars(float(k + 1), 2.5e-4, 0.9, 0.999)[0]), (program, k, b)
    assert isinstance(ospec, OptimStepSpec)


# ----------------------------------------------------------------------------------------------------------- 3. hyper-parameters
def test_hyper_reads_the_model_at_the_call():
    T = _T()
    m = types.SimpleNamespace(batch_size=100)
    assert T.hyper(m, True) == dict(batch_size=100, n_updates=0, target_update_interval=1)
    assert T.hyper(m, False) == dict(batch_size=100, n_updates=0, policy_delay=2)
    m = types.SimpleNamespace(batch_size=256, _n_updates=5, target_update_interval=3, policy_delay=4)
    assert T.hyper(m, True, 64) == dict(batch_size=64, n_updates=5, target_update_interval=3)
    assert T.hyper(m, False) == dict(batch_size=256, n_updates=5, policy_delay=4)
    for bad in (dict(batch_size=0), dict(batch_size=2.0), dict(batch_size=True), dict(batch_size=8, _n_updates=-1),
                dict(batch_size=8, target_update_interval=0), dict(batch_size=8, target_update_interval=1.5)):
        with pytest.raises(ValueError):
            T.hyper(types.SimpleNamespace(**bad), True)
    with pytest.raises(ValueError, match="policy_delay"):
        T.hyper(types.SimpleNamespace(batch_size=8, policy_delay=0), False)
    with pytest.raises(ValueError, match="batch_size"):
        T.hyper(types.SimpleNamespace(), True)


def test_the_sample_chunk_fills_the_named_cap():
    T = _T()
    assert T.SAMPLE_FLOATS == 41 and T.SAMPLE_WORKSPACE_BYTES == 64 << 20
    assert T.pick_chunk(5, 100) == 5
    assert T.pick_chunk(65536, 256) == (64 << 20) // (256 * 41 * 4) == 1598
    assert T.pick_chunk(3, 10 ** 7) == 1                     # one batch beyond the cap: still a chunk of one
    assert T.pick_chunk(8, 100, cap_bytes=2 * 100 * 41 * 4) == 2


# ----------------------------------------------------------------------------------------------------------- 4. refusals
@pytest.mark.parametrize("kind", ["sac", "td3"])
def test_the_spec_takes_the_two_recipes(kind):
    T = _T()
    spec = T.OffPolicyTrainSpec.from_sb3(TR.model(kind, device="cpu"))
    assert spec.sac == (kind == "sac") and spec.learned == (kind == "sac")
    assert type(spec.actor).__name__ == ("ActorGradSpec" if kind == "sac" else "TD3ActorGradSpec")
    fixed = T.OffPolicyTrainSpec(TR.model("sac", device="cpu", learned=False))
    assert fixed.sac and not fixed.learned and len(fixed.optimizers()) == 2


def test_refusals_name_their_reason():
    import torch
    T = _T()
    mk = lambda **kw: TR.model("sac", device="cpu", **kw)     # noqa: E731
    with pytest.raises(ValueError, match="use_sde"):
        T.OffPolicyTrainSpec(mk(use_sde=True))
    with pytest.raises(ValueError, match="optimize_memory_usage"):
        T.OffPolicyTrainSpec(mk(optimize_memory_usage=True))
    with pytest.raises(ValueError, match="_vec_normalize_env"):
        T.OffPolicyTrainSpec(mk(_vec_normalize_env=object()))
    with pytest.raises(ValueError, match="batch-norm"):
        T.OffPolicyTrainSpec(mk(batch_norm_stats=[torch.zeros(3)]))
    with pytest.raises(ValueError, match="target_update_interval"):
        T.OffPolicyTrainSpec(mk(target_update_interval=0))
    with pytest.raises(ValueError, match="policy_delay"):
        T.OffPolicyTrainSpec(TR.model("td3", device="cpu", policy_delay=-2))
    # what the driven specs refuse: one critic, another architecture, another optimiser
    one = rl_stubs.sac_model(n_critics=1)
    with pytest.raises(ValueError, match="n_critics = 1"):
        T.OffPolicyTrainSpec(one)
    with pytest.raises(ValueError, match="hidden layers"):
        T.OffPolicyTrainSpec(rl_stubs.sac_model(H=64))
    m = mk()
    m.critic.optimizer = torch.optim.SGD(TR.critic_params(m), lr=0.1)
    with pytest.raises(ValueError, match="not torch.optim.Adam"):
        T.OffPolicyTrainSpec(m)
    m = mk()
    m.critic.optimizer = torch.optim.Adam(TR.critic_params(m)[:-1], lr=3e-4)
    with pytest.raises(ValueError, match="critic optimiser's parameters"):
        T.OffPolicyTrainSpec(m)
    with pytest.raises(ValueError, match="neither SAC's"):
        T.OffPolicyTrainSpec(types.SimpleNamespace(critic_target=rl_stubs.twin_critic()))
    # the replay buffer
    with pytest.raises(ValueError, match="not a DeviceReplayBuffer"):
        T.check_replay_buffer(object(), None)
    # gradient_steps
    for bad in (0, -1, 1.0, True, None):
        with pytest.raises(ValueError, match="gradient_steps"):
            T.check_gradient_steps(bad)
    with pytest.raises(ValueError, match="at most 65536"):
        T.check_gradient_steps(65537)
    assert T.check_gradient_steps(65536) == 65536


# ----------------------------------------------------------------------------------------------------------- 5. the counter
def test_the_default_counter_continues_across_calls():
    T = _T()
    running, used = 0, []
    for K in (3, 5, 1):
        first, running = T.draw_counters(running, None, K)
        used += list(range(first, first + K))
    assert used == list(range(9)) and running == 9           # no draw is used twice
    assert T.draw_counters(9, 100, 4) == (100, 104)          # an explicit counter restarts the count after itself
    assert T.draw_counters(0, 2 ** 64 - 1, 2) == (2 ** 64 - 1, 1)
    assert T.DEFAULT_SEED == 0


# ----------------------------------------------------------------------------------------------------------- 6. packaging
def test_exports_constants_and_header():
    import reinforcementlearning4meshgeneration_amd as pkg
    from reinforcementlearning4meshgeneration_amd import _capi
    T = _T()
    assert pkg.FusedOffPolicyTrain is T.FusedOffPolicyTrain and pkg.OffPolicyTrainLogs is T.OffPolicyTrainLogs
    assert all(k in pkg.__all__ for k in ("FusedOffPolicyTrain", "OffPolicyTrainSpec", "OffPolicyTrainLogs"))
    assert T.FusedOffPolicyTrain.PREFIX == "meshenv_offpolicy_train"
    from reinforcementlearning4meshgeneration_amd import onpolicy_train
    assert T.scalar_sets is onpolicy_train.scalar_sets and T.step_values is onpolicy_train.step_values
    assert T.update_learning_rate is onpolicy_train.update_learning_rate
    names = _capi.EXPORTS_OFFPOLICY_TRAIN
    assert len(names) == 6 and len(set(names)) == 6
    header = open(os.path.join(ROOT, "include", "meshenv_offpolicy_train.h")).read()
    defines = dict(re.findall(r"#define\s+(MESHENV_[A-Z_]+)\s+(\d+)", header))
    assert int(defines["MESHENV_OFFTRAIN_OUTPUTS"]) == _capi.OFFTRAIN_OUTPUTS == len(T.OUTPUTS) == 8
    assert int(defines["MESHENV_OFFTRAIN_MAX_STEPS"]) == _capi.OFFTRAIN_MAX_STEPS == T.MAX_STEPS == 65536
    assert int(defines["MESHENV_OFFTRAIN_SAMPLE_FLOATS"]) == _capi.OFFTRAIN_SAMPLE_FLOATS == 41
    assert int(defines["MESHENV_REPLAY_BATCHES_MAX_SAMPLES"]) == _capi.REPLAY_BATCHES_MAX_SAMPLES == 2 ** 24
    enum = re.findall(r"MESHENV_OFFTRAIN_([A-Z_]+) = (\d+)", header)
    assert [k.lower() for k, _ in enum] == list(T.OUTPUTS) and [int(v) for _, v in enum] == list(range(8))
