"""GPU: ``FusedOnPolicyLearn.learn`` (include/meshenv_onpolicy_learn.h; csrc/meshenv_onpolicy_train.h: k_optim_step_counted,
k_learn_finish) against the loop of examples/ppo_train.py written out by hand on a twin model with an env of its own and the
same seeds, counters and permutations: ``collect_rollout`` -> ``EpisodeStats.update`` -> ``num_timesteps`` ->
``FusedOnPolicyTrain.train``, the existing path with its read-back per train() when there is a ``target_kl``.  Both sides run
the same kernels on the same inputs in the same order (the counted step differs from the gated one only in where its two
Adam scalars come from), so everything is compared for EQUAL BITS.

The models are tests/on_policy_stubs.py's; n_envs = 11, n_steps = 3 (33 rows), PPO with batch_size 8 (5 minibatches per epoch,
the last of one row) and 3 epochs (K = 15), A2C with its one minibatch of all rows; 5 iterations.

The ``target_kl`` of the early-stop tests comes from the twin's side alone: the hand loop is first run without one through
tests/onpolicy_train_ref.compose, which records approx_kl per minibatch.  With M_i the largest approx_kl of iteration i, the
limit 1.5 x target_kl is set just under M_i* for the first i* >= 1 whose M exceeds every earlier iteration's: iterations before
i* then apply all K steps on the recorded trajectory, and iteration i* stops inside (minibatch 0 of a train() has an
approx_kl of rounding size: the parameters are the rollout's).  Without such an i* the limit goes just under M_0 (what these
inputs give: iteration 0 applies 11 of its 15 steps, the other four all 15).  The test asserts both kinds of iteration from the
twin's ``steps_applied`` and fails if either is missing."""
import numpy as np
import pytest

import learn_twins as LT
import on_policy_stubs as S

pytestmark = pytest.mark.gpu

SHAPE = LT.DEFAULT_SHAPE                                     # the twins and the learners of tests/learn_twins.py at their defaults
N, T, BATCH, EPOCHS, ITERS, SEED = SHAPE.n, SHAPE.T, SHAPE.batch, SHAPE.epochs, 5, SHAPE.seed
ROWS, K = N * T, EPOCHS * 5
assert (N, T, BATCH, EPOCHS, SEED, K) == (11, 3, 8, 3, 5, SHAPE.K)


def _env(n=N):
    return LT.make_env(n, reset=True)


def _perms(kind, iterations=ITERS, seed=3):
    return LT.onpolicy_perms(kind, iterations, seed)


Twin, Learner, _bits, _assert_equal = LT.OnPolicyTwin, LT.Learner, LT.bits, LT.assert_onpolicy_equal


def _target(variant):
    """(target_kl, the recorded approx_kl per iteration and minibatch, i*): see the module docstring."""
    return LT.onpolicy_target(variant, ITERS, _perms("ppo"), key=("target", variant))


# ----------------------------------------------------------------------------------------------------------- 1. the hand loop
@pytest.mark.parametrize("kind", ["ppo", "a2c"])
def test_learn_without_a_target_kl_has_the_hand_loops_bits(kind):
    import torch
    a, b = Learner(kind), Twin(kind)
    perms = _perms(kind)
    logs = a.learn.learn(ITERS * ROWS - 1, seed=SEED, perms=perms)       # below a multiple: the fifth collect overshoots
    b.loop(ITERS * ROWS - 1, perms)
    assert a.model.num_timesteps == ITERS * ROWS and logs.iterations == ITERS and a.learn.readbacks == 0 and a.learn.counter is None
    _assert_equal(a, b, f"{kind} first learn", logs.device)
    assert a.model._n_updates == ITERS * (EPOCHS if kind == "ppo" else 1)
    assert all(float(a.opt.state[p]["step"]) == float(ITERS * (K if kind == "ppo" else 1)) for p in a.params)
    assert not any(torch.equal(p, q) for p, q in zip(a.params, S.policy(kind, "cuda")[1]))      # it did train
    read = logs.read()
    assert read["time/total_timesteps"] == ITERS * ROWS and read["time/iterations"] == ITERS and "episodes" in read
    assert read["train/n_updates"] == a.model._n_updates and read["train/value_loss"] == float(b.rows[-1][2])
    assert np.array_equal(logs.history().view(np.int64), torch.stack(b.rows).cpu().numpy().view(np.int64))
    b.rows = []
    perms2 = _perms(kind, 2, seed=4)
    logs = a.learn.learn(2 * ROWS, seed=SEED, perms=lambda i: perms2[i])   # a second learn() continues; perms as a callable
    b.loop(2 * ROWS, perms2)
    assert a.model.num_timesteps == (ITERS + 2) * ROWS and logs.iterations == ITERS + 2
    _assert_equal(a, b, f"{kind} second learn", logs.device)
    a.close(); b.close()


# ----------------------------------------------------------------------------------------------------------- 2. target_kl
@pytest.mark.parametrize("variant", ["plain", "scheduled"])
def test_learn_with_a_target_kl_has_the_bits_of_the_loop_with_a_read_back_per_train(variant):
    """scheduled: a linear lr_schedule and a callable clip_range, both read at every train() from _current_progress_remaining."""
    target, kls, star = _target(variant)
    a, b = Learner("ppo", variant, target), Twin("ppo", variant, target)
    perms = _perms("ppo")
    logs = a.learn.learn(ITERS * ROWS, seed=SEED, perms=perms)
    b.loop(ITERS * ROWS, perms)
    print(f"\n{variant}: steps applied per iteration {b.applied} of K = {K}")
    assert any(0 < s < K for s in b.applied), ("no iteration stops strictly inside its train()", b.applied, kls)
    assert any(s == K for s in b.applied), ("no iteration applies all K steps", b.applied, kls)
    assert a.learn.readbacks == 1 and a.learn.counter is not None and logs.iterations == ITERS
    _assert_equal(a, b, f"target_kl {variant}", logs.device)
    assert all(float(a.opt.state[p]["step"]) == float(sum(b.applied)) for p in a.params) and sum(b.applied) < ITERS * K
    words = a.learn.counter.words[:3].cpu().tolist()
    assert words == [a.model._n_updates, 0, sum(b.applied)], words
    assert [int(v) for v in logs.history()[:, 8]] == b.applied
    assert logs.read()["train/n_updates"] == b.model._n_updates
    if variant == "scheduled":
        assert a.opt.param_groups[0]["lr"] == 1.0e-4 + 4.0e-4 * a.model._current_progress_remaining == b.opt.param_groups[0]["lr"]
    a.close(); b.close()


# ----------------------------------------------------------------------------------------------------------- 3. mixing
def test_counted_learn_mixes_with_train_and_a_stock_optimizer_step():
    """On the caller's own handles: a counted learn(), a plain tr.train(out), a stock optimizer.step() and a state_dict round
    trip, a second counted learn().  The table's origin is re-derived from the host ``step`` at every learn()."""
    target, _, _ = _target("plain")
    a, b = Learner("ppo", "plain", target, own_handles=True), Twin("ppo", "plain", target)
    perms, mid, perms2 = _perms("ppo", 2), _perms("ppo", 1, seed=8)[0], _perms("ppo", 3, seed=9)
    a.learn.learn(2 * ROWS, seed=SEED, perms=perms)
    b.loop(2 * ROWS, perms)
    _assert_equal(a, b, "first counted learn")
    for side in (a, b):
        m = side.model
        out = side.env.collect_rollout(side.fp, T, seed=SEED, counter=1000, gamma=m.gamma, gae_lambda=m.gae_lambda)
        side.tr.train(out, mid)                                                  # the existing path, with its read-back
        side.opt.step()                                                          # stock torch on the same state
        side.opt.load_state_dict(side.opt.state_dict())
    _assert_equal(a, b, "after train() and optimizer.step()")
    step = float(a.opt.state[a.params[0]]["step"])
    logs = a.learn.learn(3 * ROWS, seed=SEED, perms=perms2)
    b.rows = []
    b.loop(3 * ROWS, perms2)
    _assert_equal(a, b, "second counted learn", logs.device)
    assert float(a.opt.state[a.params[0]]["step"]) == step + sum(b.applied[-3:]) and a.learn.readbacks == 2
    assert a.tr.calls == 6 and a.fp._h and a.tr._h                            # the caller's handles stay the caller's
    a.close(); b.close()


# ----------------------------------------------------------------------------------------------------------- 4. segments
def test_a_table_cap_below_the_run_gives_segments_with_equal_bits(monkeypatch):
    from reinforcementlearning4meshgeneration_amd import onpolicy_learn as L
    target, _, _ = _target("plain")
    perms = _perms("ppo")
    a, b = Learner("ppo", "plain", target), Learner("ppo", "plain", target)
    whole = a.learn.learn(ITERS * ROWS, seed=SEED, perms=perms)                   # iterations x K = 75 entries in one table
    assert a.learn.readbacks == 1 and a.learn.counter.entries == ITERS * K
    monkeypatch.setattr(L, "TABLE_CAP", 7)
    cut = b.learn.learn(ITERS * ROWS, seed=SEED, perms=perms)
    assert b.learn.readbacks == ITERS and b.learn.counter.entries == K           # a cap below K: one train() per segment
    _assert_equal(b, a, "segmented against whole", cut.device, want=list(whole.device))
    assert b.learn.counter.words[:3].cpu().tolist()[1] == 0                      # the error word is clear
    a.close(); b.close()


# ----------------------------------------------------------------------------------------------------------- 5. the guard
def test_a_table_too_short_is_refused_before_the_launch_in_python_and_in_c():
    """A table of 1 entry, K = 15, a target that never triggers: refused by StepCounter.check, and with that check taken away
    by meshenv_onpolicy_learn_run itself (MESHENV_E_ARG).  Nothing is enqueued either time; no launch indexes past a table."""
    import torch

    from reinforcementlearning4meshgeneration_amd import MeshEnvError, StepCounter
    a = Learner("ppo", "plain", 1.0e9, own_handles=True)
    m = a.model
    before = [p.detach().clone() for p in a.params]
    counter = StepCounter(m)
    counter.bind(a.tr._prepared()[0], 1, 1)
    out = a.env.collect_rollout(a.fp, T, seed=SEED, counter=0, gamma=m.gamma, gae_lambda=m.gae_lambda)
    perms = _perms("ppo", 1)[0]
    with pytest.raises(ValueError, match="15 minibatches after 0 claimed since the bind; the table has 1 entries"):
        a.tr.train(out, perms, counted=counter)
    counter.check = lambda train, K: None
    with pytest.raises(MeshEnvError, match=r"meshenv_onpolicy_learn_run failed \(code -1\).*the table has 1 entries"):
        a.tr.train(out, perms, counted=counter)
    torch.cuda.synchronize()
    assert a.tr.calls == 0 and counter.claimed == 0 and counter.pending == []
    assert counter.words[:3].cpu().tolist() == [0, 0, 0] and bool((counter.history == 0).all())
    assert all(torch.equal(p, q) for p, q in zip(a.params, before)) and all(len(a.opt.state[p]) == 0 or float(a.opt.state[p]["step"]) == 0.0 for p in a.params)
    assert counter.read() == (0, 0) and m._n_updates == 0
    del counter.check                                                            # the class's own again
    with pytest.raises(ValueError, match="no table bound"):
        a.tr.train(out, perms, counted=counter)
    a.tr.train(out, perms)                                                       # the handles are as usable as before
    assert a.tr.calls == 1 and float(a.opt.state[a.params[0]]["step"]) == float(K)
    counter.close()
    a.close()


# ----------------------------------------------------------------------------------------------------------- 6. the callback
def test_learn_with_an_eval_callback_equals_the_loop_cut_at_the_same_points():
    import torch

    from reinforcementlearning4meshgeneration_amd import DeviceEvalCallback
    target, _, _ = _target("plain")
    a, b = Learner("ppo", "plain", target), Twin("ppo", "plain", target)
    envs = [_env(4), _env(4)]
    kw = dict(eval_freq=6, eval_steps=8, deterministic=True, capacity=4)           # 15 vector steps: evaluations at 6 and 12
    ca, cb = DeviceEvalCallback(envs[0], a.model, **kw), DeviceEvalCallback(envs[1], b.model, **kw)
    perms = _perms("ppo")
    with pytest.raises(ValueError, match="another model"):
        a.learn.learn(ITERS * ROWS, seed=SEED, perms=perms, callback=cb)
    with pytest.raises(TypeError, match="DeviceEvalCallback"):
        a.learn.learn(ITERS * ROWS, seed=SEED, perms=perms, callback=object())
    assert a.model.num_timesteps == 0 and a.learn.steps == 0
    logs = a.learn.learn(ITERS * ROWS, seed=SEED, perms=perms, callback=ca)
    b.loop(ITERS * ROWS, perms, cb=cb)
    _assert_equal(a, b, "with a callback", logs.device)
    ra, rb = ca.read(), cb.read()
    assert ra["evaluations"] == rb["evaluations"] == 2 and list(ra["timesteps"]) == [2 * ROWS, 4 * ROWS] and ca.n_calls == cb.n_calls == 15
    for k in ra:
        x, y = np.asarray(ra[k]), np.asarray(rb[k])
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), k
    assert torch.equal(_bits(ca.best), _bits(cb.best)) and torch.equal(_bits(ca._log), _bits(cb._log))
    assert a.learn.readbacks == 1
    for h in (ca, cb, *envs):
        h.close()
    a.close(); b.close()


# ----------------------------------------------------------------------------------------------------------- 7. repeatability
def test_two_fresh_runs_give_equal_bits_and_close_twice_is_harmless():
    import torch
    target, _, _ = _target("plain")
    perms = _perms("ppo")
    runs = []
    for _ in range(2):
        a = Learner("ppo", "plain", target)
        logs = a.learn.learn(ITERS * ROWS, seed=SEED, perms=perms)
        runs.append(([p.detach().clone() for p in a.params], logs.device.clone(), a.stats.state.clone(), a.model._n_updates))
        torch.cuda.synchronize()
        a.learn.close()
        a.learn.close()
        a.close()
    assert all(torch.equal(_bits(p), _bits(q)) for p, q in zip(runs[0][0], runs[1][0]))
    assert torch.equal(_bits(runs[0][1]), _bits(runs[1][1])) and torch.equal(_bits(runs[0][2]), _bits(runs[1][2]))
    assert runs[0][3] == runs[1][3]
