"""GPU: the device evaluation callback (include/meshenv_eval_callback.h, csrc/meshenv_eval_callback.h,
reinforcementlearning4meshgeneration_amd/eval_callback.py), every comparison bit for bit:

1. meshenv_evaluate_queued against MeshVecEnv.evaluate (the polling loop) on twin envs: the same records with the polling
   loop's step count, the prefix of them with half of it;
2. k_eval_reduce against tests/eval_callback_ref.py on hand-filled tally buffers with NaN planted in every hole;
3. k_keep_best: the gate over means [1.0, 0.5, 1.0, 2.0, NaN], misaligned sources and destinations, canaries, and the round
   trip of the real SAC / TD3 / PPO snapshot sets through load_best;
4. learn(callback=cb) for SAC and TD3 against the same loop cut at the evaluation points with a host-side callback
   (evaluate(), the restated reduce, clone()), and against learn() without a callback: evaluation does not disturb training;
5. evaluate_now from the PPO loop of examples/ppo_train.py."""
import ctypes as C

import numpy as np
import pytest

import eval_callback_ref as ER
import offpolicy_train_ref as TR
import on_policy_stubs

pytestmark = pytest.mark.gpu

LOW = np.array([-1.0, -1.5, 0.0]); HIGH = np.array([1.0, 1.5, 1.5])
MEAN = np.array([0.0, 0.6, 0.75])        # the centre of the biased random actions of tests/test_gpu_eval.py: episodes that end
SPREAD = np.array([0.6, 0.25, 0.3])
SCALED_MEAN = np.arctanh((MEAN - LOW) / (HIGH - LOW) * 2 - 1)


def _env(n, log_capacity=160):
    from reinforcementlearning4meshgeneration_amd import MeshVecEnv, boundary
    return MeshVecEnv([boundary(0)], n_envs=n, log_capacity=log_capacity)


def _raw_handle():
    from reinforcementlearning4meshgeneration_amd._handle import Handle
    return type("RawEvalCallback", (Handle,), {"PREFIX": "meshenv_eval_callback"})(0)


# ------------------------------------------------------------------------------------------ 1. the queued evaluation
def _policy(seed):
    import torch
    from reinforcementlearning4meshgeneration_amd.policy import FusedPolicy
    torch.manual_seed(seed)
    tower = lambda: [torch.nn.Linear(18, 64), torch.nn.Linear(64, 64)]   # noqa: E731
    head = torch.nn.Linear(64, 3)
    with torch.no_grad():
        head.weight.mul_(0.3)
        head.bias.copy_(torch.tensor(MEAN))
    return FusedPolicy.actor_critic(tower(), tower(), head, torch.nn.Linear(64, 1), torch.tensor(np.log(SPREAD)), activation="relu")


def _actor(seed):
    import torch
    from reinforcementlearning4meshgeneration_amd.actor import FusedActor
    torch.manual_seed(seed)
    lin = [torch.nn.Linear(18, 128), torch.nn.Linear(128, 128), torch.nn.Linear(128, 128)]
    mu, ls = torch.nn.Linear(128, 3), torch.nn.Linear(128, 3)
    with torch.no_grad():
        mu.weight.mul_(0.3); mu.bias.copy_(torch.tensor(SCALED_MEAN))
        ls.weight.mul_(0.1); ls.bias.copy_(torch.tensor(np.log([0.7, 0.25, 0.4])))
    return FusedActor.from_torch(lin, mu, ls)


def _queued(env, pol, det, seed, counter, steps, targets):
    """meshenv_evaluate_queued with the buffers MeshVecEnv.evaluate builds, read back the way it reads them.
    Returns (EvalResult, count [n], short)."""
    import torch as t
    from reinforcementlearning4meshgeneration_amd import _capi
    from reinforcementlearning4meshgeneration_amd.actor import FusedActor
    from reinforcementlearning4meshgeneration_amd.evaluation import EvalResult
    n = env.num_envs
    offsets = np.zeros(n, np.int32)
    offsets[1:] = np.cumsum(targets, dtype=np.int64)[:-1]
    total = int(targets.sum())
    m = max(total, 1)
    i32, f64 = dict(dtype=t.int32, device=env.device), dict(dtype=t.float64, device=env.device)
    buf = dict(target_dev=t.from_numpy(targets).to(env.device), offset_dev=t.from_numpy(offsets).to(env.device),
               count_dev=t.empty(n, **i32), length_dev=t.empty(n, **i32), seen_dev=t.empty(n, **i32),
               return_dev=t.empty(n, **f64), return_raw_dev=t.empty(n, **f64), short_dev=t.zeros(1, **i32),
               ep_env_dev=t.zeros(m, **i32), ep_domain_dev=t.zeros(m, **i32), ep_step_dev=t.zeros(m, **i32),
               ep_length_dev=t.zeros(m, **i32), ep_flags_dev=t.zeros(m, **i32), ep_n_elements_dev=t.zeros(m, **i32),
               ep_archive_dev=t.zeros(m, **i32), ep_return_dev=t.zeros(m, **f64), ep_return_raw_dev=t.zeros(m, **f64),
               ep_quality_dev=t.zeros((m, 8, 4), **f64))
    buf.update(obs_dev=env.obs, reward_dev=env.reward, done_dev=env.done, complete_dev=env.complete)
    B = _capi.MeshEvalBuffers()
    B.struct_size = C.sizeof(_capi.MeshEvalBuffers)
    for k, v in buf.items():
        setattr(B, k, v.data_ptr())
    env._bind_stream()
    pol._bind_stream()
    actor = isinstance(pol, FusedActor)
    rc = env._L.meshenv_evaluate_queued(env._handle, None if actor else pol._h, pol._h if actor else None, 0 if det else 1,
                                        C.c_uint64(seed), C.c_uint64(counter), int(steps), C.byref(B))
    env._check(rc, "meshenv_evaluate_queued")
    counts = buf["count_dev"].cpu().numpy()
    owner = np.repeat(np.arange(n), targets)
    keep = (np.arange(total) - offsets[owner]) < counts[owner]
    rec = {k[3:-4]: buf[k][:total].cpu().numpy()[keep] for k in buf if k.startswith("ep_")}
    short = int(buf["short_dev"].item())
    return EvalResult.from_records(rec, targets, steps, short == 0), counts, short


FIELDS = ("env", "domain", "step", "length", "reward", "reward_raw", "complete", "overflow", "n_elements", "archive", "quality")


def _same_records(a, b, sel=None):
    for f in FIELDS:
        x, y = getattr(a, f), getattr(b, f)
        y = y if sel is None else y[sel]
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), f


@pytest.mark.parametrize("kind", ["policy", "actor"])
@pytest.mark.parametrize("det", [True, False], ids=["det", "stoch"])
def test_queued_evaluation_equals_the_polling_loop(kind, det):
    """96 envs (not a multiple of 64), targets that mix 0, 1 and 2.  Every episode of boundary(0) ends (the fail limit truncates
    it), so the polling loop finishes; `finished` and a few hundred steps are asserted below, or the comparison would be empty."""
    n, seed, counter = 96, 5, 1000
    targets = (np.arange(n) % 3).astype(np.int32)
    pol = _policy(3) if kind == "policy" else _actor(3)
    poll, queue, cut = _env(n), _env(n), _env(n)      # one fresh env per run: ep_archive counts an env's episodes since its creation
    try:
        res = poll.evaluate(pol, episodes_per_env=targets, deterministic=det, seed=seed, counter=counter, max_steps=1500, check_every=1)
        S = res.steps
        print(kind, "det" if det else "stoch", "steps", S, "episodes", len(res), "complete", int(res.complete.sum()))
        assert res.finished and 2 <= S <= 1000 and len(res) == int(targets.sum())
        full, count, short = _queued(queue, pol, det, seed, counter, S, targets)
        assert short == 0 and np.array_equal(count, targets) and full.finished
        _same_records(full, res)
        half, count, short = _queued(cut, pol, det, seed, counter, S // 2, targets)
        first = res.step < S // 2
        assert 0 < first.sum() < len(res) or S < 4
        _same_records(half, res, first)
        want = np.bincount(res.env[first], minlength=n)
        assert np.array_equal(count, want) and short == int((want < targets).sum()) and short > 0
    finally:
        pol.close(); poll.close(); queue.close(); cut.close()


# ------------------------------------------------------------------------------------------ 2. the reduction
def _upload(b, device):
    import torch as t
    from reinforcementlearning4meshgeneration_amd import _capi
    dev = {k: t.from_numpy(np.ascontiguousarray(v)).to(device) for k, v in b.items()}
    B = _capi.MeshEvalBuffers()
    B.struct_size = C.sizeof(_capi.MeshEvalBuffers)
    B.target_dev, B.offset_dev, B.count_dev = dev["target"].data_ptr(), dev["offset"].data_ptr(), dev["count"].data_ptr()
    B.ep_return_dev, B.ep_length_dev = dev["ep_return"].data_ptr(), dev["ep_length"].data_ptr()
    B.ep_flags_dev, B.ep_n_elements_dev, B.short_dev = dev["ep_flags"].data_ptr(), dev["ep_n_elem"].data_ptr(), dev["short"].data_ptr()
    return B, dev


def _counts(k, n, rng):
    counts = np.zeros(n, np.int32)
    for _ in range(k):
        counts[rng.integers(n)] += 1
    return counts


def test_reduce_equals_the_restated_order_bit_for_bit():
    import torch as t
    h = _raw_handle()
    cap = 16
    log = t.zeros(cap * 9 + 4, dtype=t.float64, device="cuda")
    log[cap * 9:] = t.tensor([-np.inf, -1.0, np.nan, 0.0], dtype=t.float64)
    improved = t.full((1,), 7, dtype=t.int32, device="cuda")
    ref = ER.CallbackRef()
    rng = np.random.default_rng(0)
    cases = []
    for k, n, log_on in ((0, 5, True), (1, 3, True), (63, 64, True), (64, 200, True), (65, 65, True), (1000, 333, True), (1000, 4096, True),
                         (64, 130, False), (0, 130, True)):
        counts = _counts(k, n, rng)
        targets = counts + rng.integers(0, 3, n).astype(np.int32)          # unrecorded slots after the recorded ones
        targets[(counts == 0) & (rng.random(n) < 0.5)] = 0                  # envs with a zero target: holes of their own kind
        cases.append((targets, counts, log_on))
    try:
        flags = []
        for row, (targets, counts, log_on) in enumerate(cases):
            b = ER.tally_buffers(targets, counts, seed=50 + row, log=log_on)
            short = int((counts < targets).sum())
            B, dev = _upload(dict(b, short=np.array([short], np.int32)), h.device)
            rc = h._L.meshenv_eval_reduce(h._h, len(targets), int(targets.sum()), C.byref(B), row, cap, float(1000 * row + 7),
                                          log.data_ptr(), log[cap * 9:].data_ptr(), improved.data_ptr())
            h._check(rc, "meshenv_eval_reduce")
            flags.append(int(improved.item()))
            _, want = ref.add(**b, short=short, num_timesteps=1000 * row + 7)
            assert flags[-1] == int(want), row
        host = log.cpu().numpy()
        got, state = host[:cap * 9].reshape(cap, 9), host[cap * 9:]
        want = ref.history()
        for row in range(len(cases)):
            assert ER.bits(got[row]).tolist() == ER.bits(want[row]).tolist(), (row, got[row], want[row])
        assert ER.bits(state).tolist() == ER.bits(ref.state()).tolist()
        assert not got[len(cases):].any()                                   # rows never asked for stay untouched
        recorded = want[:, 4].tolist()
        assert recorded == [0, 1, 63, 64, 65, 1000, 1000, 64, 0] and flags[0] == 0 and sum(flags) >= 2 and 0 in flags[1:]
        assert (want[1:7, 1] < 0).any() and (want[1:7, 1] > 0).any()        # means of both signs
        # refusals in front of the launch
        B, _ = _upload(dict(ER.tally_buffers([1], [1], seed=1), short=np.zeros(1, np.int32)), h.device)
        for args in ((0, 1, 0, cap), (1, -1, 0, cap), (1, 1, cap, cap), (1, 1, -1, cap)):
            rc = h._L.meshenv_eval_reduce(h._h, args[0], args[1], C.byref(B), args[2], args[3], 0.0, log.data_ptr(), log.data_ptr(), improved.data_ptr())
            assert rc == -1
    finally:
        h.close()


# ------------------------------------------------------------------------------------------ 3. the gated copy
def _feed_mean(h, mean, row, cap, log, improved):
    """One evaluation of one env whose single episode returned `mean` (None: nothing recorded, a NaN mean)."""
    b = ER.tally_buffers([1], [0 if mean is None else 1], seed=row)
    if mean is not None:
        b["ep_return"][0] = mean
    B, dev = _upload(dict(b, short=np.zeros(1, np.int32)), h.device)
    h._check(h._L.meshenv_eval_reduce(h._h, 1, 1, C.byref(B), row, cap, float(row), log.data_ptr(), log[cap * 9:].data_ptr(),
                                      improved.data_ptr()), "meshenv_eval_reduce")
    return dev


def test_keep_best_copies_on_a_strict_improvement_only():
    import torch as t
    from reinforcementlearning4meshgeneration_amd import _capi
    h = _raw_handle()
    cap = 8
    log = t.zeros(cap * 9 + 4, dtype=t.float64, device="cuda")
    log[cap * 9:] = t.tensor([-np.inf, -1.0, np.nan, 0.0], dtype=t.float64)
    improved = t.zeros(1, dtype=t.int32, device="cuda")
    # sources: views of one buffer at offsets 1, 2, 5 (4-byte aligned only), 2310 (8 bytes), 4616 and 4624 (16 bytes)
    sizes = [1, 3, 128 * 18, 5, 1027, 64]
    src_at = [1, 2, 5, 2310, 4616, 5644]
    pool = t.zeros(5644 + 64 + 3, dtype=t.float32, device="cuda")
    assert pool.data_ptr() % 16 == 0
    live = [pool[a:a + s] for a, s in zip(src_at, sizes)]
    # destinations with canary words before, between and after; offsets 3, 5, 9 and 2318 start off a 16-byte boundary
    dst_at = [3, 5, 9, 2318, 2324, 3352]
    floats = 3352 + 64 + 5
    CANARY = 1234.5
    best = t.full((floats,), CANARY, dtype=t.float32, device="cuda")
    assert best.data_ptr() % 16 == 0
    covered = np.zeros(floats, bool)
    for a, s in zip(dst_at, sizes):
        assert not covered[a:a + s].any()
        covered[a:a + s] = True
    assert not covered[0] and not covered[-1] and (~covered).sum() >= len(sizes) + 1
    tab = (_capi.MeshKeepEntry * len(sizes))()
    for e, x, a in zip(tab, live, dst_at):
        e.src_dev, e.dst_offset, e.numel = x.data_ptr(), a, x.numel()
    try:
        snaps, keeps = [], []
        for row, mean in enumerate([1.0, 0.5, 1.0, 2.0, None]):
            pool.copy_(t.randn(pool.numel(), device="cuda") + 10.0 * (row + 1))      # the live tensors change between evaluations
            snaps.append([x.clone() for x in live])
            keepalive = _feed_mean(h, mean, row, cap, log, improved)
            h._check(h._L.meshenv_keep_best(h._h, tab, len(sizes), best.data_ptr(), floats, improved.data_ptr()), "meshenv_keep_best")
            keeps.append(int(improved.item()))
            want = snaps[0] if row < 3 else snaps[3]
            got = best.cpu().numpy()
            for x, a, s in zip(want, dst_at, sizes):
                assert got[a:a + s].tobytes() == x.cpu().numpy().tobytes(), (row, s)
            assert (got[~covered] == np.float32(CANARY)).all(), row
            del keepalive
        assert keeps == [1, 0, 0, 1, 0]
        state = log[cap * 9:].cpu().numpy()
        assert state[0] == 2.0 and state[1] == 3.0 and np.isnan(state[2]) and state[3] == 5.0
        # refusals in front of the launch: outside the buffer, no entries, too many, a null source
        tab[5].numel = 70
        assert h._L.meshenv_keep_best(h._h, tab, len(sizes), best.data_ptr(), floats, improved.data_ptr()) == -1
        tab[5].numel = 64
        assert h._L.meshenv_keep_best(h._h, tab, 0, best.data_ptr(), floats, improved.data_ptr()) == -1
        assert h._L.meshenv_keep_best(h._h, tab, 65, best.data_ptr(), floats, improved.data_ptr()) == -1
        tab[0].src_dev = None
        assert h._L.meshenv_keep_best(h._h, tab, len(sizes), best.data_ptr(), floats, improved.data_ptr()) == -1
        assert (best.cpu().numpy()[~covered] == np.float32(CANARY)).all()
    finally:
        h.close()


def _ppo_model():
    import torch
    model, params = on_policy_stubs.model("ppo", device="cuda")
    with torch.no_grad():
        model.policy.action_net.weight.mul_(0.3)
        model.policy.action_net.bias.copy_(torch.tensor(MEAN))
        model.policy.log_std.copy_(torch.tensor(np.log(SPREAD)))
    return model, params


@pytest.mark.parametrize("kind", ["sac", "td3", "ppo"])
def test_real_snapshot_sets_round_trip_through_load_best(kind):
    import torch as t
    from reinforcementlearning4meshgeneration_amd import DeviceEvalCallback
    from reinforcementlearning4meshgeneration_amd.eval_callback import snapshot_set
    model = _ppo_model()[0] if kind == "ppo" else TR.model(kind)
    env = _env(8, log_capacity=0)
    cb = DeviceEvalCallback(env, model, eval_freq=1, eval_steps=1)
    try:
        named = snapshot_set(model)[1]
        assert len(named) == {"sac": 43, "td3": 36, "ppo": 13}[kind]
        with pytest.raises(ValueError, match="nothing was kept"):
            cb.load_best()
        kept = {k: x.detach().clone() for k, x in named}
        cb.improved.fill_(1)                                                   # the word k_eval_reduce leaves after an improvement
        cb.state[1] = 0.0
        cb._check(cb._L.meshenv_keep_best(cb._h, cb._entries, len(cb._entries), cb.best.data_ptr(), cb.best.numel(), cb.improved.data_ptr()),
                  "meshenv_keep_best")
        with t.no_grad():
            for _, x in named:
                x.add_(1.0)                                                     # training goes on
        best = cb.best_state()
        assert list(best) == [k for k, _ in named]
        for k, x in named:
            assert best[k].shape == x.shape and t.equal(best[k].view(t.int32), kept[k].view(t.int32)) and not t.equal(x.detach(), kept[k])
        used = sum(-(-x.numel() // 4) * 4 for _, x in named)
        assert cb.best.numel() == used                                          # padding words between the tensors stay zero
        pad = t.ones(used, dtype=t.bool, device="cuda")
        for (k, x), at in zip(named, cb._offsets):
            pad[at:at + x.numel()] = False
        assert not cb.best[pad].any()
        cb.load_best(model)
        for k, x in named:
            assert t.equal(x.detach().view(t.int32), kept[k].view(t.int32)), k
    finally:
        cb.close(); env.close()


# ------------------------------------------------------------------------------------------ 4. in the learn loop
N, T, LS, GS, BATCH, SEED = 33, 3, 50, 2, 16, 6
SIGMA = np.array([0.1, 0.2, 0.05], np.float32)
N_EVAL, EVAL_STEPS, EVAL_FREQ, EVAL_SEED = 20, 192, 2, 77


def _model(kind):
    """tests/offpolicy_train_ref.py's SAC / TD3 stand-in with the actor's mean moved to MEAN, so that evaluation episodes end with
    elements in them."""
    import torch
    m = TR.model(kind, learning_starts=LS, train_freq=T, gradient_steps=GS, batch_size=BATCH, buffer_size=64 * N, num_timesteps=0)
    head = m.actor.mu if kind == "sac" else m.actor.mu[-2]
    with torch.no_grad():
        head.weight.mul_(0.3)
        head.bias.copy_(torch.tensor(SCALED_MEAN))
    return m


def _slot_layout(res, targets):
    """An EvalResult back in the tally's slot layout: record k of env e (in step order) at offset[e] + k."""
    n, total = len(targets), int(targets.sum())
    offset = np.zeros(n, np.int32)
    offset[1:] = np.cumsum(targets)[:-1]
    count = np.zeros(n, np.int32)
    b = dict(target=targets, offset=offset, count=count, ep_return=np.full(max(total, 1), np.nan), ep_length=np.zeros(max(total, 1), np.int32),
             ep_flags=np.zeros(max(total, 1), np.int32), ep_n_elem=np.zeros(max(total, 1), np.int32))
    for i in np.lexsort((res.step, res.env)):
        e = res.env[i]
        s = offset[e] + count[e]
        b["ep_return"][s], b["ep_length"][s], b["ep_n_elem"][s] = res.reward[i], res.length[i], res.n_elements[i]
        b["ep_flags"][s] = int(res.complete[i]) | (2 if res.overflow[i] else 0)
        count[e] += 1
    return b, int((count < targets).sum())


def _same_training(a, b, ma, mb):
    import torch
    assert TR.differing(ma, mb) == []                                      # parameters, Adam moments and steps, targets, _n_updates
    assert ma.num_timesteps == mb.num_timesteps
    assert (a.buffer.pos, a.buffer.full, a.buffer.size()) == (b.buffer.pos, b.buffer.full, b.buffer.size())
    assert torch.equal(a.buffer.store.view(torch.int32), b.buffer.store.view(torch.int32))
    assert torch.equal(a.venv.obs.view(torch.int32), b.venv.obs.view(torch.int32))
    assert torch.equal(a.stats.state.view(torch.int64), b.stats.state.view(torch.int64))
    assert torch.equal(a.stats.carry_return.view(torch.int64), b.stats.carry_return.view(torch.int64))
    assert torch.equal(a.stats.carry_len, b.stats.carry_len)


@pytest.mark.parametrize("kind", ["sac", "td3"])
def test_learn_with_the_callback_equals_the_loop_cut_at_the_evaluations(kind):
    """eval_freq = 2 with train_freq = 3 and learning_starts = 50 of 33 envs: evaluations at n_calls = 2 (inside the first
    collect, whose first two steps are warm-up), 4 (inside the second), 6 (on its boundary), 8, 10, 12 -- the last two in a second
    learn().  SAC evaluates stochastically (the noise counter k * eval_steps under eval_seed), TD3 deterministically."""
    from reinforcementlearning4meshgeneration_amd import DeviceEvalCallback, FusedOffPolicyLearn
    from reinforcementlearning4meshgeneration_amd.eval_callback import eval_points, snapshot_set
    det = kind == "td3"
    sigma = SIGMA if kind == "td3" else None
    m = _model(kind)
    tw, plain = TR.twin(m), TR.twin(m)
    envs = [_env(N, log_capacity=0) for _ in range(3)]
    evals = [_env(N_EVAL) for _ in range(2)]
    targets = (1 + np.arange(N_EVAL) % 2).astype(np.int32)
    learn, twin, bare = (FusedOffPolicyLearn.from_sb3(x, e, action_noise_sigma=sigma) for x, e in zip((m, tw, plain), envs))
    cb = DeviceEvalCallback(evals[0], m, episodes_per_env=targets, eval_freq=EVAL_FREQ, eval_steps=EVAL_STEPS, deterministic=det,
                            eval_seed=EVAL_SEED, capacity=6)
    own = DeviceEvalCallback(envs[0], m, eval_freq=1, eval_steps=1)          # on the training env itself
    try:
        with pytest.raises(ValueError, match="is the training env"):
            learn.learn(99, seed=SEED, callback=own)
        assert m.num_timesteps == 0 and own.n_calls == 0
        own.close()
        # the device loop: two learn() calls, nothing read in between
        learn.learn(3 * 99, seed=SEED, callback=cb)
        assert cb.n_calls == 9 and cb.evaluations == 4
        learn.learn(99, seed=SEED, callback=cb)
        assert cb.n_calls == 12 and cb.evaluations == 6 and m.num_timesteps == 396
        with pytest.raises(ValueError, match="capacity = 6"):
            learn.learn(99, seed=SEED, callback=cb)                         # refused on the host: nothing enqueued, nothing counted
        assert cb.n_calls == 12 and m.num_timesteps == 396
        # the host loop: learn() cut in front of every collect
        ref, best, n_calls, k = ER.CallbackRef(), None, 0, 0
        kept_names = [name for name, _ in snapshot_set(tw)[1]]
        for _ in range(4):
            for j in eval_points(n_calls, T, EVAL_FREQ):
                res = evals[1].evaluate(twin.behaviour, episodes_per_env=targets, deterministic=det, seed=EVAL_SEED, counter=k * EVAL_STEPS,
                                        max_steps=EVAL_STEPS, check_every=1, quality=False)
                b, short = _slot_layout(res, targets)
                row, improved = ref.add(**b, short=short, num_timesteps=tw.num_timesteps + j * N)
                print(kind, "evaluation", k, "recorded", int(row[4]), "short", short, "mean", row[1], "improved", improved)
                if improved:
                    best = {name: x.detach().clone() for name, x in snapshot_set(tw)[1]}
                k += 1
            n_calls += T
            twin.learn(99, seed=SEED)
        bare.learn(3 * 99, seed=SEED)
        bare.learn(99, seed=SEED)
        got = cb.read(episodes=True)
        want = ref.history()
        assert got["evaluations"] == 6 == len(want) and got["timesteps"].tolist() == [66, 132, 198, 264, 330, 396]
        host = cb.history.cpu().numpy()
        for r in range(6):
            assert ER.bits(host[r]).tolist() == ER.bits(want[r]).tolist(), (r, host[r], want[r])
        assert ER.bits(cb.state.cpu().numpy()).tolist() == ER.bits(ref.state()).tolist()
        assert want[:, 4].max() > 0 and want[:, 8].sum() >= 1                 # episodes were recorded and a model was kept
        assert got["best_eval"] == ref.best_eval and got["best_mean_reward"] == ref.best_mean
        assert got["results"].shape == (6, int(targets.sum())) and np.array_equal(np.isfinite(got["results"]).sum(1), got["recorded"])
        kept = cb.best_state()
        assert list(kept) == kept_names
        for name in kept_names:
            assert kept[name].cpu().numpy().tobytes() == best[name].cpu().numpy().tobytes(), name
        # evaluation does not disturb training: the callback run, the cut run and the run without a callback end equal
        _same_training(learn, twin, m, tw)
        _same_training(learn, bare, m, plain)
    finally:
        cb.close()
        for x in (learn, twin, bare):
            x.close()
        for e in envs + evals:
            e.close()


# ------------------------------------------------------------------------------------------ 5. from the PPO loop
def test_evaluate_now_from_the_ppo_loop():
    import torch as t
    from reinforcementlearning4meshgeneration_amd import DeviceEvalCallback, FusedOnPolicyTrain, FusedPolicy
    from reinforcementlearning4meshgeneration_amd.eval_callback import snapshot_set
    t.manual_seed(0)
    model, _ = _ppo_model()
    model._n_updates = 0
    env, evals = _env(64, log_capacity=0), [_env(N_EVAL) for _ in range(2)]
    policy = FusedPolicy.from_sb3(model)
    policy.bind_live(model)
    tr = FusedOnPolicyTrain.from_sb3(model, policy)
    # stochastic, 512 steps: the noise of SPREAD ends episodes early and late (the polling loop of test 1 needs about 570 steps for
    # two episodes per env), so some are recorded and some envs stay short
    cb = DeviceEvalCallback(evals[0], model, n_eval_episodes=N_EVAL + 7, eval_freq=32, eval_steps=512, deterministic=False, capacity=2)
    try:
        env.reset()
        named = snapshot_set(model)[1]
        before = {k: x.detach().clone() for k, x in named}
        res = evals[1].evaluate(policy, n_eval_episodes=N_EVAL + 7, deterministic=False, seed=0, counter=0, max_steps=512, check_every=1,
                                quality=False)
        # one iteration of examples/ppo_train.py with the evaluation in front of its collect
        assert cb.evaluate_now(policy, 64 * 32) == 0
        out = env.collect_rollout(policy, 32, seed=0, counter=0, gamma=model.gamma, gae_lambda=model.gae_lambda)
        tr.train(out)
        b, short = _slot_layout(res, cb.targets)
        row, improved = ER.CallbackRef().add(**b, short=short, num_timesteps=64 * 32)
        print("ppo evaluation: recorded", int(row[4]), "short", short, "mean", row[1])
        got = cb.read()
        assert ER.bits(cb.history[0].cpu().numpy()).tolist() == ER.bits(row).tolist()
        assert improved and row[4] > 0 and got["improved"].tolist() == [True] and got["best_eval"] == 0 and got["timesteps"].tolist() == [2048]
        assert got["best_mean_reward"] == got["last_mean_reward"] == row[1] == got["mean_reward"][0]
        kept = cb.best_state()
        changed = 0
        for k, x in named:
            assert t.equal(kept[k].view(t.int32), before[k].view(t.int32)), k     # the parameters the evaluation ran with
            changed += int(not t.equal(x.detach(), before[k]))
        assert changed > 0                                                        # ... which train() has since moved
        with pytest.raises(ValueError, match="evaluated through an actor-critic FusedPolicy"):
            cb.evaluate_now(object(), 0)
        assert cb.evaluations == 1
    finally:
        cb.close(); tr.close(); policy.close(); env.close()
        for e in evals:
            e.close()
