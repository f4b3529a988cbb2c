"""GPU: DDPG's forward half (csrc/meshenv_wide.h: k_wide_policy, k_wide_target) against the fp64 restatements of
tests/ddpg_ref.py, every element of every output within its own bound; the in-kernel Philox noise against the host
restatements (tag 0 for the policy, tag 2 for the target); row independence; output subsets; live refresh; the
rollout -> replay -> sample -> target chain; and the eager torch statements a user writes today.

Weights: torch's default init, and a stress set (action head x 6 so that actions reach the clamps, rewards x 1e3).
Inputs: policy_ref.input_rows() / noise_rows().  Sizes: 1, 15, 16, 17, 33, R - 1, R, R + 1, 4101 with R = ddpg_ref.ROWS rows
per workgroup: tile edges, the last partial workgroup, a second row tile.  Each test prints max |kernel - fp64| / bound."""
import copy
import ctypes as C
import warnings

import numpy as np
import pytest

import ddpg_ref as D
import policy_ref as R
import rl_stubs
import td_target_ref as T

pytestmark = pytest.mark.gpu

NS = sorted({1, 15, 16, 17, 33, D.ROWS - 1, D.ROWS, D.ROWS + 1, 4101})
BS = sorted({1, 15, 16, 17, 100, 256, D.ROWS - 1, D.ROWS + 1, 4101})
SEED = (0x5EED << 32) | 77          # seeds and counters >= 2^32: both words of each reach the key / counter
COUNTER = (3 << 32) | 1000
NAN_BITS = 0x7FC0DEAD
SIGMA = D.SIGMA


@pytest.fixture(scope="module")
def inputs():
    obs = R.input_rows()
    n = max(NS)
    return np.ascontiguousarray(obs[:n]), R.noise_rows(n)


def _fmt(worst):
    return " ".join(f"{k}={v:.4f}" for k, v in sorted(worst.items()))


def _policy(model, sigma=SIGMA):
    from reinforcementlearning4meshgeneration_amd.policy import FusedPolicy
    return FusedPolicy.from_sb3(model, sigma=sigma)


def _target(model, noise=None):
    from reinforcementlearning4meshgeneration_amd.td_target import FusedTDTarget
    if noise is None:
        return FusedTDTarget.from_sb3(model)
    mu, q = model.actor_target.mu, model.critic_target.q_networks[0]
    return FusedTDTarget.ddpg([mu[0], mu[2]], mu[4], q, model.gamma, policy_noise=noise[0], noise_clip=noise[1])


def _batch(torch, obs, rew, done):
    return (torch.from_numpy(obs).cuda(), torch.from_numpy(rew).cuda().reshape(-1, 1), torch.from_numpy(done).cuda().reshape(-1, 1))


def _same(torch, a, b):
    return all(torch.equal(a[k], b[k]) for k in a) and set(a) == set(b)


# ----------------------------------------------------------------------------------------------------------- 3. policy
@pytest.mark.parametrize("stress", [False, True], ids=["default", "stress"])
def test_policy_against_fp64(stress, inputs):
    import torch
    obs_all, noise_all = inputs
    model = D.ddpg_model(head_scale=6.0 if stress else 1.0)
    layers = D.actor_layers(model)
    pol = _policy(D.to_cuda(copy.deepcopy(model)))
    assert pol.kind == "deterministic" and pol.spec.widths == (400, 300)
    worst, worst_eps, clamped = {}, 0.0, 0
    for n in NS:
        obs_np, noise_np = obs_all[:n], noise_all[:n]
        obs, noise = torch.from_numpy(obs_np).cuda(), torch.from_numpy(noise_np).cuda()
        what = f"{'stress' if stress else 'default'} n={n}"
        det = pol.forward(obs, deterministic=True)
        assert set(det) == {"actions", "buffer_actions"} and det["actions"].shape == (n, 3)
        ref = D.policy_forward(layers, obs_np, None)
        D.assert_all_within(det, ref, what + " deterministic", worst)
        clamped += R.check_clamps(det, ref)
        exp = pol.forward(obs, noise)
        ref = D.policy_forward(layers, obs_np, noise_np)
        D.assert_all_within(exp, ref, what + " noise", worst)
        clamped += R.check_clamps(exp, ref)
        smp = pol.sample(obs, SEED, COUNTER + n)
        eps = smp["eps"].cpu().numpy()
        worst_eps = max(worst_eps, R.assert_within(eps, R.philox_normal(SEED, COUNTER + n, np.arange(n)), what + " eps"))
        ref = D.policy_forward(layers, obs_np, eps)
        D.assert_all_within(smp, ref, what + " sampled", worst)
        clamped += R.check_clamps(smp, ref)
        replay = pol.forward(obs, smp["eps"])
        assert all(torch.equal(replay[k], smp[k]) for k in replay), what      # forward(obs, eps) replays sample bit for bit
        assert _same(torch, pol.forward(obs, noise), exp), what               # two identical launches
    if stress:
        assert clamped > 0
    print(f"\nddpg policy {'stress' if stress else 'default'}: max |kernel - fp64| / bound: {_fmt(worst)} eps={worst_eps:.4f}; "
          f"{clamped} clamped elements")
    pol.close()


# ----------------------------------------------------------------------------------------------------------- 4. rows
def test_rows_do_not_depend_on_the_launch(inputs):
    import torch
    obs_np, noise_np = inputs
    model = D.to_cuda(D.ddpg_model(head_scale=6.0))
    pol, td = _policy(model), _target(model, (0.2, 0.5))
    rew_np, done_np = T.batch_rows(4101, reward_scale=1e3)
    outs = []
    for n in (17, 4101):
        obs, rew, done = _batch(torch, obs_np[:n], rew_np[:n], done_np[:n])
        noise = torch.from_numpy(noise_np[:n]).cuda()
        a = pol.forward(obs, noise)
        y, parts = td.target(next_observations=obs, rewards=rew, dones=done, noise=noise, return_parts=True)
        outs.append(dict(a, target=y, **parts))
    for k in outs[0]:
        assert torch.equal(outs[1][k][:17], outs[0][k]), k
    pol.close(); td.close()


# ----------------------------------------------------------------------------------------------------------- 5. subsets
@pytest.mark.parametrize("n", [17, 4101])
def test_policy_output_subsets(n, inputs):
    import torch

    from reinforcementlearning4meshgeneration_amd import _capi
    L = _capi.load()
    pol = _policy(D.to_cuda(D.ddpg_model(head_scale=6.0)))
    obs = torch.from_numpy(inputs[0][:n]).cuda()
    names = ["actions", "buffer_actions", "eps"]

    def launch(req, extra=(None, None)):
        bufs = {k: torch.full((n + 32, 3), NAN_BITS, dtype=torch.int32, device="cuda") for k in names}
        ptr = lambda k: bufs[k][16:16 + n].data_ptr() if k in req else None   # noqa: E731
        pol._bind_stream()
        rc = L.meshenv_policy_forward(pol._h, n, obs.data_ptr(), None, 1, C.c_uint64(SEED), C.c_uint64(COUNTER), ptr("actions"),
                                      ptr("buffer_actions"), extra[0], extra[1], ptr("eps"))
        torch.cuda.synchronize()
        return rc, bufs

    rc, full = launch(names)
    assert rc == 0, L.meshenv_policy_last_error(pol._h)
    for k in names:
        assert (full[k][:16] == NAN_BITS).all() and (full[k][16 + n:] == NAN_BITS).all(), k
        assert not (full[k][16:16 + n] == NAN_BITS).any(), k
    for req in names:
        rc, got = launch([req])
        assert rc == 0
        for k in names:
            assert torch.equal(got[k], full[k]) if k == req else (got[k] == NAN_BITS).all(), (req, k)
    scratch = torch.empty(n, device="cuda")
    for extra in ((scratch.data_ptr(), None), (None, scratch.data_ptr())):            # log_prob, value
        rc, got = launch(names, extra)
        assert rc == _capi.E_ARG and b"no log_prob / value" in L.meshenv_policy_last_error(pol._h)
        assert all((got[k] == NAN_BITS).all() for k in names)
    pol.close()


@pytest.mark.parametrize("B", [17, 4101])
def test_target_output_subsets(B, inputs):
    import torch

    from reinforcementlearning4meshgeneration_amd import _capi
    L = _capi.load()
    td = _target(D.to_cuda(D.ddpg_model(head_scale=6.0)), (0.2, 0.5))
    rew_np, done_np = T.batch_rows(B)
    obs, rew, done = _batch(torch, inputs[0][:B], rew_np, done_np)
    widths = dict(target=1, next_actions=3, q1=1, eps=3)
    names = list(widths)

    def launch(req, q2=None, lp=None):
        bufs = {k: torch.full((B + 32, w), NAN_BITS, dtype=torch.int32, device="cuda") for k, w in widths.items()}
        ptr = lambda k: bufs[k][16:16 + B].data_ptr() if k in req else None   # noqa: E731
        td._bind_stream()
        rc = L.meshenv_target_forward(td._h, B, obs.data_ptr(), rew.data_ptr(), done.data_ptr(), None, 1, C.c_uint64(SEED),
                                      C.c_uint64(COUNTER), ptr("target"), ptr("next_actions"), lp, ptr("q1"), q2, ptr("eps"))
        torch.cuda.synchronize()
        return rc, bufs

    rc, full = launch(names)
    assert rc == 0, L.meshenv_target_last_error(td._h)
    for k in names:
        assert (full[k][:16] == NAN_BITS).all() and (full[k][16 + B:] == NAN_BITS).all(), k
        assert not (full[k][16:16 + B] == NAN_BITS).any(), k
    for req in names:
        rc, got = launch([req])
        assert rc == 0
        for k in names:
            assert torch.equal(got[k], full[k]) if k == req else (got[k] == NAN_BITS).all(), (req, k)
    scratch = torch.empty(B, device="cuda")
    rc, got = launch(names, q2=scratch.data_ptr())
    assert rc == _capi.E_ARG and b"no q2" in L.meshenv_target_last_error(td._h) and all((got[k] == NAN_BITS).all() for k in names)
    rc, got = launch(names, lp=scratch.data_ptr())
    assert rc == _capi.E_ARG and b"next_log_prob" in L.meshenv_target_last_error(td._h)
    y, parts = td.target(next_observations=obs, rewards=rew, dones=done, seed=SEED, counter=COUNTER, return_parts=True)
    assert set(parts) == {"next_actions", "q1", "eps"} and torch.equal(y.view(torch.int32), full["target"][16:16 + B])
    # a second critic is refused where the tensors are bound
    s = td.spec
    rc = L.meshenv_target_bind(td._h, td._ptrs(s.actor), 6, td._ptrs(s.q1), td._ptrs(s.q1), 6, None)
    assert rc == _capi.E_ARG and b"one critic" in L.meshenv_target_last_error(td._h)
    td.close()


# ----------------------------------------------------------------------------------------------------------- 6. refresh
def _perturb(torch, model):
    with torch.no_grad():
        for i, p in enumerate(D.live_tensors(model)):
            p.add_(0.01 * (1 + i % 3))


def test_policy_refresh_reads_the_live_parameters(inputs):
    import torch
    n = 1000
    model = D.to_cuda(D.ddpg_model())
    pol = _policy(model)
    obs, noise = torch.from_numpy(inputs[0][:n]).cuda(), torch.from_numpy(inputs[1][:n]).cuda()
    loaded = pol.forward(obs, noise)
    pol.bind_live(model)
    pol.refresh()
    assert _same(torch, pol.forward(obs, noise), loaded)            # the same parameters through the device pack
    _perturb(torch, model)
    assert _same(torch, pol.forward(obs, noise), loaded)            # no refresh: the old snapshot
    pol.refresh()
    new = pol.forward(obs, noise)
    assert not torch.equal(new["buffer_actions"], loaded["buffer_actions"])
    fresh = _policy(model)
    assert _same(torch, fresh.forward(obs, noise), new)             # bit-equal to a fresh load of the changed parameters
    D.assert_all_within(new, D.policy_forward(D.actor_layers(model), inputs[0][:n], inputs[1][:n]), "refreshed policy")
    td3 = rl_stubs.td3_model()
    for part in (td3.actor, td3.actor_target):
        part.mu = part.mu.cuda()
    with pytest.raises(ValueError, match=r"\[256, 256\].*\[400, 300\]"):
        pol.bind_live(td3)
    pol256 = _policy(td3)
    with pytest.raises(ValueError, match=r"\[400, 300\].*\[256, 256\]"):
        pol256.bind_live(model)
    pol.close(); fresh.close(); pol256.close()


def test_target_refresh_reads_the_live_parameters(inputs):
    import torch
    B = 1000
    model = D.to_cuda(D.ddpg_model())
    td = _target(model, (0.2, 0.5))
    obs_np, eps_np = inputs[0][:B], inputs[1][:B]
    rew_np, done_np = T.batch_rows(B)
    obs, rew, done = _batch(torch, obs_np, rew_np, done_np)
    eps = torch.from_numpy(eps_np).cuda()
    old = td.target(next_observations=obs, rewards=rew, dones=done, noise=eps)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        _perturb(torch, model)
        stale = td.target(next_observations=obs, rewards=rew, dones=done, noise=eps)       # no refresh: the old snapshot
        td.refresh()                                                                        # no synchronise in between
        y, parts = td.target(next_observations=obs, rewards=rew, dones=done, noise=eps, return_parts=True)
    s.synchronize()
    assert torch.equal(stale, old) and not torch.equal(y, old)
    worst = {}
    ref = D.target(D.actor_layers(model, target=True), D.critic_layers(model), obs_np, rew_np, done_np, eps_np,
                   policy_noise=0.2, noise_clip=0.5)
    D.assert_all_within(dict(parts, target=y), ref, "refreshed target", worst)
    fresh = _target(model, (0.2, 0.5))
    y2, parts2 = fresh.target(next_observations=obs, rewards=rew, dones=done, noise=eps, return_parts=True)
    assert torch.equal(y2, y) and _same(torch, parts2, parts)
    print(f"\nddpg target refreshed on a side stream: max |kernel - fp64| / bound: {_fmt(worst)}")
    td.close(); fresh.close()


# ----------------------------------------------------------------------------------------------------------- 7. target
@pytest.mark.parametrize("noise", [(0.1, 0.0), (0.2, 0.5)], ids=["ddpg_constants", "noise_0.2_0.5"])
@pytest.mark.parametrize("stress", [False, True], ids=["default", "stress"])
def test_target_against_fp64(stress, noise, inputs):
    import torch
    obs_all, noise_all = inputs
    model = D.ddpg_model(head_scale=6.0 if stress else 1.0)
    actor, critic = D.actor_layers(model, target=True), D.critic_layers(model)
    td = _target(D.to_cuda(copy.deepcopy(model)), None if noise == (0.1, 0.0) else noise)
    assert td.kind == "ddpg" and (td.spec.policy_noise, td.spec.noise_clip) == noise
    kw = dict(gamma_=0.99, policy_noise=noise[0], noise_clip=noise[1])
    worst, worst_eps = {}, 0.0
    for B in BS:
        obs_np, noise_np = obs_all[:B], noise_all[:B]
        rew_np, done_np = T.batch_rows(B, reward_scale=1e3 if stress else 1.0, done_p=0.3 if stress else 0.2)
        obs, rew, done = _batch(torch, obs_np, rew_np, done_np)
        what = f"{'stress' if stress else 'default'} {noise} B={B}"
        y, parts = td.target(next_observations=obs, rewards=rew, dones=done, return_parts=True)
        assert set(parts) == {"next_actions", "q1"} and y.shape == (B, 1)
        D.assert_all_within(dict(parts, target=y), D.target(actor, critic, obs_np, rew_np, done_np, None, **kw), what + " eps=0", worst)
        y, parts = td.target(next_observations=obs, rewards=rew, dones=done, noise=torch.from_numpy(noise_np).cuda(), return_parts=True)
        assert torch.equal(parts["eps"].cpu(), torch.from_numpy(noise_np))
        D.assert_all_within(dict(parts, target=y), D.target(actor, critic, obs_np, rew_np, done_np, noise_np, **kw), what + " noise", worst)
        y, parts = td.target(next_observations=obs, rewards=rew, dones=done, seed=SEED, counter=COUNTER + B, return_parts=True)
        eps = parts["eps"].cpu().numpy()
        worst_eps = max(worst_eps, R.assert_within(eps, T.philox_normal(SEED, COUNTER + B, np.arange(B)), what + " eps"))
        D.assert_all_within(dict(parts, target=y), D.target(actor, critic, obs_np, rew_np, done_np, eps, **kw), what + " sampled", worst)
        y2, parts2 = td.target(next_observations=obs, rewards=rew, dones=done, noise=parts["eps"], return_parts=True)
        assert torch.equal(y2, y) and _same(torch, parts2, parts), what
        assert torch.equal(y[done != 0], rew[done != 0]), what      # (1 - done) = 0: the reward itself
    print(f"\nddpg target {'stress' if stress else 'default'} {noise}: max |kernel - fp64| / bound: {_fmt(worst)} eps={worst_eps:.4f}")
    td.close()


# ----------------------------------------------------------------------------------------------------------- 8. the chain
def test_rollout_replay_sample_target():
    import torch
    from reinforcementlearning4meshgeneration_amd import DeviceReplayBuffer, MeshVecEnv, boundary, evaluate_policy
    n, steps, B = 64, 8, 256
    model = D.to_cuda(D.ddpg_model())
    pol, td = _policy(model, sigma=0.1), _target(model)
    env = MeshVecEnv([boundary(0)], n_envs=n)
    buf = DeviceReplayBuffer(env, buffer_size=n * 16)
    env.reset_tensor()
    out = env.collect_rollout(pol, steps, seed=5, counter=0)
    assert buf.add_rollout(out) == steps
    assert torch.equal(buf.actions[:steps], out["buffer_actions"])        # what ReplayBuffer stores: the [-1, 1] action, bit for bit
    samples, rows_d, envs_d = buf.sample(B, seed=9, counter=COUNTER, return_indices=True)
    y, parts = td.target(samples, seed=9, counter=COUNTER, return_parts=True)
    rows_i, envs_i = rows_d.cpu().numpy(), envs_d.cpu().numpy()
    nxt = buf.next_observations.cpu().numpy()[rows_i, envs_i]
    rew = buf.rewards.cpu().numpy()[rows_i, envs_i]
    done = (buf.dones.cpu().numpy() * (1.0 - buf.timeouts.cpu().numpy()))[rows_i, envs_i].astype(np.float32)
    assert np.array_equal(nxt, samples.next_observations.cpu().numpy()) and np.array_equal(rew, samples.rewards.cpu().numpy()[:, 0])
    eps = parts["eps"].cpu().numpy()
    R.assert_within(eps, T.philox_normal(9, COUNTER, np.arange(B)), "eps")
    worst = {}
    ref = D.target(D.actor_layers(model, target=True), D.critic_layers(model), nxt, rew, done, eps)
    D.assert_all_within(dict(parts, target=y), ref, "chain", worst)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)               # (an untrained actor may run into max_steps)
        res = env.evaluate(pol, n_eval_episodes=n, max_steps=400, quality=False)
        mean, std = evaluate_policy(model, env, n_eval_episodes=n, warn=False)
    assert np.isfinite(res.mean_reward) and np.isfinite(mean) and np.isfinite(std)
    print(f"\nddpg chain ({n} envs x {steps} steps, batch {B}): max |kernel - fp64| / bound: {_fmt(worst)}")
    pol.close(); td.close(); env.close()


# ----------------------------------------------------------------------------------------------------------- 9. eager torch
def eager_policy(torch, model, obs, eps, sigma=SIGMA):
    low, high = torch.from_numpy(R.ACTION_LOW).cuda(), torch.from_numpy(R.ACTION_HIGH).cuda()
    with torch.no_grad():
        s = torch.clamp(model.actor.mu(obs) + sigma * eps, -1, 1)
        return low + 0.5 * (s + 1.0) * (high - low), s


def eager_target(torch, model, obs, rew, done, eps, policy_noise=0.1, noise_clip=0.0):
    """SB3's TD3.train block on the stand-in's modules (n_critics = 1)."""
    with torch.no_grad():
        noise = (policy_noise * eps).clamp(-noise_clip, noise_clip)
        next_actions = (model.actor_target.mu(obs) + noise).clamp(-1, 1)
        qin = torch.cat([obs, next_actions], dim=1)
        q = torch.cat(tuple(qn(qin) for qn in model.critic_target.q_networks), dim=1)
        q, _ = torch.min(q, dim=1, keepdim=True)
        return rew + (1 - done) * model.gamma * q


@pytest.mark.parametrize("n", [100, 4101])
def test_against_eager_torch(n, inputs):
    """Fused against the eager fp32 statements fed the same eps: within 2 x bound elementwise, both within bound of fp64."""
    import torch
    model = D.to_cuda(D.ddpg_model())
    pol, td = _policy(model), _target(model, (0.2, 0.5))
    obs_np, eps_np = inputs[0][:n], inputs[1][:n]
    rew_np, done_np = T.batch_rows(n)
    obs, rew, done = _batch(torch, obs_np, rew_np, done_np)
    eps = torch.from_numpy(eps_np).cuda()
    fused = pol.forward(obs, eps)
    e_act, e_ba = eager_policy(torch, model, obs, eps)
    ref = D.policy_forward(D.actor_layers(model), obs_np, eps_np)
    y = td.target(next_observations=obs, rewards=rew, dones=done, noise=eps)
    e_y = eager_target(torch, model, obs, rew, done, eps, 0.2, 0.5)
    tref = D.target(D.actor_layers(model, target=True), D.critic_layers(model), obs_np, rew_np, done_np, eps_np, policy_noise=0.2, noise_clip=0.5)
    for name, f, e, rb in (("actions", fused["actions"], e_act, ref["actions"]), ("buffer_actions", fused["buffer_actions"], e_ba, ref["buffer_actions"]),
                           ("target", y[:, 0], e_y[:, 0], tref["target"])):
        f, e = f.cpu().numpy(), e.cpu().numpy()
        r_fused, r_eager = R.assert_within(f, rb, f"fused {name}"), R.assert_within(e, rb, f"eager {name}")
        r_pair, bad = R.ratio(f, (e.astype(np.float64), 2.0 * rb[1]))
        print(f"\nddpg {name} n={n}: |fused - fp64| / bound {r_fused:.4f}, |eager - fp64| / bound {r_eager:.4f}, "
              f"|fused - eager| / (2 bound) {r_pair:.4f}")
        assert not bad.any(), name
    pol.close(); td.close()
