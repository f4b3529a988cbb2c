"""GPU: the fused SAC / TD3 TD target (csrc/meshenv_target.h: k_td_target<SAC>, k_td_target<TD3>, k_target_pack) against
the fp64 restatement of tests/td_target_ref.py, every element of every output within its own bound; the in-kernel Philox
noise (tag 2) against the host restatement; output subsets; refresh from live parameters on a side stream; the whole
rollout -> replay -> sample -> target chain; and the eager torch block a user writes today.

Weights: torch's default init, and a stress set (SAC: action head x 6, log_std bias +40 / -40; TD3: action head x 6).
Inputs: policy_ref.input_rows() (repeated beyond its 5028 rows) and noise_rows().  Each test prints
max |kernel - fp64| / bound per output."""
import copy
import ctypes as C

import numpy as np
import pytest

import policy_ref as R
import td_target_ref as T

pytestmark = pytest.mark.gpu

BS = (1, 15, 16, 17, 100, 256, 4101, 65536)
GAMMA = 0.99
SEED = (0x5EED << 32) | 77          # seeds and counters >= 2^32: both words of each reach the key / counter
COUNTER = (3 << 32) | 1000
NAN_BITS = 0x7FC0DEAD


@pytest.fixture(scope="module")
def inputs():
    obs = R.input_rows()
    n = max(BS)
    obs = np.ascontiguousarray(np.resize(obs, (n, 18)))
    return obs, R.noise_rows(n)


def _modules(kind, stress):
    if kind == "sac":
        return T.sac_modules(stress=stress)
    return T.td3_modules(head_scale=6.0 if stress else 1.0)


def _cuda(m):
    out = {}
    for k, v in m.items():
        if isinstance(v, list):
            out[k] = [copy.deepcopy(l).cuda() for l in v]
        else:
            out[k] = copy.deepcopy(v).cuda() if hasattr(v, "weight") else v
    return out


def _fused(mc, log_ent_coef=None, ent_coef=None):
    from reinforcementlearning4meshgeneration_amd.td_target import FusedTDTarget
    if mc["kind"] == "sac":
        return FusedTDTarget.sac(mc["lin"], mc["mu"], mc["ls"], mc["q1"], mc["q2"], GAMMA, log_ent_coef=log_ent_coef, ent_coef=ent_coef)
    return FusedTDTarget.td3(mc["lin"], mc["mu"], mc["q1"], mc["q2"], GAMMA, policy_noise=0.2, noise_clip=0.5)


def _kw(kind, lec):
    return dict(gamma_=GAMMA, log_ent_coef=np.float32(lec)) if kind == "sac" else dict(gamma_=GAMMA, policy_noise=0.2, noise_clip=0.5)


def _fmt(worst):
    return " ".join(f"{k}={v:.4f}" for k, v in sorted(worst.items()))


def _batch(torch, obs, rew, done):
    return (torch.from_numpy(obs).cuda(), torch.from_numpy(rew).cuda().reshape(-1, 1), torch.from_numpy(done).cuda().reshape(-1, 1))


def _got(y, parts):
    return dict(parts, target=y)


# ----------------------------------------------------------------------------------------------------------- 1. fp64
@pytest.mark.parametrize("stress", [False, True], ids=["default", "stress"])
@pytest.mark.parametrize("kind", ["sac", "td3"])
def test_target_against_fp64(kind, stress, inputs):
    import torch
    obs_all, noise_all = inputs
    m = _modules(kind, stress)
    lec = 1.0 if stress else -3.0
    lec_dev = torch.tensor([lec], dtype=torch.float32, device="cuda") if kind == "sac" else None
    td = _fused(_cuda(m), log_ent_coef=lec_dev)
    kw = _kw(kind, lec)
    worst, worst_eps = {}, 0.0
    for B in BS:
        if stress and B > 4101:
            continue            # the stress weights run up to 4101 rows; every B and every noise mode runs on the default ones
        obs_np, noise_np = obs_all[:B], noise_all[:B]
        rew_np, done_np = T.batch_rows(B, reward_scale=1e3 if stress else 1.0, done_p=0.3 if stress else 0.2)
        obs, rew, done = _batch(torch, obs_np, rew_np, done_np)
        what = f"{kind} {'stress' if stress else 'default'} B={B}"
        y, parts = td.target(next_observations=obs, rewards=rew, dones=done, return_parts=True)
        assert "eps" not in parts and y.shape == (B, 1)
        T.assert_all_within(_got(y, parts), T.target_ref(m, obs_np, rew_np, done_np, None, **kw), what + " eps=0", worst)
        y, parts = td.target(next_observations=obs, rewards=rew, dones=done, noise=torch.from_numpy(noise_np).cuda(), return_parts=True)
        assert torch.equal(parts["eps"].cpu(), torch.from_numpy(noise_np))
        T.assert_all_within(_got(y, parts), T.target_ref(m, obs_np, rew_np, done_np, noise_np, **kw), what + " noise", worst)
        y, parts = td.target(next_observations=obs, rewards=rew, dones=done, seed=SEED, counter=COUNTER + B, return_parts=True)
        eps = parts["eps"].cpu().numpy()
        worst_eps = max(worst_eps, R.assert_within(eps, T.philox_normal(SEED, COUNTER + B, np.arange(B)), what + " eps"))
        T.assert_all_within(_got(y, parts), T.target_ref(m, obs_np, rew_np, done_np, eps, **kw), what + " sampled", worst)
        y2, parts2 = td.target(next_observations=obs, rewards=rew, dones=done, noise=parts["eps"], return_parts=True)
        assert torch.equal(y2, y), what
        for k in parts:
            assert torch.equal(parts2[k], parts[k]), (what, k)
        assert torch.equal(td.target(next_observations=obs, rewards=rew, dones=done, seed=SEED, counter=COUNTER + B), y)
        assert torch.equal(y[done != 0], rew[done != 0]), what      # (1 - done) = 0: the reward itself
    print(f"\ntd target {kind} {'stress' if stress else 'default'}: max |kernel - fp64| / bound: {_fmt(worst)} eps={worst_eps:.4f}")
    td.close()


def test_noise_stream_is_the_kernels_own(inputs):
    """The same (seed, counter) gives another stream than FusedActor.sample (tag 0) and than the replay draw's words (tag 1)."""
    import torch
    from reinforcementlearning4meshgeneration_amd.actor import FusedActor
    B = 4101
    m = T.sac_modules()
    td = _fused(_cuda(m), ent_coef=0.1)
    obs_np = inputs[0][:B]
    rew_np, done_np = T.batch_rows(B)
    obs, rew, done = _batch(torch, obs_np, rew_np, done_np)
    _, parts = td.target(next_observations=obs, rewards=rew, dones=done, seed=SEED, counter=COUNTER, return_parts=True)
    eps = parts["eps"].cpu().numpy()
    actor = FusedActor.from_torch(m["lin"], m["mu"], m["ls"])
    eps_actor = torch.empty((B, 3), dtype=torch.float32, device="cuda")
    actor.sample(obs, SEED, COUNTER, eps_out=eps_actor)
    assert (eps_actor.cpu().numpy() != eps).mean() > 0.999
    idx = np.arange(B)
    R.assert_within(eps, T.philox_normal(SEED, COUNTER, idx), "tag 2")
    R.assert_within(eps_actor.cpu().numpy(), R.philox_normal(SEED, COUNTER, idx), "tag 0")
    for tag in (0, 1):
        other = T._normal(T.philox_words(SEED, COUNTER, idx, tag))
        assert R.ratio(eps, other)[1].mean() > 0.999, tag
    td.close()


# ----------------------------------------------------------------------------------------------------------- 2. subsets
@pytest.mark.parametrize("B", [17, 4101])
@pytest.mark.parametrize("kind", ["sac", "td3"])
def test_output_subsets(kind, B, inputs):
    """meshenv_target_forward with each single output and with all of them (sampled noise): every requested output bit-equal
    to the all-outputs launch; 16 guard rows on either side and every buffer not requested keep their NaN bit pattern."""
    import torch

    from reinforcementlearning4meshgeneration_amd import _capi
    L = _capi.load()
    m = _modules(kind, True)
    td = _fused(_cuda(m), ent_coef=0.1 if kind == "sac" else None)
    rew_np, done_np = T.batch_rows(B)
    obs, rew, done = _batch(torch, inputs[0][:B], rew_np, done_np)
    widths = dict(target=1, next_actions=3, next_log_prob=1, q1=1, q2=1, eps=3)
    if kind == "td3":
        del widths["next_log_prob"]
    names = list(widths)
    subsets = [(k,) for k in names] + [tuple(names)]

    def launch(req):
        bufs = {k: torch.full((B + 32, w), NAN_BITS, dtype=torch.int32, device="cuda") for k, w in widths.items()}
        ptr = lambda k: bufs[k][16:16 + B].data_ptr() if k in req else None   # noqa: E731
        td._bind_stream()
        rc = L.meshenv_target_forward(td._h, B, obs.data_ptr(), rew.data_ptr(), done.data_ptr(), None, 1, C.c_uint64(SEED),
                                      C.c_uint64(COUNTER), ptr("target"), ptr("next_actions"), ptr("next_log_prob"), ptr("q1"),
                                      ptr("q2"), ptr("eps"))
        assert rc == 0, L.meshenv_target_last_error(td._h)
        torch.cuda.synchronize()
        return bufs

    full = launch(subsets[-1])
    for k in names:
        assert (full[k][:16] == NAN_BITS).all() and (full[k][16 + B:] == NAN_BITS).all(), k
        assert not (full[k][16:16 + B] == NAN_BITS).any(), k
    for req in subsets[:-1]:
        got = launch(req)
        for k in names:
            if k in req:
                assert torch.equal(got[k], full[k]), (req, k)
            else:
                assert (got[k] == NAN_BITS).all(), (req, k)
    # refusals of the C entry point
    rc = L.meshenv_target_forward(td._h, B, obs.data_ptr(), None, None, None, 1, C.c_uint64(0), C.c_uint64(0),
                                  full["target"].data_ptr(), None, None, None, None, None)
    assert rc == _capi.E_ARG and b"rewards_dev" in L.meshenv_target_last_error(td._h)
    rc = L.meshenv_target_forward(td._h, B, obs.data_ptr(), rew.data_ptr(), done.data_ptr(), None, 0, C.c_uint64(0), C.c_uint64(0),
                                  None, None, None, None, None, None)
    assert rc == _capi.E_ARG and b"no output" in L.meshenv_target_last_error(td._h)
    td.close()


# ----------------------------------------------------------------------------------------------------------- 3. refresh
@pytest.mark.parametrize("kind", ["sac", "td3"])
def test_refresh_reads_the_live_parameters(kind, inputs):
    import torch
    B = 1000
    m = _modules(kind, False)
    mc = _cuda(m)
    other = _cuda(_modules(kind, True))          # the "online" networks a Polyak step mixes in
    lec = torch.tensor([-3.0], dtype=torch.float32, device="cuda") if kind == "sac" else None
    td = _fused(mc, log_ent_coef=lec)
    obs_np, eps_np = inputs[0][:B], inputs[1][:B]
    rew_np, done_np = T.batch_rows(B)
    obs, rew, done = _batch(torch, obs_np, rew_np, done_np)
    eps = torch.from_numpy(eps_np).cuda()
    old = td.target(next_observations=obs, rewards=rew, dones=done, noise=eps)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s), torch.no_grad():
        for key in ("lin", "q1", "q2"):
            for p_l, q_l in zip(mc[key], other[key]):
                for p, q in ((p_l.weight, q_l.weight), (p_l.bias, q_l.bias)):
                    p.data.mul_(0.995).add_(0.005 * q.data)
        for key in ("mu", "ls"):
            if key in mc:
                mc[key].weight.data.mul_(0.995).add_(0.005 * other[key].weight.data)
                mc[key].bias.data.mul_(0.995).add_(0.005 * other[key].bias.data)
        if lec is not None:
            lec.add_(0.75)
        stale = td.target(next_observations=obs, rewards=rew, dones=done, noise=eps)       # no refresh: the old snapshot
        td.refresh()                                                                        # no synchronise in between
        y, parts = td.target(next_observations=obs, rewards=rew, dones=done, noise=eps, return_parts=True)
    s.synchronize()
    assert torch.equal(stale, old)
    assert not torch.equal(y, old)
    m_new = {k: ([copy.deepcopy(l).cpu() for l in v] if isinstance(v, list) else (copy.deepcopy(v).cpu() if hasattr(v, "weight") else v))
             for k, v in mc.items()}
    kw = _kw(kind, 0.0)
    if kind == "sac":
        kw["log_ent_coef"] = lec.cpu().numpy()[0]
        assert kw["log_ent_coef"] == np.float32(-2.25)
    worst = {}
    T.assert_all_within(_got(y, parts), T.target_ref(m_new, obs_np, rew_np, done_np, eps_np, **kw), f"{kind} refreshed", worst)
    fresh = _fused(_cuda(m_new), log_ent_coef=lec.clone() if lec is not None else None)
    y2, parts2 = fresh.target(next_observations=obs, rewards=rew, dones=done, noise=eps, return_parts=True)
    assert torch.equal(y2, y)
    for k in parts:
        assert torch.equal(parts2[k], parts[k]), k
    print(f"\ntd target {kind} refreshed on a side stream: max |kernel - fp64| / bound: {_fmt(worst)}")
    fresh.close()
    td.close()


# ----------------------------------------------------------------------------------------------------------- 4. end to end
def test_rollout_replay_sample_target():
    import torch
    from reinforcementlearning4meshgeneration_amd import DeviceReplayBuffer, MeshVecEnv, boundary
    from reinforcementlearning4meshgeneration_amd.actor import FusedActor
    n, steps, B = 4096, 128, 256
    m = T.sac_modules()
    mc = _cuda(m)
    lec = torch.tensor([-1.5], dtype=torch.float32, device="cuda")
    td = _fused(mc, log_ent_coef=lec)
    actor = FusedActor.from_torch(m["lin"], m["mu"], m["ls"])
    env = MeshVecEnv([boundary(0)], n_envs=n)
    buf = DeviceReplayBuffer(env, buffer_size=n * 128)
    obs0 = env.reset_tensor().clone()
    acts = actor.sample(obs0, 5, 0)
    out = env.step_actor_T(actor, acts, steps, seed=5, counter=1, want_terminal_obs=True)
    buf.add_rollout(out, obs0=obs0)
    samples, rows_d, envs_d = buf.sample(B, seed=9, counter=COUNTER, return_indices=True)
    y, parts = td.target(samples, seed=9, counter=COUNTER, return_parts=True)
    # the host copies, gathered at the drawn indices
    rows_i, envs_i = rows_d.cpu().numpy(), envs_d.cpu().numpy()
    nxt = buf.next_observations.cpu().numpy()[rows_i, envs_i]
    rew = buf.rewards.cpu().numpy()[rows_i, envs_i]
    done = (buf.dones.cpu().numpy() * (1.0 - buf.timeouts.cpu().numpy()))[rows_i, envs_i].astype(np.float32)
    assert np.array_equal(nxt, samples.next_observations.cpu().numpy()) and np.array_equal(rew, samples.rewards.cpu().numpy()[:, 0])
    assert np.array_equal(done, samples.dones.cpu().numpy()[:, 0])
    eps = parts["eps"].cpu().numpy()
    R.assert_within(eps, T.philox_normal(9, COUNTER, np.arange(B)), "eps")
    worst = {}
    ref = T.sac_target(m, nxt, rew, done, eps, GAMMA, log_ent_coef=np.float32(-1.5))
    T.assert_all_within(_got(y, parts), ref, "end to end", worst)
    # a batch with terminal transitions: dones == 1 rows give the reward exactly
    d_all = buf.dones[:steps] * (1.0 - buf.timeouts[:steps])
    idx = torch.nonzero(d_all != 0)[:64]
    assert len(idx) > 0, "no terminal transition in the rollout"
    term = buf.gather(idx[:, 0].to(torch.int32).contiguous(), idx[:, 1].to(torch.int32).contiguous())
    yt = td.target(term, seed=9, counter=COUNTER + 1)
    assert torch.equal(yt, term.rewards)
    print(f"\ntd target end to end ({n} envs x {steps} steps, batch {B}): max |kernel - fp64| / bound: {_fmt(worst)}; "
          f"{int((done != 0).sum())} terminal rows in the batch, {len(idx)} gathered")
    td.close()
    env.close()


# ----------------------------------------------------------------------------------------------------------- 5. eager torch
def _eager(torch, mc, obs, rew, done, eps, ent_coef=None):
    """The block a user writes today, fp32 on the device (SB3's statements on stand-in modules)."""
    relu = torch.relu
    with torch.no_grad():
        def mlp(layers, x):
            for l in layers[:-1]:
                x = relu(l(x))
            return layers[-1](x)
        if mc["kind"] == "sac":
            latent = obs
            for l in mc["lin"]:
                latent = relu(l(latent))
            mean, log_std = mc["mu"](latent), torch.clamp(mc["ls"](latent), -20, 2)
            std = log_std.exp()
            gaussian = mean + std * eps
            next_actions = torch.tanh(gaussian)
            lp = torch.distributions.Normal(mean, std).log_prob(gaussian).sum(dim=1)
            lp -= torch.sum(torch.log(1 - next_actions ** 2 + 1e-6), dim=1)
        else:
            noise = (0.2 * eps).clamp(-0.5, 0.5)
            next_actions = (torch.tanh(mlp(mc["lin"] + [mc["mu"]], obs)) + noise).clamp(-1, 1)
        qin = torch.cat([obs, next_actions], dim=1)
        q = torch.cat((mlp(mc["q1"], qin), mlp(mc["q2"], qin)), dim=1)
        q, _ = torch.min(q, dim=1, keepdim=True)
        if mc["kind"] == "sac":
            q = q - ent_coef * lp.reshape(-1, 1)
        return rew + (1 - done) * GAMMA * q


@pytest.mark.parametrize("B", [100, 4101])
@pytest.mark.parametrize("kind", ["sac", "td3"])
def test_against_eager_torch(kind, B, inputs):
    """Fused against the eager fp32 block fed the same eps: within 2 x bound elementwise (both within bound of fp64)."""
    import torch
    m = _modules(kind, False)
    mc = _cuda(m)
    lec = torch.tensor([-3.0], dtype=torch.float32, device="cuda") if kind == "sac" else None
    td = _fused(mc, log_ent_coef=lec)
    obs_np, eps_np = inputs[0][:B], inputs[1][:B]
    rew_np, done_np = T.batch_rows(B)
    obs, rew, done = _batch(torch, obs_np, rew_np, done_np)
    eps = torch.from_numpy(eps_np).cuda()
    y = td.target(next_observations=obs, rewards=rew, dones=done, noise=eps).cpu().numpy()[:, 0]
    e = _eager(torch, mc, obs, rew, done, eps, torch.exp(lec.detach()) if lec is not None else None).cpu().numpy()[:, 0]
    ref, bound = T.target_ref(m, obs_np, rew_np, done_np, eps_np, **_kw(kind, -3.0))["target"]
    r_fused, _ = R.ratio(y, (ref, bound))
    r_eager, _ = R.ratio(e, (ref, bound))
    r_pair, bad = R.ratio(y, (e.astype(np.float64), 2.0 * bound))
    print(f"\ntd target {kind} B={B}: |fused - fp64| / bound {r_fused:.4f}, |eager - fp64| / bound {r_eager:.4f}, "
          f"|fused - eager| / (2 bound) {r_pair:.4f}")
    assert not bad.any()
    td.close()
