"""GPU: FusedPolicy.bind_live + refresh() (meshenv_policy_bind / _refresh: one k_target_pack launch) carries the live parameters
into the packed weights exactly as a new FusedPolicy.from_sb3 would build them on the host; and the chain rollout ->
FusedPPOGrad.backward -> stock Adam -> refresh -> rollout stays on the device."""
import types

import numpy as np
import pytest

import policy_ref as R
import ppo_grad_ref as P

pytestmark = pytest.mark.gpu


def _sb3_policy(case, seed=11):
    """An SB3-2.x-shaped ActorCriticPolicy on the GPU from ppo_grad_ref.modules(case)."""
    import torch
    m = P.modules(case, seed=seed)
    act = torch.nn.Tanh if m["act"] == "tanh" else torch.nn.ReLU
    seq = lambda ls: torch.nn.Sequential(ls[0], act(), ls[1], act()).cuda()   # noqa: E731
    fe = type("FlattenExtractor", (torch.nn.Module,), {})()
    pol = types.SimpleNamespace(mlp_extractor=types.SimpleNamespace(policy_net=seq(m["pi"]), value_net=seq(m["vf"])),
                                action_net=m["action_net"].cuda(), value_net=m["value_net"].cuda(),
                                log_std=torch.nn.Parameter(m["log_std"].detach().clone().cuda()), use_sde=False, squash_output=False,
                                features_extractor=fe, pi_features_extractor=fe, vf_features_extractor=fe, share_features_extractor=True)
    params = [p for mod in (pol.mlp_extractor.policy_net, pol.action_net, pol.mlp_extractor.value_net, pol.value_net)
              for p in mod.parameters()] + [pol.log_std]
    return pol, params


def _same(a, b):
    import torch
    return all(torch.equal(a[k], b[k]) for k in ("actions", "buffer_actions", "log_prob", "value"))


@pytest.mark.parametrize("case", list(P.CASES))
def test_refresh_equals_a_policy_rebuilt_from_the_updated_parameters(case):
    import torch
    from reinforcementlearning4meshgeneration_amd import FusedPolicy
    n = 33
    pol, params = _sb3_policy(case)
    obs = torch.from_numpy(R.input_rows()[:n].copy()).cuda()
    noise = torch.from_numpy(R.noise_rows(n)).cuda()
    fp = FusedPolicy.from_sb3(pol)
    before = fp.forward(obs, noise)
    with pytest.raises(ValueError, match="bind_live"):
        fp.refresh()
    fp.bind_live(pol)
    fp.refresh()
    assert _same(fp.forward(obs, noise), before)                    # unchanged parameters: the packed buffer is rewritten as it was
    g = torch.Generator(device="cuda").manual_seed(5)
    with torch.no_grad():                                           # in place, as an optimiser writes
        for p in params:
            p.add_(0.05 * torch.randn(p.shape, device="cuda", generator=g))
    stale = fp.forward(obs, noise)
    assert _same(stale, before)                                     # nothing moves before the refresh
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                   # the refresh is ordered with the forward behind it
        fp.refresh()
        got = fp.forward(obs, noise)
    side.synchronize()
    want = FusedPolicy.from_sb3(pol).forward(obs, noise)
    assert _same(got, want) and not torch.equal(got["log_prob"], before["log_prob"])
    fp.close()


def test_chain_rollout_backward_adam_refresh_rollout():
    import torch
    from reinforcementlearning4meshgeneration_amd import FusedPolicy, FusedPPOGrad, MeshVecEnv, boundary
    n_envs, T = 64, 8
    pol, params = _sb3_policy("ppo-relu128")
    model = types.SimpleNamespace(policy=pol, clip_range_vf=None)
    fp = FusedPolicy.from_sb3(model)
    fp.bind_live(model)
    pg = FusedPPOGrad.from_sb3(model)
    opt = torch.optim.Adam(params, lr=3e-4, eps=1e-5)
    start = [p.detach().clone() for p in params]
    env = MeshVecEnv([boundary(0)], n_envs=n_envs)
    env.reset()
    out = env.collect_rollout(fp, T, seed=3, counter=0, gamma=0.99)
    flat = {k: out[k].reshape(T * n_envs, *out[k].shape[2:]) for k in ("obs", "buffer_actions", "log_prob", "advantages", "returns")}
    perm = torch.randperm(T * n_envs, device="cuda")
    losses = []
    for idx in perm.chunk(2):
        res = pg.backward(observations=flat["obs"][idx], actions=flat["buffer_actions"][idx], old_log_prob=flat["log_prob"][idx],
                          advantages=flat["advantages"][idx], returns=flat["returns"][idx], clip_range=0.2, ent_coef=0.01,
                          vf_coef=0.5, max_grad_norm=0.5)
        opt.step()
        losses.append(torch.stack([res[k] for k in ("loss", "policy_loss", "value_loss", "approx_kl", "clip_fraction", "grad_norm")]))
    fp.refresh()
    out2 = env.collect_rollout(fp, T, seed=3, counter=T, gamma=0.99)
    ls = torch.stack(losses).cpu().numpy()
    print(f"\nppo chain: loss policy value kl clip_fraction grad_norm per minibatch\n{ls}")
    assert np.isfinite(ls).all() and all(not torch.equal(p, s) for p, s in zip(params, start))
    assert all(bool(torch.isfinite(out2[k]).all()) for k in ("log_prob", "value", "advantages", "returns"))
    fresh = FusedPolicy.from_sb3(model).forward(out2["obs"].reshape(-1, 18), out2["eps"].reshape(-1, 3))
    assert torch.equal(out2["log_prob"].reshape(-1), fresh["log_prob"]) and torch.equal(out2["value"].reshape(-1), fresh["value"])
    pg.close(); fp.close(); env.close()
