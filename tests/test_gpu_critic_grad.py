"""GPU: the fused critic loss and its gradients (csrc/meshenv_critic_grad.h: k_critic_grad<SAC>, k_critic_grad<TD3>,
k_critic_grad_reduce) against the fp64 restatement of tests/critic_grad_ref.py, every element of every output within its own
bound; the ReLU masks; overwrite semantics, determinism and a side stream; live parameters; eager torch and a stock Adam
step on the gradients the call left; and the whole chain from the rollout to the optimiser step.

Weights: torch's default init, and a stress set (first-layer weights x 6, targets of magnitude 1e3).  Inputs:
policy_ref.input_rows() (repeated beyond its 5028 rows), uniform actions.  Each test prints max |kernel - fp64| / bound."""
import copy

import numpy as np
import pytest

import critic_grad_ref as G
import policy_ref as R

pytestmark = pytest.mark.gpu

BS = (1, 15, 16, 17, 100, 256, 4101, 65536)
STRESS_MAX_B = 4101
KINDS = ("sac", "td3")


@pytest.fixture(scope="module")
def rows():
    return R.input_rows()


def _cuda(m):
    return dict(kind=m["kind"], q1=[copy.deepcopy(l).cuda() for l in m["q1"]], q2=[copy.deepcopy(l).cuda() for l in m["q2"]])


def _fused(mc):
    from reinforcementlearning4meshgeneration_amd.critic_grad import FusedCriticGrad
    return (FusedCriticGrad.sac if mc["kind"] == "sac" else FusedCriticGrad.td3)(mc["q1"], mc["q2"])


def _dev(torch, obs, act, y):
    return torch.from_numpy(obs).cuda(), torch.from_numpy(act).cuda(), torch.from_numpy(y).cuda().reshape(-1, 1)


def _params(mc):
    return [p for c in ("q1", "q2") for l in mc[c] for p in (l.weight, l.bias)]


def _grads(mc):
    """name -> p.grad in critic_grad_ref's naming."""
    return {f"q{c}.{n}{i}": getattr(l, a).grad for c in (1, 2) for i, l in enumerate(mc[f"q{c}"]) for n, a in (("w", "weight"), ("b", "bias"))}


def _got(mc, loss, parts):
    return dict(_grads(mc), loss=loss, q1=parts["q1"], q2=parts["q2"])


def _acts(parts):
    return {1: [a.cpu().numpy() for a in parts["acts1"]], 2: [a.cpu().numpy() for a in parts["acts2"]]}


def _fmt(worst):
    top = sorted(worst.items(), key=lambda kv: -kv[1])
    return f"max {top[0][1]:.4f} ({top[0][0]}) " + " ".join(f"{k}={v:.3f}" for k, v in sorted(worst.items()))


def _eager_loss(torch, mc, obs, act, y):
    x = torch.cat([obs, act], dim=1)
    qs = []
    for c in ("q1", "q2"):
        h = x
        for l in mc[c][:-1]:
            h = torch.relu(l(h))
        qs.append(mc[c][-1](h))
    return 0.5 * sum(torch.nn.functional.mse_loss(q, y) for q in qs)


# ----------------------------------------------------------------------------------------------------------- 1, 2. fp64, masks
@pytest.mark.parametrize("stress", [False, True], ids=["default", "stress"])
@pytest.mark.parametrize("kind", KINDS)
def test_gradients_against_fp64(kind, stress, rows):
    import torch
    m = G.critic_modules(kind, stress=stress)
    mc = _cuda(m)
    cg = _fused(mc)
    worst = {}
    for B in BS:
        if stress and B > STRESS_MAX_B:
            continue
        obs_np, act_np, y_np = G.batch(B, rows, target_scale=1e3 if stress else 1.0)
        obs, act, y = _dev(torch, obs_np, act_np, y_np)
        what = f"{kind} {'stress' if stress else 'default'} B={B}"
        loss, parts = cg.backward(observations=obs, actions=act, target_q_values=y, return_parts=True)
        assert loss.shape == () and loss.dtype == torch.float32 and parts["q1"].shape == (B,)
        acts = _acts(parts)
        ref, info = G.critic_grad(m, obs_np, act_np, y_np, other_acts=acts)
        G.assert_share(info, what)                 # the condition on the case, from the reference alone
        G.assert_masks(info, acts, what)           # 2. masks equal the reference's off the ambiguous pairs
        w = {}
        G.assert_all_within(_got(mc, loss, parts), ref, what, w)
        print(f"\ncritic grad {what}: ambiguous {info['ambiguous_pairs']}; |kernel - fp64| / bound: {_fmt(w)}")
        for k, v in w.items():
            worst[k] = max(worst.get(k, 0.0), v)
        loss2 = cg.backward(observations=obs, actions=act, target_q_values=y.reshape(-1))      # [B] targets, no parts
        assert torch.equal(loss2, loss), what
    print(f"\ncritic grad {kind} {'stress' if stress else 'default'} over all B: {_fmt(worst)}")
    cg.close()


# ----------------------------------------------------------------------------------------------------------- 3. overwrite
@pytest.mark.parametrize("B", [17, 256, 4101])
@pytest.mark.parametrize("kind", KINDS)
def test_overwrite_repeat_and_side_stream(kind, B, rows):
    import torch
    mc = _cuda(G.critic_modules(kind))
    cg = _fused(mc)
    obs, act, y = _dev(torch, *G.batch(B, rows))
    ps = _params(mc)
    assert all(p.grad is None for p in ps)
    loss0 = cg.backward(observations=obs, actions=act, target_q_values=y)
    want = [p.grad.clone() for p in ps]
    assert len(ps) == (16 if kind == "sac" else 12) and all(g.shape == p.shape for g, p in zip(want, ps))
    assert all(float(g.abs().max()) > 0 for g in want)
    # a previous call's result (bit-identical repeat)
    assert torch.equal(cg.backward(observations=obs, actions=act, target_q_values=y), loss0)
    assert all(torch.equal(p.grad, w) for p, w in zip(ps, want))
    # stale garbage, in the views and in tensors of the caller's own
    cg.grad_buffer.fill_(float("nan"))
    assert torch.equal(cg.backward(observations=obs, actions=act, target_q_values=y), loss0)
    assert all(torch.equal(p.grad, w) for p, w in zip(ps, want))
    for p in ps:
        p.grad = torch.full_like(p, float("nan"))
    assert torch.equal(cg.backward(observations=obs, actions=act, target_q_values=y), loss0)
    assert all(torch.equal(p.grad, w) for p, w in zip(ps, want))
    # None after zero_grad(set_to_none=True)
    torch.optim.SGD(ps, lr=0.1).zero_grad(set_to_none=True)
    assert all(p.grad is None for p in ps)
    assert torch.equal(cg.backward(observations=obs, actions=act, target_q_values=y), loss0)
    assert all(torch.equal(p.grad, w) for p, w in zip(ps, want))
    # a side stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        cg.grad_buffer.zero_()
        loss_s = cg.backward(observations=obs, actions=act, target_q_values=y)
    side.synchronize()
    assert torch.equal(loss_s, loss0) and all(torch.equal(p.grad, w) for p, w in zip(ps, want))
    cg.close()


# ----------------------------------------------------------------------------------------------------------- 4. live parameters
@pytest.mark.parametrize("kind", KINDS)
def test_reads_the_live_parameters(kind, rows):
    import torch
    B = 100
    m = G.critic_modules(kind)
    mc = _cuda(m)
    cg = _fused(mc)
    obs_np, act_np, y_np = G.batch(B, rows)
    obs, act, y = _dev(torch, obs_np, act_np, y_np)
    cg.backward(observations=obs, actions=act, target_q_values=y)
    before = [p.grad.clone() for p in _params(mc)]
    with torch.no_grad():                      # in place, as an optimiser writes: no rebind
        for c in ("q1", "q2"):
            mc[c][1].weight.mul_(1.5)
            mc[c][-1].bias.add_(0.25)
            m[c][1].weight.mul_(1.5)
            m[c][-1].bias.add_(0.25)
    loss, parts = cg.backward(observations=obs, actions=act, target_q_values=y, return_parts=True)
    acts = _acts(parts)
    ref, info = G.critic_grad(m, obs_np, act_np, y_np, other_acts=acts)
    G.assert_share(info, kind)
    G.assert_masks(info, acts, kind)
    G.assert_all_within(_got(mc, loss, parts), ref, f"{kind} after an in-place change")
    assert not any(torch.equal(p.grad, b) for p, b in zip(_params(mc), before))
    cg.close()


# ----------------------------------------------------------------------------------------------------------- 5. eager torch, Adam
@pytest.mark.parametrize("B", [100, 256, 4101])
@pytest.mark.parametrize("kind", KINDS)
def test_against_eager_torch_and_a_stock_adam_step(kind, B, rows):
    import torch
    m = G.critic_modules(kind)
    mc, me = _cuda(m), _cuda(m)
    cg = _fused(mc)
    obs_np, act_np, y_np = G.batch(B, rows)
    obs, act, y = _dev(torch, obs_np, act_np, y_np)
    loss, parts = cg.backward(observations=obs, actions=act, target_q_values=y, return_parts=True)
    ref, info = G.critic_grad(m, obs_np, act_np, y_np, other_acts=_acts(parts))
    G.assert_share(info, kind)
    opt_e = torch.optim.Adam(_params(me), lr=3e-4)
    opt_e.zero_grad()
    loss_e = _eager_loss(torch, me, obs, act, y)
    loss_e.backward()
    fused, eager = _got(mc, loss, parts), dict(_grads(me), loss=loss_e)
    worst = 0.0
    for k, (r, bound) in ref.items():
        if k in ("q1", "q2"):
            continue
        d = np.abs(fused[k].detach().cpu().numpy().astype(np.float64).reshape(r.shape) - eager[k].detach().cpu().numpy().astype(np.float64).reshape(r.shape))
        assert (d <= 2.0 * bound).all(), (kind, B, k, float((d / np.maximum(bound, 1e-300)).max()))
        worst = max(worst, float((d / np.maximum(bound, 1e-300)).max()))
    print(f"\ncritic grad {kind} B={B}: max |fused - eager| / bound = {worst:.4f} (allowed 2)")
    # the stock optimiser consumes what the call left: same step as a cloned model whose p.grad were filled by copy_
    mk = _cuda(m)
    opt_f, opt_k = torch.optim.Adam(_params(mc), lr=3e-4), torch.optim.Adam(_params(mk), lr=3e-4)
    for pk, pf in zip(_params(mk), _params(mc)):
        pk.grad = torch.empty_like(pk)
        pk.grad.copy_(pf.grad)
    opt_f.step()
    opt_k.step()
    assert all(torch.equal(pf, pk) for pf, pk in zip(_params(mc), _params(mk)))
    assert not any(torch.equal(pf, pe) for pf, pe in zip(_params(mc), _params(_cuda(m))))       # and it moved them
    cg.close()


# ----------------------------------------------------------------------------------------------------------- 6. the chain
def test_rollout_replay_target_critic_update_chain():
    """add_rollout -> sample -> FusedTDTarget.target -> FusedCriticGrad.backward -> optimizer.step -> polyak (eager) ->
    td.refresh, a few iterations: every loss is finite and the parameters moved (no assertion on learning)."""
    import torch
    from reinforcementlearning4meshgeneration_amd import (DeviceReplayBuffer, FusedActor, FusedCriticGrad, FusedTDTarget, MeshVecEnv,
                                                          boundary)
    torch.manual_seed(999)
    latent_pi = torch.nn.Sequential(*[m for i in range(3) for m in (torch.nn.Linear(18 if i == 0 else 128, 128), torch.nn.ReLU())])
    mu, log_std = torch.nn.Linear(128, 3), torch.nn.Linear(128, 3)

    def q():
        return torch.nn.Sequential(torch.nn.Linear(21, 128), torch.nn.ReLU(), torch.nn.Linear(128, 128), torch.nn.ReLU(),
                                   torch.nn.Linear(128, 128), torch.nn.ReLU(), torch.nn.Linear(128, 1))
    critic = [q(), q()]
    lin = [m for m in latent_pi if isinstance(m, torch.nn.Linear)]
    actor = FusedActor.from_torch(lin, mu, log_std)
    for m in (latent_pi, mu, log_std, *critic):
        m.cuda()
    critic_target = copy.deepcopy(critic)
    log_ent_coef = torch.zeros(1, device="cuda")
    params = [p for c in critic for p in c.parameters()]
    target_params = [p for c in critic_target for p in c.parameters()]
    start = [p.detach().clone() for p in params]
    opt = torch.optim.Adam(params, lr=3e-4)
    td = FusedTDTarget.sac(lin, mu, log_std, critic_target[0], critic_target[1], 0.99, log_ent_coef=log_ent_coef)
    cg = FusedCriticGrad.sac(critic[0], critic[1])
    env = MeshVecEnv([boundary(0)], n_envs=256)
    buf = DeviceReplayBuffer(env, buffer_size=100_000)
    T = 8
    obs0 = env.reset().clone()
    actions = actor.sample(obs0, 999, 0)
    draw, batch_no, losses = 1, 0, []
    for _ in range(3):
        out = env.step_actor_T(actor, actions, T, seed=999, counter=draw, want_terminal_obs=True)
        buf.add_rollout(out, obs0=obs0)
        obs0, actions, draw = out["obs"][T - 1].clone(), out["actions"][T], draw + T
        for _ in range(4):
            batch_no += 1
            s = buf.sample(100, seed=1, counter=batch_no)
            y = td.target(s, seed=2, counter=batch_no)
            losses.append(cg.backward(s, y))
            opt.step()
            with torch.no_grad():
                for p, pt in zip(params, target_params):
                    pt.data.mul_(1 - 0.005).add_(p.data, alpha=0.005)
            td.refresh()
    losses = torch.stack(losses).cpu().numpy()
    print(f"\ncritic losses over the chain: {losses[0]:.5f} .. {losses[-1]:.5f}")
    assert losses.shape == (12,) and np.isfinite(losses).all() and (losses >= 0).all()
    assert all(not torch.equal(p, p0) for p, p0 in zip(params, start))
    assert all(bool(torch.isfinite(p).all()) for p in params)
    cg.close(); td.close(); actor.close(); env.close()
