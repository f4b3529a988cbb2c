"""GPU: the fused TD3 / DDPG actor-loss statement (csrc/meshenv_td3_actor_grad.h: k_td3_actor_grad, k_td3_actor_grad_reduce)
against the fp64 restatement of tests/td3_actor_grad_ref.py, every element of every output and of every return_parts entry
within its own bound; the ReLU masks; overwrite semantics, determinism, a side stream and untouched critic gradients; live
parameters; eager torch and a stock Adam step on the gradients the call left; and the TD3 recipe end to end.

Weights: torch's default init (td_target_ref.td3_modules()) on the tight rows of policy_ref.input_rows(), and the stress set
(td3_actor_grad_ref.modules(stress=True): components 0 and 2 of tanh saturated).  Each test prints max |kernel - fp64| / bound.
The batch sizes: a lone row, a partial tile, exactly one tile, one row into a second, the recipe's 100 and 256, and 4101 (257
tiles: more than 64 x 4, with a ragged tail)."""
import copy

import numpy as np
import pytest

import policy_ref as R
import td3_actor_grad_ref as A

pytestmark = pytest.mark.gpu

BS = (1, 15, 16, 17, 100, 256, 4101)
STRESS_MAX_B = 256


@pytest.fixture(scope="module")
def rows():
    return R.input_rows()


def _cuda(m):
    return dict(kind="td3", lin=[copy.deepcopy(l).cuda() for l in m["lin"]], mu=copy.deepcopy(m["mu"]).cuda(),
                q1=[copy.deepcopy(l).cuda() for l in m["q1"]], q2=[copy.deepcopy(l).cuda() for l in m["q2"]])


def _fused(mc):
    from reinforcementlearning4meshgeneration_amd.td3_actor_grad import FusedTD3ActorGrad
    return FusedTD3ActorGrad.td3(mc["lin"], mc["mu"], mc["q1"])


def _actor_params(mc):
    return [p for l in (*mc["lin"], mc["mu"]) for p in (l.weight, l.bias)]


def _critic_params(mc):
    return [p for c in ("q1", "q2") for l in mc[c] for p in (l.weight, l.bias)]


def _grads(mc):
    """name -> p.grad in td3_actor_grad_ref's naming."""
    g = {f"a.{n}{i}": getattr(l, a).grad for i, l in enumerate(mc["lin"]) for n, a in (("w", "weight"), ("b", "bias"))}
    g.update({"mu.w": mc["mu"].weight.grad, "mu.b": mc["mu"].bias.grad})
    return g


def _got(mc, loss, parts):
    return dict(_grads(mc), actor_loss=loss, **{k: parts[k] for k in A.PARTS})


def _host_parts(parts):
    out = {k: parts[k].cpu().numpy() for k in A.PARTS}
    out.update({k: [a.cpu().numpy() for a in parts[k]] for k in ("acts", "acts1")})
    return out


def _fmt(worst):
    top = sorted(worst.items(), key=lambda kv: -kv[1])
    return f"max {top[0][1]:.4f} ({top[0][0]}) " + " ".join(f"{k}={v:.3f}" for k, v in sorted(worst.items()))


# ----------------------------------------------------------------------------------------------------------- 1. fp64, masks
@pytest.mark.parametrize("stress", [False, True], ids=["default", "stress"])
def test_gradients_and_parts_against_fp64(stress, rows):
    import torch
    m = A.modules(stress)
    mc = _cuda(m)
    ag = _fused(mc)
    worst = {}
    for B in BS:
        if stress and B > STRESS_MAX_B:
            continue
        obs_np, _ = A.batch(B, rows)
        obs = torch.from_numpy(obs_np).cuda()
        what = f"{'stress' if stress else 'default'} B={B}"
        loss, parts = ag.backward(observations=obs, return_parts=True)
        assert loss.shape == () and loss.dtype == torch.float32 and loss.is_cuda
        assert parts["actions_pi"].shape == (B, 3) and parts["q1_pi"].shape == (B,) and parts["dq_da"].shape == (B, 3)
        assert parts["d_pre"].shape == (B, 3) and [tuple(a.shape) for k in ("acts", "acts1") for a in parts[k]] == [(B, 256)] * 4
        hp = _host_parts(parts)
        ref, info = A.td3_actor_grad(m, obs_np, other=hp)
        A.assert_conditions(info, what, stress=stress)                             # from the reference alone
        A.assert_choices(info, hp, what)                                          # the masks off the ambiguous pairs
        w = {}
        A.assert_all_within(_got(mc, loss, parts), ref, what, w)
        assert set(w) == set(ref)
        print(f"\ntd3 actor grad {what}: {A.describe(info)}; |kernel - fp64| / bound: {_fmt(w)}")
        for k, v in w.items():
            worst[k] = max(worst.get(k, 0.0), v)
        if stress:                                                                # components 0 and 2 saturated, 1 not
            assert (np.abs(hp["actions_pi"][:, [0, 2]]) > 0.9999).all() and (hp["d_pre"][:, 1] != 0).any()
        want = [p.grad.clone() for p in _actor_params(mc)]
        loss2 = ag.backward(observations=obs)                                      # no parts: the same bits
        assert torch.equal(loss2, loss) and all(torch.equal(p.grad, g) for p, g in zip(_actor_params(mc), want)), what
    print(f"\ntd3 actor grad {'stress' if stress else 'default'} over all B: {_fmt(worst)}")
    ag.close()


# ----------------------------------------------------------------------------------------------------------- 2. overwrite
@pytest.mark.parametrize("B", [17, 256, 4101])
def test_overwrite_repeat_side_stream_and_critic_grads(B, rows):
    import torch
    mc = _cuda(A.modules())
    ag = _fused(mc)
    obs = torch.from_numpy(A.batch(B, rows)[0]).cuda()
    ps, qs = _actor_params(mc), _critic_params(mc)
    for i, p in enumerate(qs):                       # the critics' gradients are the caller's: left exactly as they are
        p.grad = None if i % 3 == 0 else torch.full_like(p, float(i))
    kept = [None if p.grad is None else (p.grad, p.grad.clone()) for p in qs]
    assert all(p.grad is None for p in ps)
    l0 = ag.backward(observations=obs)
    want = [p.grad.clone() for p in ps]
    assert len(ps) == 6 and all(g.shape == p.shape for g, p in zip(want, ps)) and all(float(g.abs().max()) > 0 for g in want)
    assert all(p.grad.data_ptr() == ag.grad_buffer.data_ptr() + 4 * at for p, at in ag.spec.offsets())   # views of one buffer

    def same(l):
        return torch.equal(l, l0) and all(torch.equal(p.grad, w) for p, w in zip(ps, want))
    assert same(ag.backward(observations=obs))                                     # a bit-identical repeat
    ag.grad_buffer.fill_(float("nan"))                                            # stale garbage in the buffer
    assert same(ag.backward(observations=obs))
    for p in ps:                                                                  # and in tensors of the caller's own
        p.grad = torch.full_like(p, float("nan"))
    assert same(ag.backward(observations=obs))
    torch.optim.SGD(ps, lr=0.1).zero_grad(set_to_none=True)
    assert all(p.grad is None for p in ps)
    assert same(ag.backward(observations=obs))                                     # re-attached
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ag.grad_buffer.zero_()
        ls = ag.backward(observations=obs)
    side.synchronize()
    assert same(ls)
    for p, k in zip(qs, kept):
        assert (p.grad is None) if k is None else (p.grad is k[0] and torch.equal(p.grad, k[1]))
    ag.close()


# ----------------------------------------------------------------------------------------------------------- 3. live parameters
def test_reads_the_live_parameters(rows):
    import torch
    B = 100
    m = A.modules()
    mc = _cuda(m)
    ag = _fused(mc)
    obs_np, _ = A.batch(B, rows)
    obs = torch.from_numpy(obs_np).cuda()
    l0 = ag.backward(observations=obs)
    before = [p.grad.clone() for p in _actor_params(mc)]
    with torch.no_grad():                      # in place, as an optimiser writes: no rebind
        for mm in (m, mc):
            mm["lin"][1].weight.mul_(1.25)
            mm["q1"][1].weight.mul_(1.5)
            mm["q1"][0].bias.add_(0.125)
    loss, parts = ag.backward(observations=obs, return_parts=True)
    hp = _host_parts(parts)
    ref, info = A.td3_actor_grad(m, obs_np, other=hp)
    A.assert_choices(info, hp, "after an in-place change")
    A.assert_all_within(_got(mc, loss, parts), ref, "after an in-place change")
    assert not any(torch.equal(p.grad, b) for p, b in zip(_actor_params(mc), before)) and not torch.equal(loss, l0)
    ag.close()


# ----------------------------------------------------------------------------------------------------------- 4. eager torch, Adam
def _eager(torch, me, obs):
    """SB3's statement on the CUDA modules: -critic.q1_forward(obs, actor(obs)).mean()."""
    h = obs
    for l in me["lin"]:
        h = torch.relu(l(h))
    hc = torch.cat([obs, torch.tanh(me["mu"](h))], dim=1)
    for l in me["q1"][:-1]:
        hc = torch.relu(l(hc))
    return -me["q1"][-1](hc).mean()


@pytest.mark.parametrize("B", [100, 256, 4101])
def test_against_eager_torch_and_a_stock_adam_step(B, rows):
    import torch
    m = A.modules()
    mc, me = _cuda(m), _cuda(m)
    ag = _fused(mc)
    obs_np, _ = A.batch(B, rows)
    obs = torch.from_numpy(obs_np).cuda()
    loss, parts = ag.backward(observations=obs, return_parts=True)
    ref, info = A.td3_actor_grad(m, obs_np, other=_host_parts(parts))
    A.assert_conditions(info, f"B={B}")
    loss_e = _eager(torch, me, obs)
    loss_e.backward()
    fused, eager = dict(_grads(mc), actor_loss=loss), dict(_grads(me), actor_loss=loss_e)
    worst = 0.0
    for k in (*A.GRADS, "actor_loss"):
        r, bound = ref[k]
        f64 = lambda v: v.detach().cpu().numpy().astype(np.float64).reshape(r.shape)   # noqa: E731
        d = np.abs(f64(fused[k]) - f64(eager[k]))
        assert (d <= 2.0 * bound).all(), (B, k, float((d / np.maximum(2.0 * bound, 1e-300)).max()))
        worst = max(worst, float((d / np.maximum(2.0 * bound, 1e-300)).max()))
    print(f"\ntd3 actor grad B={B}: max |fused - eager| / (2 bound) = {worst:.4f}")
    # the stock optimiser consumes what the call left: same step as a cloned model whose p.grad were filled by copy_
    mk = _cuda(m)
    pf, pk = _actor_params(mc), _actor_params(mk)
    opt_f, opt_k = torch.optim.Adam(pf, lr=3e-4), torch.optim.Adam(pk, lr=3e-4)
    for k_, f_ in zip(pk, pf):
        k_.grad = torch.empty_like(k_)
        k_.grad.copy_(f_.grad)
    opt_f.step()
    opt_k.step()
    assert all(torch.equal(f_, k_) for f_, k_ in zip(pf, pk))
    assert not any(torch.equal(f_, e_) for f_, e_ in zip(pf, _actor_params(_cuda(m))))       # and it moved them
    ag.close()


# ----------------------------------------------------------------------------------------------------------- 5. the chain
def _seq(lins, tail=None):
    import torch
    mods = [x for l in lins[:-1] for x in (l, torch.nn.ReLU())] + [lins[-1]] + ([tail] if tail else [])
    return torch.nn.Sequential(*mods)


def _lins(seq):
    return [l for l in seq if type(l).__name__ == "Linear"]


def test_td3_recipe_chain():
    """rollout -> add_rollout -> sample -> FusedTDTarget.td3 target -> FusedCriticGrad.td3 backward -> critic_step -> every
    second step FusedTD3ActorGrad.backward and actor_step(polyak=True) -> td.refresh: every loss finite, both parameter groups
    and both target groups moved (no assertion on learning)."""
    import torch
    from reinforcementlearning4meshgeneration_amd import (DeviceReplayBuffer, FusedActor, FusedCriticGrad, FusedOptimStep, FusedTD3ActorGrad,
                                                          FusedTDTarget, MeshVecEnv, boundary)
    import td_target_ref as T
    m = T.td3_modules()
    c = lambda l: copy.deepcopy(l).cuda()   # noqa: E731
    critic = torch.nn.ModuleList([_seq([c(l) for l in m["q1"]]), _seq([c(l) for l in m["q2"]])])
    actor = _seq([c(l) for l in m["lin"]] + [c(m["mu"])], torch.nn.Tanh())
    critic_target, actor_target = copy.deepcopy(critic), copy.deepcopy(actor)
    cp, ctp = list(critic.parameters()), list(critic_target.parameters())
    ap, atp = list(actor.parameters()), list(actor_target.parameters())
    start = [[p.detach().clone() for p in g] for g in (cp, ap, ctp, atp)]
    opt_c, opt_a = torch.optim.Adam(cp, lr=3e-4), torch.optim.Adam(ap, lr=3e-4)
    al, atl = _lins(actor), _lins(actor_target)
    td = FusedTDTarget.td3(atl[:2], atl[2], critic_target[0], critic_target[1], 0.99)
    cg = FusedCriticGrad.td3(_lins(critic[0]), _lins(critic[1]))
    ag = FusedTD3ActorGrad.td3(al[:2], al[2], critic[0])
    fo = FusedOptimStep.td3(opt_c, opt_a, cp, ctp, ap, atp, tau=0.005)
    # the rollout's behaviour policy is beside the point here: a SAC-shaped FusedActor fills the buffer
    torch.manual_seed(999)
    lin = [torch.nn.Linear(18, 128), torch.nn.Linear(128, 128), torch.nn.Linear(128, 128)]
    roll = FusedActor.from_torch(lin, torch.nn.Linear(128, 3), torch.nn.Linear(128, 3))
    env = MeshVecEnv([boundary(0)], n_envs=256)
    buf = DeviceReplayBuffer(env, buffer_size=100_000)
    Tn, policy_delay = 8, 2
    obs0 = env.reset().clone()
    actions = roll.sample(obs0, 999, 0)
    out = env.step_actor_T(roll, actions, Tn, seed=999, counter=1, want_terminal_obs=True)
    buf.add_rollout(out, obs0=obs0)
    losses_c, losses_a = [], []
    for step in range(1, 5):
        s = buf.sample(100, seed=1, counter=step)
        y = td.target(s, seed=2, counter=step)
        losses_c.append(cg.backward(s, y))
        fo.critic_step()
        if step % policy_delay == 0:
            losses_a.append(ag.backward(s))
            fo.actor_step(polyak=True)
        td.refresh()
    lc, la = torch.stack(losses_c).cpu().numpy(), torch.stack(losses_a).cpu().numpy()
    print(f"\ntd3 chain: critic losses {lc}, actor losses {la}; uploads {fo.binds}")
    assert lc.shape == (4,) and la.shape == (2,) and np.isfinite(lc).all() and np.isfinite(la).all() and (lc >= 0).all()
    for group, first in zip((cp, ap, ctp, atp), start):
        assert all(not torch.equal(p, p0) for p, p0 in zip(group, first))
        assert all(bool(torch.isfinite(p).all()) for p in group)
    assert all(float(opt_c.state[p]["step"]) == 4.0 for p in cp) and all(float(opt_a.state[p]["step"]) == 2.0 for p in ap)
    fo.close(); ag.close(); cg.close(); td.close(); roll.close(); env.close()
