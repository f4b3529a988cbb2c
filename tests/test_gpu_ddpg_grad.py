"""GPU: DDPG's two fused gradient statements at [400, 300] (csrc/meshenv_wide_grad.h: k_wgrad_critic_rows,
k_wgrad_actor_rows, k_wgrad_weights, k_wgrad_reduce) against the fp64 restatements of tests/ddpg_grad_ref.py, every element
of every output and of every return_parts entry within its own bound; the ReLU masks; NaN rows past the batch and a shrinking
workspace; determinism, a side stream, row independence and the two gradient sets' isolation; loss_scale; live parameters;
one optimiser step on the gradients the calls left; and examples/ddpg_train_step.py --check.

Weights: torch's default init (ddpg_ref.ddpg_model()) on the tight rows of policy_ref.input_rows(), the first layer x 6 and
the saturated head.  Each accuracy test prints max |kernel - fp64| / bound.  The batch sizes: a lone row, a partial tile,
exactly one tile, one row into a second, three tiles with a ragged tail, the recipes' 100 and 256, and 4101 (257 tiles: the
first size with more than four tiles to a chunk, 52 chunks, a ragged tail)."""
import copy
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import ddpg_grad_ref as G
import ddpg_ref as D
import optim_step_ref as O
import policy_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rows():
    return R.input_rows()


def _cuda(m):
    return G.attach_optimizers(D.to_cuda(copy.deepcopy(m)), lr=1e-3)


def _fused(mc, loss_scale=1.0):
    from reinforcementlearning4meshgeneration_amd import FusedDDPGGrad
    return FusedDDPGGrad.from_sb3(mc, loss_scale=loss_scale)


def _lin(seq):
    return [l for l in seq if type(l).__name__ == "Linear"]


def _actor_params(mc):
    return [p for l in _lin(mc.actor.mu) for p in (l.weight, l.bias)]


def _critic_params(mc):
    return [p for l in _lin(mc.critic.q_networks[0]) for p in (l.weight, l.bias)]


def _critic_grads(mc):
    return {f"c.{n}{i}": getattr(l, a).grad for i, l in enumerate(_lin(mc.critic.q_networks[0])) for n, a in (("w", "weight"), ("b", "bias"))}


def _actor_grads(mc):
    lin = _lin(mc.actor.mu)
    g = {f"a.{n}{i}": getattr(l, a).grad for i, l in enumerate(lin[:2]) for n, a in (("w", "weight"), ("b", "bias"))}
    g.update({"mu.w": lin[2].weight.grad, "mu.b": lin[2].bias.grad})
    return g


def _t(torch, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _host_parts(parts):
    out = {k: parts[k].cpu().numpy() for k in G.PARTS}
    out.update({k: [a.cpu().numpy() for a in parts[k]] for k in ("acts", "acts1")})
    return out


def _fmt(worst):
    top = sorted(worst.items(), key=lambda kv: -kv[1])
    return f"max {top[0][1]:.4f} ({top[0][0]}) " + " ".join(f"{k}={v:.3f}" for k, v in sorted(worst.items()))


# ----------------------------------------------------------------------------------------------------------- 1. fp64, masks
@pytest.mark.parametrize("stress", [None, "critic_w6"], ids=str)
def test_critic_gradients_against_fp64(stress, rows):
    import torch
    m = G.model(stress)
    mc = _cuda(m)
    worst = {}
    for loss_scale in G.LOSS_SCALES:
        dg = _fused(mc, loss_scale)
        for B in G.GPU_BS:
            obs_np, act_np, y_np = G.batch(B, rows)
            obs, act, y = _t(torch, obs_np, act_np, y_np)
            what = f"critic {stress} scale {loss_scale} B={B}"
            loss, parts = dg.critic_backward(observations=obs, actions=act, target_q_values=y, return_parts=True)
            assert loss.shape == () and loss.dtype == torch.float32 and loss.is_cuda and parts["q1"].shape == (B,)
            assert [tuple(a.shape) for a in parts["acts1"]] == [(B, 400), (B, 300)]
            acts = [a.cpu().numpy() for a in parts["acts1"]]
            ref, info = G.critic_grad(m, obs_np, act_np, y_np, loss_scale, other_acts=acts)
            G.assert_critic_conditions(info, what)                                  # from the reference alone
            G.assert_masks(info["ambiguous"], info["mask"], acts, what)            # the masks off the ambiguous pairs
            w = {}
            G.assert_all_within(dict(_critic_grads(mc), critic_loss=loss, q1=parts["q1"]), ref, what, w)
            assert set(w) == set(ref)
            print(f"\n{what}: ambiguous {info['share']:.1e}; |kernel - fp64| / bound: {_fmt(w)}")
            for k, v in w.items():
                worst[k] = max(worst.get(k, 0.0), v)
            want = [p.grad.clone() for p in _critic_params(mc)]
            loss2 = dg.critic_backward(observations=obs, actions=act, target_q_values=y.reshape(B, 1))   # no parts: the same bits
            assert torch.equal(loss2, loss) and all(torch.equal(p.grad, g) for p, g in zip(_critic_params(mc), want)), what
        dg.close()
    print(f"\nddpg critic grad {stress} over all B and both scales: {_fmt(worst)}")


@pytest.mark.parametrize("stress", [None, "actor_w6", "head"], ids=str)
def test_actor_gradients_and_parts_against_fp64(stress, rows):
    import torch
    m = G.model(stress)
    mc = _cuda(m)
    dg = _fused(mc)
    worst = {}
    for B in G.GPU_BS:
        obs_np, _, _ = G.batch(B, rows)
        obs, = _t(torch, obs_np)
        what = f"actor {stress} B={B}"
        before = [p.grad for p in _critic_params(mc)]
        loss, parts = dg.actor_backward(observations=obs, return_parts=True)
        assert loss.shape == () and loss.dtype == torch.float32 and loss.is_cuda
        assert parts["actions_pi"].shape == (B, 3) and parts["q1_pi"].shape == (B,) and parts["dq_da"].shape == (B, 3)
        assert parts["d_pre"].shape == (B, 3) and [tuple(a.shape) for k in ("acts", "acts1") for a in parts[k]] == [(B, 400), (B, 300)] * 2
        hp = _host_parts(parts)
        ref, info = G.actor_grad(m, obs_np, other=hp)
        G.assert_actor_conditions(info, what, head_stress=stress == "head")       # from the reference alone
        G.assert_actor_choices(info, hp, what)
        assert all(a is b for a, b in zip(before, (p.grad for p in _critic_params(mc))))
        got = dict(_actor_grads(mc), actor_loss=loss, **{k: parts[k] for k in G.PARTS})
        got.update({"c.w2": np.zeros((1, 300)), "c.b2": np.zeros(1)})              # (the critic's set: test 3 compares its bits)
        w = {}
        G.assert_all_within(got, ref, what, w)
        assert set(w) == set(ref)
        print(f"\n{what}: ambiguous actor {info['actor_share']:.1e} critic {info['critic_share']:.1e}; |kernel - fp64| / bound: {_fmt(w)}")
        for k, v in w.items():
            worst[k] = max(worst.get(k, 0.0), v)
        if stress == "head":                                                       # components 0 and 2 saturated, 1 not
            assert (np.abs(hp["actions_pi"][:, [0, 2]]) > 0.9999).all() and (hp["d_pre"][:, 1] != 0).any()
        want = [p.grad.clone() for p in _actor_params(mc)]
        loss2 = dg.actor_backward(observations=obs)
        assert torch.equal(loss2, loss) and all(torch.equal(p.grad, g) for p, g in zip(_actor_params(mc), want)), what
    print(f"\nddpg actor grad {stress} over all B: {_fmt(worst)}")
    dg.close()


# ----------------------------------------------------------------------------------------------------------- 2. tails, workspace
def _both(dg, mc, obs, act, y):
    """Both statements with every part; everything the calls wrote, cloned."""
    lc, pc = dg.critic_backward(observations=obs, actions=act, target_q_values=y, return_parts=True)
    out = [lc.clone(), pc["q1"], *pc["acts1"]] + [p.grad.clone() for p in _critic_params(mc)]
    la, pa = dg.actor_backward(observations=obs, return_parts=True)
    out += [la.clone()] + [pa[k] for k in G.PARTS] + pa["acts"] + pa["acts1"] + [p.grad.clone() for p in _actor_params(mc)]
    return out


@pytest.mark.parametrize("B", [17, 33])
def test_nan_rows_past_the_batch_are_never_read(B, rows):
    import torch
    mc = _cuda(G.model())
    dg = _fused(mc)
    obs, act, y = _t(torch, *G.batch(B, rows))
    want = _both(dg, mc, obs, act, y)
    big = [torch.full((B + 16, *x.shape[1:]), float("nan"), device="cuda") for x in (obs, act, y)]
    for b, x in zip(big, (obs, act, y)):
        b[:B] = x
    got = _both(dg, mc, *(b[:B] for b in big))
    assert all(bool(torch.isfinite(g).all()) for g in got)
    assert all(torch.equal(g, w) for g, w in zip(got, want))
    dg.close()


def test_a_smaller_batch_after_a_larger_one_reads_no_stale_rows(rows):
    import torch
    mc = _cuda(G.model())
    dg, fresh = _fused(mc), _fused(mc)
    big = _t(torch, *G.batch(4101, rows))
    small = _t(torch, *G.batch(17, rows))
    _both(dg, mc, *big)
    got = _both(dg, mc, *small)
    want = _both(fresh, mc, *small)
    assert all(torch.equal(g, w) for g, w in zip(got, want))
    dg.close(); fresh.close()


# ----------------------------------------------------------------------------------------------------------- 3. determinism, isolation
def test_repeat_side_stream_row_independence_and_isolation(rows):
    import torch
    mc = _cuda(G.model())
    dg = _fused(mc)
    obs, act, y = _t(torch, *G.batch(4101, rows))
    cp, ap = _critic_params(mc), _actor_params(mc)
    assert all(p.grad is None for p in cp + ap)
    want = _both(dg, mc, obs, act, y)
    assert all(p.grad.data_ptr() == dg.grad_buffer.data_ptr() + 4 * at for p, at in dg.spec.offsets())   # views of one buffer
    assert all(float(p.grad.abs().max()) > 0 for p in cp + ap)
    assert all(torch.equal(g, w) for g, w in zip(_both(dg, mc, obs, act, y), want))        # a bit-identical repeat
    dg.grad_buffer.fill_(float("nan"))                                                     # overwritten, not accumulated
    assert all(torch.equal(g, w) for g, w in zip(_both(dg, mc, obs, act, y), want))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        dg.grad_buffer.zero_()
        got = _both(dg, mc, obs, act, y)
    side.synchronize()
    assert all(torch.equal(g, w) for g, w in zip(got, want))
    # ---- the first 17 rows of the per-row outputs do not depend on the batch
    n = 17
    lc, pc = dg.critic_backward(observations=obs[:n], actions=act[:n], target_q_values=y[:n], return_parts=True)
    la, pa = dg.actor_backward(observations=obs[:n], return_parts=True)
    lc_big, pc_big = dg.critic_backward(observations=obs, actions=act, target_q_values=y, return_parts=True)
    la_big, pa_big = dg.actor_backward(observations=obs, return_parts=True)
    for small, big in [(pc["q1"], pc_big["q1"])] + list(zip(pc["acts1"], pc_big["acts1"])) + \
            [(pa[k], pa_big[k]) for k in ("actions_pi", "q1_pi", "dq_da")] + list(zip(pa["acts"] + pa["acts1"], pa_big["acts"] + pa_big["acts1"])):
        assert torch.equal(small, big[:n])
    # ---- each statement leaves the other network's .grad objects and contents alone
    for mine, other, call in ((ap, cp, lambda: dg.actor_backward(observations=obs)),
                              (cp, ap, lambda: dg.critic_backward(observations=obs, actions=act, target_q_values=y))):
        for i, p in enumerate(other):
            p.grad = None if i % 3 == 0 else torch.full_like(p, float(i + 1))
        kept = [None if p.grad is None else (p.grad, p.grad.clone()) for p in other]
        other_set = dg.grad_buffer[:dg.spec.n_actor] if other is ap else dg.grad_buffer[dg.spec.n_actor:]
        set_before = other_set.clone()
        call()
        for p, k in zip(other, kept):
            assert (p.grad is None) if k is None else (p.grad is k[0] and torch.equal(p.grad, k[1]))
        assert torch.equal(other_set, set_before) and all(p.grad is not None for p in mine)
    dg.close()


# ----------------------------------------------------------------------------------------------------------- 4. loss_scale
def test_loss_scale_doubles_the_critic_statement_exactly(rows):
    import torch
    mc = _cuda(G.model())
    one, half = _fused(mc, 1.0), _fused(mc, 0.5)
    obs, act, y = _t(torch, *G.batch(256, rows))
    l1 = one.critic_backward(observations=obs, actions=act, target_q_values=y)
    g1 = one.grad_buffer[one.spec.n_actor:].clone()
    lh = half.critic_backward(observations=obs, actions=act, target_q_values=y)
    gh = half.grad_buffer[half.spec.n_actor:]
    big = g1.abs() > 2.0 ** -120
    assert int(big.sum()) > 120000 and torch.equal(g1[big], 2.0 * gh[big]) and torch.equal(l1, 2.0 * lh) and float(l1) > 0
    a1, ah = one.actor_backward(observations=obs), half.actor_backward(observations=obs)          # the actor statement has no scale
    assert torch.equal(a1, ah) and torch.equal(one.grad_buffer[:one.spec.n_actor], half.grad_buffer[:half.spec.n_actor])
    one.close(); half.close()


# ----------------------------------------------------------------------------------------------------------- 5. live parameters
def test_reads_the_live_parameters(rows):
    import torch
    B = 100
    m = G.model()
    mc = _cuda(m)
    dg = _fused(mc)
    obs_np, act_np, y_np = G.batch(B, rows)
    obs, act, y = _t(torch, obs_np, act_np, y_np)
    before = _both(dg, mc, obs, act, y)
    gen = torch.Generator().manual_seed(5)
    with torch.no_grad():                      # in place, as an optimiser writes: no rebind
        for host, dev in zip(list(m.actor.mu.parameters()) + list(m.critic.q_networks[0].parameters()), _actor_params(mc) + _critic_params(mc)):
            assert host.shape == dev.shape
            delta = 0.02 * torch.randn(host.shape, generator=gen)
            host.add_(delta)
            dev.add_(delta.cuda())
    lc, pc = dg.critic_backward(observations=obs, actions=act, target_q_values=y, return_parts=True)
    acts = [a.cpu().numpy() for a in pc["acts1"]]
    ref, info = G.critic_grad(m, obs_np, act_np, y_np, other_acts=acts)
    G.assert_masks(info["ambiguous"], info["mask"], acts, "critic after an in-place change")
    G.assert_all_within(dict(_critic_grads(mc), critic_loss=lc, q1=pc["q1"]), ref, "critic after an in-place change")
    la, pa = dg.actor_backward(observations=obs, return_parts=True)
    hp = _host_parts(pa)
    ref, info = G.actor_grad(m, obs_np, other=hp)
    G.assert_actor_choices(info, hp, "actor after an in-place change")
    got = dict(_actor_grads(mc), actor_loss=la, **{k: pa[k] for k in G.PARTS})
    G.assert_all_within(got, {k: v for k, v in ref.items() if k in got}, "actor after an in-place change")
    after = [lc, pc["q1"]] + [p.grad for p in _critic_params(mc)]
    assert not any(torch.equal(a, b) for a, b in zip(after, [before[0], before[1]] + before[4:10]))
    dg.close()


# ----------------------------------------------------------------------------------------------------------- 6. one optimiser step
def _np(x):
    return x.detach().cpu().numpy().copy()


def _snap(opt, params):
    out = []
    for p in params:
        st = opt.state.get(p, {})
        zeros = np.zeros(tuple(p.shape), np.float32)
        out.append((_np(p), _np(st["exp_avg"]) if "exp_avg" in st else zeros, _np(st["exp_avg_sq"]) if "exp_avg_sq" in st else zeros, _np(p.grad)))
    return out


def test_one_gradient_step_with_the_fused_optimiser(rows):
    """critic_backward -> critic_step -> actor_backward -> actor_step(polyak=True) on the [400, 300] tensors: parameters, Adam
    moments and targets within optim_step_ref's bounds; step counts as stock torch's; the refreshes read the stepped values."""
    import torch
    from reinforcementlearning4meshgeneration_amd import FusedOptimStep, FusedPolicy, FusedTDTarget
    lr, tau, B = 1e-3, 0.005, 256
    mc, twin = _cuda(G.model()), _cuda(G.model())
    dg, fo = _fused(mc), FusedOptimStep.from_sb3(mc)
    td, policy = FusedTDTarget.from_sb3(mc), FusedPolicy.from_sb3(mc, sigma=0.0)
    policy.bind_live(mc)
    obs, act, y = _t(torch, *G.batch(B, rows))
    cp, ap = _critic_params(mc), _actor_params(mc)
    ctp, atp = list(mc.critic_target.q_networks[0].parameters()), list(mc.actor_target.mu.parameters())
    sc, top = O.scalars(1, lr=lr), {}
    for params, tparams, opt, topt, twin_params, backward, step in (
            (cp, ctp, mc.critic.optimizer, twin.critic.optimizer, _critic_params(twin),
             lambda: dg.critic_backward(observations=obs, actions=act, target_q_values=y), fo.critic_step),
            (ap, atp, mc.actor.optimizer, twin.actor.optimizer, _actor_params(twin),
             lambda: dg.actor_backward(observations=obs), lambda: fo.actor_step(polyak=True))):
        assert bool(torch.isfinite(backward()))
        before = _snap(opt, params)
        for q, p in zip(twin_params, params):
            q.grad = p.grad.clone()
        step()
        topt.step()
        for i, (p, q, b) in enumerate(zip(params, twin_params, before)):
            got = {"p": p, "exp_avg": opt.state[p]["exp_avg"], "exp_avg_sq": opt.state[p]["exp_avg_sq"]}
            O.worst(got, O.adam(*b, sc), f"tensor {i}", top)
            assert float(opt.state[p]["step"]) == float(topt.state[q]["step"]) == 1.0
            assert not np.array_equal(_np(p), b[0])
    # both Polyak pairs moved with the second launch, from the STEPPED parameters
    t0 = [_np(t) for t in list(twin.critic_target.q_networks[0].parameters()) + list(twin.actor_target.mu.parameters())]
    ratio = max(O.assert_within(_np(t), O.polyak(a, _np(p), tau), f"target {i}") for i, (t, a, p) in enumerate(zip(ctp + atp, t0, cp + ap)))
    assert all(not np.array_equal(_np(t), a) for t, a in zip(ctp + atp, t0))
    print(f"\nddpg one step: Adam max |kernel - fp64| / bound {top}; targets {ratio:.4f}")
    # the refreshes read the stepped values: the fused forward equals the stepped modules', not the old ones'
    zero = torch.zeros(B, 1, device="cuda")

    def fused_now():
        return (td.target(next_observations=obs, rewards=zero, dones=zero).reshape(-1),
                policy.forward(obs, deterministic=True)["buffer_actions"])
    y_stale, a_stale = fused_now()
    td.refresh(); policy.refresh()
    y_new, a_new = fused_now()
    with torch.no_grad():                      # (target_noise_clip = 0: the target takes no noise)
        want_y = mc.gamma * mc.critic_target.q_networks[0](torch.cat([obs, mc.actor_target.mu(obs)], dim=1))[:, 0]
        want_a = mc.actor.mu(obs)
        old_y = twin.gamma * twin.critic_target.q_networks[0](torch.cat([obs, twin.actor_target.mu(obs)], dim=1))[:, 0]
        old_a = twin.actor_target.mu(obs)      # the twin's target actor was never stepped: the actor before the step
    err = lambda a, b: float((a - b).abs().max())   # noqa: E731
    assert err(y_stale, old_y) < 1e-5 and err(a_stale, old_a) < 1e-5           # before the refreshes: the values of the bind
    assert err(y_new, want_y) < 1e-5 and err(a_new, want_a) < 1e-5             # after them: the stepped ones
    assert err(y_new, y_stale) > 10 * err(y_new, want_y) and err(a_new, a_stale) > 10 * err(a_new, want_a)
    fo.close(); dg.close(); td.close(); policy.close()


# ----------------------------------------------------------------------------------------------------------- 7. the example
def _example(name, *flags):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", name), *flags], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


def test_example_check_against_the_td3_example():
    """examples/ddpg_train_step.py --check exits 0 and its fused-minus-stock parameter difference lies within what the same
    flags give examples/td3_train_step.py --check on this machine, times the ratio of the optimiser step counts.

    The same flags include --policy-delay 1, DDPG's value, which both examples take: the difference is the rounding of the
    optimiser and Polyak launches (both twins are fed the gradients the fused calls left), it grows with their number, and
    TD3's default policy_delay 2 runs half the actor steps and Polyak updates.  Measured at these flags on the MI355X: DDPG
    1.043e-07 after [8, 8] steps; TD3 at policy_delay 1 1.043e-07 after [8, 8]; TD3 at its default policy_delay 2 4.470e-08
    after [8, 4], where neither the ratio of the summed step counts (1.33) nor that of the actor steps (2) covers the 7 : 3
    units in the last place between them; at 16 steps each both print 1.788e-07."""
    flags = ("--envs", "64", "--chunk", "8", "--iterations", "2", "--gradient-steps", "4", "--batch", "100", "--policy-delay", "1",
             "--check")
    ddpg, td3 = _example("ddpg_train_step.py", *flags), _example("td3_train_step.py", *flags)
    steps = sum(ddpg["optimizer_steps"]) / sum(td3["optimizer_steps"])
    assert ddpg["optimizer_steps"] == td3["optimizer_steps"] and steps == 1.0
    d, t = ddpg["max_abs_fused_minus_stock_parameter"], td3["max_abs_fused_minus_stock_parameter"]
    print(f"\nexamples --check: ddpg {d:.3e} after {ddpg['optimizer_steps']} steps, td3 {t:.3e} after {td3['optimizer_steps']}; ratio of steps {steps:.2f}")
    assert ddpg["optimizer_steps"] == [8.0, 8.0] and np.isfinite([ddpg["last_critic_loss"], ddpg["last_actor_loss"]]).all()
    assert 0.0 <= d <= t * steps, (d, t, steps)
