"""GPU: the fused PPO / A2C loss statement (csrc/meshenv_ppo_grad.h: k_ppo_adv_stats, k_ppo_grad, k_ppo_grad_reduce,
k_ppo_grad_clip) against the fp64 restatement of tests/ppo_grad_ref.py, every output, gradient and part within its own bound;
the ReLU and pass masks; both branches of the clip launch; determinism, a side stream, overwrite semantics and untouched
inputs; live parameters; eager torch and a stock Adam step.  Each test prints max |kernel - fp64| / bound.

Batch sizes: 1 (no normalisation, 15 padded rows), 17 (a one-row second tile), the recipes' 100 and 256, 4101 (257 tiles: more
tiles than workgroups and a partial last tile)."""
import copy

import numpy as np
import pytest

import policy_ref as R
import ppo_grad_ref as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rows():
    return R.input_rows()


def _cuda(m):
    import torch
    d = {k: v for k, v in m.items() if k in ("act", "H", "a2c")}
    d.update(pi=[copy.deepcopy(l).cuda() for l in m["pi"]], vf=[copy.deepcopy(l).cuda() for l in m["vf"]],
             action_net=copy.deepcopy(m["action_net"]).cuda(), value_net=copy.deepcopy(m["value_net"]).cuda(),
             log_std=torch.nn.Parameter(m["log_std"].detach().clone().cuda()))
    return d


def _fused(mc):
    from reinforcementlearning4meshgeneration_amd.ppo_grad import FusedPPOGrad
    return FusedPPOGrad.actor_critic(mc["pi"], mc["vf"], mc["action_net"], mc["value_net"], mc["log_std"], mc["act"])


def _hp(m, **kw):
    kw.setdefault("max_grad_norm", P.MAX_GRAD_NORM)
    return P.hyper(clip_range=None if m["a2c"] else 0.2, **kw)


def _dev(data):
    import torch
    return {k: torch.from_numpy(v).cuda() for k, v in data.items()}


def _call(pg, dd, hp, **kw):
    return pg.backward(observations=dd["observations"], actions=dd["actions"], old_log_prob=dd["old_log_prob"],
                       advantages=dd["advantages"], returns=dd["returns"], **hp, **kw)


def _got(mc, res):
    g = {k: p.grad for k, p in zip(P.GRADS, P.params(mc))}
    g.update({k: res[k] for k in (*P.SCALARS, *P.PARTS) if k in res})
    return P.with_acts(dict(g, acts_pi=res["acts_pi"], acts_vf=res["acts_vf"])) if "acts_pi" in res else g


def _host_parts(res):
    out = {k: [a.cpu().numpy() for a in res[k]] for k in ("acts_pi", "acts_vf")}
    out["pass"] = res["pass"].cpu().numpy()
    return out


def _fmt(worst):
    top = sorted(worst.items(), key=lambda kv: -kv[1])
    return f"max {top[0][1]:.4f} ({top[0][0]}) " + " ".join(f"{k}={v:.3f}" for k, v in sorted(worst.items()))


# ----------------------------------------------------------------------------------------------------------- 1. fp64, masks
@pytest.mark.parametrize("case,stress", [(c, s) for c in P.CASES for s in (False, True) if not s or c in P.BOTH_SETS])
def test_outputs_gradients_and_parts_against_fp64(case, stress, rows):
    import torch
    m = P.modules(case, stress)
    mc = _cuda(m)
    pg = _fused(mc)
    hp = _hp(m)
    worst = {}
    for B in P.GPU_BS:
        what = f"{case} {'stress' if stress else 'default'} B={B}"
        data = P.batch(m, B, rows)
        dd = _dev(data)
        res = _call(pg, dd, hp, return_parts=True)
        assert all(res[k].shape == () and res[k].dtype == torch.float32 and res[k].is_cuda for k in P.SCALARS)
        assert all(res[k].shape == (B,) for k in (*P.PARTS, "pass")) and [tuple(a.shape) for k in ("acts_pi", "acts_vf") for a in res[k]] == [(B, m["H"])] * 4
        hparts = _host_parts(res)
        ref, info = P.ppo_grad(m, data, hp, other=hparts)
        P.assert_conditions(info, what)                                            # from the reference alone
        P.assert_choices(info, hparts, what)                                       # the masks off the ambiguous sets
        w = {}
        P.assert_all_within(_got(mc, res), ref, what, w)
        assert set(w) == set(ref)
        print(f"\nppo grad {what}: {P.describe(info)}; |kernel - fp64| / bound: {_fmt(w)}")
        for k, v in w.items():
            worst[k] = max(worst.get(k, 0.0), v)
        want = [p.grad.clone() for p in P.params(mc)]
        res2 = _call(pg, dd, hp)                                                   # no parts: the same bits
        assert all(torch.equal(res2[k], res[k]) for k in P.SCALARS) and all(torch.equal(p.grad, g) for p, g in zip(P.params(mc), want)), what
    print(f"\nppo grad {case} {'stress' if stress else 'default'} over all B: {_fmt(worst)}")
    pg.close()


# ----------------------------------------------------------------------------------------------------------- 2. the clip launch
@pytest.mark.parametrize("case", P.BOTH_SETS)
def test_clip_launch_both_branches(case, rows):
    import torch
    B = 256
    m = P.modules(case)
    mc = _cuda(m)
    pg = _fused(mc)
    data = P.batch(m, B, rows)
    dd = _dev(data)
    res0 = _call(pg, dd, _hp(m, max_grad_norm=None), return_parts=True)
    assert bool(torch.isnan(res0["grad_norm"]))
    hparts = _host_parts(res0)
    raw = [p.grad.clone() for p in P.params(mc)]
    for mgn in (50.0, 0.02):                                                       # firmly above the norm, firmly below it
        hp = _hp(m, max_grad_norm=mgn)
        ref, info = P.ppo_grad(m, data, hp, other=hparts)
        P.assert_conditions(info, f"{case} max_grad_norm={mgn}")
        res = _call(pg, dd, hp)
        w = {}
        P.assert_all_within(_got(mc, res), ref, f"{case} max_grad_norm={mgn}", w, names=(*P.SCALARS, *P.GRADS))
        same = all(torch.equal(p.grad, g) for p, g in zip(P.params(mc), raw))
        assert same == (mgn > 1.0)                                                 # coef = 1: bit-identical; else scaled
        print(f"\nppo clip {case} max_grad_norm={mgn}: norm {float(res['grad_norm']):.5f}; {_fmt(w)}")
    pg.close()


# ----------------------------------------------------------------------------------------------------------- 3. plumbing
@pytest.mark.parametrize("B", [17, 4101])
def test_repeat_side_stream_overwrite_and_untouched_inputs(B, rows):
    import torch
    m = P.modules("ppo-relu128")
    mc = _cuda(m)
    pg = _fused(mc)
    hp = _hp(m)
    dd = _dev(P.batch(m, B, rows))
    kept = {k: v.clone() for k, v in dd.items()}
    ps = P.params(mc)
    assert all(p.grad is None for p in ps)
    r0 = _call(pg, dd, hp)
    want = [p.grad.clone() for p in ps]
    assert len(ps) == 13 and all(float(g.abs().max()) > 0 for g in want)
    assert all(p.grad.data_ptr() == pg.grad_buffer.data_ptr() + 4 * at for p, at in pg.spec.offsets())   # views of one buffer

    def same(r):
        return all(torch.equal(r[k], r0[k]) for k in P.SCALARS) and all(torch.equal(p.grad, w) for p, w in zip(ps, want))
    assert same(_call(pg, dd, hp))                                                 # a bit-identical repeat
    pg.grad_buffer.fill_(float("nan"))                                            # stale garbage in the buffer
    assert same(_call(pg, dd, hp))
    mine = [torch.full_like(p, float("nan")) for p in ps]                         # a caller's own tensors in p.grad
    for p, g in zip(ps, mine):
        p.grad = g
    assert same(_call(pg, dd, hp))
    assert all(p.grad is not g and bool(torch.isnan(g).all()) for p, g in zip(ps, mine))   # replaced by the view, not written
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        pg.grad_buffer.zero_()
        rs = _call(pg, dd, hp)
    side.synchronize()
    assert same(rs)
    assert all(torch.equal(dd[k], kept[k]) for k in dd)                            # no argument is written
    pg.close()


# ----------------------------------------------------------------------------------------------------------- 4. live parameters
def test_reads_the_live_parameters_and_rebinds_after_to(rows):
    import torch
    B = 100
    m = P.modules("ppo-relu128")
    mc = _cuda(m)
    pg = _fused(mc)
    hp = _hp(m)
    data = P.batch(m, B, rows)
    dd = _dev(data)
    r0 = _call(pg, dd, hp)
    before = [p.grad.clone() for p in P.params(mc)]
    with torch.no_grad():                      # in place, as an optimiser writes: no rebind
        for mm in (m, mc):
            mm["pi"][1].weight.mul_(1.25)
            mm["value_net"].bias.add_(0.125)
            mm["log_std"].add_(0.25)
    res = _call(pg, dd, hp, return_parts=True)
    hparts = _host_parts(res)
    ref, info = P.ppo_grad(m, data, hp, other=hparts)
    P.assert_choices(info, hparts, "after an in-place change")
    P.assert_all_within(_got(mc, res), ref, "after an in-place change")
    assert not torch.equal(res["loss"], r0["loss"]) and not all(torch.equal(p.grad, b) for p, b in zip(P.params(mc), before))
    # .to() reallocates: the spec's tensors are replaced and bind() records the new pointers
    for l in (*mc["pi"], *mc["vf"], mc["action_net"], mc["value_net"]):
        for p in (l.weight, l.bias):
            p.data = p.data.clone()
    mc["log_std"].data = mc["log_std"].data.clone()
    pg.bind()
    res2 = _call(pg, dd, hp)
    assert all(torch.equal(res2[k], res[k]) for k in P.SCALARS)
    pg.close()


# ----------------------------------------------------------------------------------------------------------- 5. eager torch, Adam
@pytest.mark.parametrize("case", P.BOTH_SETS)
@pytest.mark.parametrize("B", [64, 256, 4101])
def test_against_eager_torch_and_a_stock_adam_step(B, case, rows):
    import torch
    m = P.modules(case)
    mc, me = _cuda(m), _cuda(m)
    pg = _fused(mc)
    hp = _hp(m)
    data = P.batch(m, B, rows)
    dd = _dev(data)
    res = _call(pg, dd, hp, return_parts=True)
    ref, info = P.ppo_grad(m, data, hp, other=_host_parts(res))
    P.assert_conditions(info, f"{case} B={B}")
    e = P.eager(torch, me, data, hp)
    names = (*P.SCALARS, *P.GRADS)
    wf, we = {}, {}
    P.assert_all_within(_got(mc, res), ref, f"{case} B={B} fused", wf, names=names)
    P.assert_all_within(e, ref, f"{case} B={B} eager", we, names=names)
    print(f"\nppo grad vs eager {case} B={B}: fused {_fmt(wf)}\n  eager {_fmt(we)}")
    # one stock optimiser step on each side: the parameters agree within twice the one-step bound of optim_step_ref
    pf, pe = P.params(mc), P.params(me)
    lr, betas, eps = 3e-4, (0.9, 0.999), 1e-5
    torch.optim.Adam(pf, lr=lr, betas=betas, eps=eps).step()
    torch.optim.Adam(pe, lr=lr, betas=betas, eps=eps).step()
    p0 = P.params(_cuda(m))
    capped = {}
    for k, a, b, p in zip(P.GRADS, pf, pe, p0):
        st = {}
        bound = P.adam_step_bound(p.detach().cpu().numpy(), np.asarray(ref[k][0]), np.asarray(ref[k][1]), lr, betas, eps, st)
        capped[k] = st["capped"]
        d = (a.detach() - b.detach()).abs().cpu().numpy().astype(np.float64)
        assert (d <= 2.0 * bound.reshape(d.shape)).all(), (case, B, k, float((d / np.maximum(2.0 * bound.reshape(d.shape), 1e-300)).max()))
        assert not torch.equal(a, p)                                               # and the step moved them
    print(f"  share of elements whose one-step bound is the cap of 2 lr (a gradient within its bound of 0): "
          + " ".join(f"{k}={v:.4f}" for k, v in capped.items()))
    pg.close()
