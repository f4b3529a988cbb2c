"""Host only: the fp64 restatement of the RMSprop step (tests/rmsprop_ref.py) against stock torch.optim.RMSprop on the CPU;
its bound against a float32 evaluation and against named mistakes; the host scalars; the state OptimStepSpec creates; the
``step`` increments; every refusal; the ``policy`` program and the ``from_sb3`` routing; the messages that stay."""
import copy
import ctypes
import types

import numpy as np
import pytest
import torch

import on_policy_stubs as S
import rl_stubs
import rmsprop_ref as Q

CASES = ["empty", "three_steps", "loaded"]


def _states(loaded, base=50):
    return [Q.state(s, seed=base + i, loaded=loaded) for i, s in enumerate(Q.SHAPES)]


def _stock(ts, loaded, step=6, cls=torch.optim.RMSprop, **kw):
    """A stock single-tensor RMSprop on CPU copies of ts ([(p, v, g)]), its state loaded when asked, gradients set."""
    params = [torch.from_numpy(p.copy()).requires_grad_(True) for p, _, _ in ts]
    opt = cls(params, lr=Q.LR, alpha=Q.ALPHA, eps=Q.EPS, foreach=False, **kw)
    if loaded:
        sd = opt.state_dict()
        sd["state"] = {i: {"step": torch.tensor(float(step)), "square_avg": torch.from_numpy(v.copy())} for i, (_, v, _) in enumerate(ts)}
        opt.load_state_dict(sd)
    for q, (_, _, g) in zip(params, ts):
        q.grad = torch.from_numpy(g.copy())
    return params, opt


def _np(x):
    return x.detach().numpy().copy()


def _snap(opt, params):
    return [(_np(q), _np(opt.state[q]["square_avg"]) if "square_avg" in opt.state.get(q, {}) else np.zeros(tuple(q.shape), np.float32),
             _np(q.grad)) for q in params]


# ----------------------------------------------------------------------------------------------------------- 1. stock torch
@pytest.mark.parametrize("case", CASES)
def test_stock_rmsprop_lies_within_the_bound(case):
    ts = _states(case == "loaded")
    params, opt = _stock(ts, case == "loaded")
    sc = Q.scalars()
    top = 0.0
    for step in range(1, 4 if case == "three_steps" else 2):
        if step > 1:
            for i, q in enumerate(params):
                q.grad = torch.from_numpy(Q.state(tuple(q.shape), seed=900 + 31 * step + i)[2].copy())
        before = _snap(opt, params)
        opt.step()
        for i, (q, b) in enumerate(zip(params, before)):
            st = opt.state[q]
            assert list(st) == ["step", "square_avg"] and float(st["step"]) == step + (6 if case == "loaded" else 0)
            top = max(top, Q.worst({"p": q, "square_avg": st["square_avg"]}, Q.rmsprop(*b, sc), f"{case} step {step} tensor {i}"))
    print(f"\nstock RMSprop on the CPU, {case}: max |torch - fp64| / bound = {top:.4f}")
    assert top > 0.0                                     # not a comparison of the reference with itself


@pytest.mark.parametrize("loaded", [False, True], ids=["empty", "loaded"])
def test_bound_admits_the_float32_restatement(loaded):
    sc = Q.scalars()
    for i, (p, v, g) in enumerate(_states(loaded)):
        ref = Q.rmsprop(p, v, g, sc)
        assert Q.worst(Q.rmsprop_f32(p, v, g, sc), ref, f"tensor {i} fp32") >= 0.0
        zero = (g == 0) & (v == 0)                        # v' = 0 exactly: s = 0 with no error, r = 0, nothing moves
        assert (ref["square_avg"][0][zero] == 0).all() and np.array_equal(ref["p"][0][zero], p[zero].astype(np.float64))


# ----------------------------------------------------------------------------------------------------------- 2. mutants
@pytest.mark.parametrize("loaded", [False, True], ids=["empty", "loaded"])
@pytest.mark.parametrize("mutant", Q.MUTANTS)
def test_bound_rejects_rmsprop_mistakes(mutant, loaded):
    caught = []
    for i, (p, v, g) in enumerate(_states(loaded)):
        ref = Q.rmsprop(p, v, g, Q.scalars())
        bad = Q.rmsprop(p, v, g, Q.scalars(mutant=mutant), mutant=mutant, step=7 if loaded else 1)
        caught += [k for k in ref if Q.ratio(bad[k][0], ref[k])[1].any()]
        assert not any(Q.ratio(ref[k][0], ref[k])[1].any() for k in ref)
    assert caught, f"the bound admits the mutant {mutant}"
    assert "p" in caught                                  # every one of them moves the parameter out of its bound


def test_the_tf_like_order_is_a_mistake_here():
    """SB3's RMSpropTFLike adds eps under the root: a different optimiser, refused by type and outside the bound."""
    p, v, g = Q.state((4097,), seed=3, loaded=True)
    ref = Q.rmsprop(p, v, g, Q.scalars())
    f = np.float32
    v1 = v * f(0.99) + (f(1 - 0.99) * g) * g
    tf_like = p + f(-Q.LR) * (g / np.sqrt(v1 + f(Q.EPS)))
    assert Q.ratio(tf_like, ref["p"])[1].any()


# ----------------------------------------------------------------------------------------------------------- 3. the host half
def test_commit_passes_float_rounded_scalars_and_steps_once():
    from reinforcementlearning4meshgeneration_amd.optim_step import RMSPROP, OptimStepSpec
    ts = _states(True)
    params, opt = _stock(ts, True)
    spec = OptimStepSpec(policy=opt)
    assert [s.op for s in spec.segments("policy")] == [RMSPROP] * len(Q.SHAPES) and [s.block for s in spec.segments("policy")] == [0] * 7
    plan = spec.prepare("policy")
    assert all(float(opt.state[q]["step"]) == 6 for q in params)               # prepare steps nothing
    for r, q in zip(plan.rows, params):                                         # (param, grad, no exp_avg, square_avg, no target)
        assert r.tensors[0] is q and r.tensors[1] is q.grad and r.tensors[2] is None and r.tensors[3] is opt.state[q]["square_avg"]
        assert r.tensors[4] is None and r.pointers[2] == 0 and r.pointers[4] == 0
    opt.param_groups[0]["lr"] = 2e-3                                            # read at the call, as SB3 rewrites it
    sc = spec.commit(plan)
    assert all(float(opt.state[q]["step"]) == 7 and opt.state[q]["step"].device.type == "cpu" for q in params)
    want = Q.scalars(lr=2e-3)
    assert (sc.step_size[0], sc.beta2[0], sc.w2[0], sc.eps[0]) == (want.lr, want.al, want.w2, want.eps)
    assert ctypes.sizeof(sc) == 4 * (6 * 4 + 2)                                 # MeshOptimScalars keeps its layout
    spec.commit(spec.prepare("policy"))
    assert all(float(opt.state[q]["step"]) == 8 for q in params)


def test_state_created_matches_init_group():
    from reinforcementlearning4meshgeneration_amd.optim_step import OptimStepSpec
    ts = _states(False)
    mine, opt_m = _stock(ts, False)
    theirs, opt_t = _stock(ts, False)
    OptimStepSpec(policy=opt_m).prepare("policy")
    opt_t.step()
    for a, b in zip(mine, theirs):
        sa, sb = opt_m.state[a], opt_t.state[b]
        assert list(sa) == list(sb) == ["step", "square_avg"]
        for k in sa:
            assert sa[k].dtype == sb[k].dtype and sa[k].device == sb[k].device and sa[k].shape == sb[k].shape, k
        assert float(sa["step"]) == 0.0 and not sa["square_avg"].any()
    sd_m, sd_t = opt_m.state_dict(), opt_t.state_dict()
    assert sd_m["state"].keys() == sd_t["state"].keys() and sd_m["param_groups"] == sd_t["param_groups"]
    opt_m.step()                                           # and stock torch steps from it
    assert all(torch.equal(a, b) for a, b in zip(mine, theirs))


def test_rmsprop_in_every_slot_and_adam_beside_it():
    from reinforcementlearning4meshgeneration_amd.optim_step import ADAM, PROGRAMS, RMSPROP, OptimStepSpec
    assert PROGRAMS == ("critic", "actor_polyak", "actor", "polyak", "policy")  # appended: the existing indices stay
    _, rms = _stock(_states(False), False)
    pa, adam = _opt()
    spec = OptimStepSpec(critic=rms, actor=[adam, _stock(_states(False), False)[1]], policy=adam)
    assert [s.op for s in spec.segments("critic")] == [RMSPROP] * 7
    assert [(s.op, s.block) for s in spec.segments("actor")] == [(ADAM, 0)] * 2 + [(RMSPROP, 1)] * 7
    assert [s.op for s in spec.segments("policy")] == [ADAM] * 2
    sc = spec.commit(spec.prepare("actor"))
    want = Q.scalars()
    assert (sc.step_size[1], sc.beta2[1], sc.w2[1], sc.eps[1]) == (want.lr, want.al, want.w2, want.eps)
    assert sc.step_size[0] == np.float32(1e-3 / (1 - 0.9)) and sc.beta2[0] == np.float32(0.999)


# ----------------------------------------------------------------------------------------------------------- 4. refusals
def _opt(n=2, cls=torch.optim.Adam, grads=True, **kw):
    ps = [torch.zeros(4, 3, requires_grad=True) for _ in range(n)]
    if grads:
        for p in ps:
            p.grad = torch.ones_like(p)
    return ps, cls(ps, lr=1e-3, **kw)


def _rms(**kw):
    return _opt(cls=torch.optim.RMSprop, **kw)


def _refused(fn, *words):
    with pytest.raises(ValueError) as e:
        fn()
    for w in words:
        assert w in str(e.value), (w, str(e.value))


class RMSpropTFLike(torch.optim.RMSprop):
    """Named as SB3's: a subclass of its own, as there."""


def test_rmsprop_refusals_at_construction_name_what_was_found():
    from reinforcementlearning4meshgeneration_amd.optim_step import OptimStepSpec as Spec
    for slot in ("critic", "policy"):
        _refused(lambda: Spec(**{slot: _rms(momentum=0.9)[1]}), f"the {slot} optimiser", "momentum=0.9", "torch.optim.RMSprop")
        _refused(lambda: Spec(**{slot: _rms(centered=True)[1]}), "centered=True")
        _refused(lambda: Spec(**{slot: _rms(weight_decay=0.01)[1]}), "weight_decay=0.01")
        for flag in ("maximize", "capturable", "differentiable"):
            _refused(lambda: Spec(**{slot: _rms(**{flag: True})[1]}), f"{flag}=True")
    _refused(lambda: Spec(actor=[_rms(momentum=0.5)[1]]), "actor-step optimiser 0", "momentum=0.5")
    ps, o = _rms()
    o.add_param_group({"params": [torch.zeros(2, requires_grad=True)]})
    _refused(lambda: Spec(policy=o), "2 param groups", "torch.optim.RMSprop")
    _refused(lambda: Spec(policy=torch.optim.RMSprop([torch.zeros(3, dtype=torch.float64, requires_grad=True)])), "float64", "(3,)")
    _refused(lambda: Spec(policy=torch.optim.RMSprop([torch.zeros(4, 6)[:, ::2].requires_grad_(True)])), "not contiguous", "(4, 3)")
    _refused(lambda: Spec(policy=_opt(cls=RMSpropTFLike)[1]), "RMSpropTFLike", "not torch.optim.Adam")
    ps, o = _rms()
    _refused(lambda: Spec(actor=[o], polyak=[(ps, [torch.zeros(4, 3), torch.zeros(4, 3)])]), "RMSprop", "Polyak")
    Spec(critic=o, polyak=[([torch.zeros(4, 3)], [torch.zeros(4, 3)])])          # pairs it does not step are fine


def test_rmsprop_refusals_at_the_call_name_what_was_found():
    from reinforcementlearning4meshgeneration_amd.optim_step import OptimStepSpec
    ps, o = _rms()
    spec = OptimStepSpec(policy=o)
    spec.prepare("policy")
    ps[1].grad = None
    _refused(lambda: spec.prepare("policy"), "the policy optimiser", "parameter 1", ".grad None")
    ps[1].grad = torch.ones(4, 6)[:, ::2]
    _refused(lambda: spec.prepare("policy"), "parameter 1", "not contiguous")
    ps[1].grad = torch.ones(4, 3)
    o.state[ps[1]]["step"] += 1
    _refused(lambda: spec.prepare("policy"), "differs between its parameters", "[0.0, 1.0]")
    o.state[ps[0]]["step"] += 1
    spec.prepare("policy")
    for key, value in (("momentum", 0.9), ("centered", True), ("weight_decay", 0.1), ("maximize", True)):   # edited after the bind
        old, o.param_groups[0][key] = o.param_groups[0][key], value
        _refused(lambda: spec.prepare("policy"), f"{key}={value!r}")
        o.param_groups[0][key] = old
    o.param_groups[0]["lr"] = torch.tensor(1e-3)
    _refused(lambda: spec.prepare("policy"), "lr, alpha and eps must be Python floats")
    o.param_groups[0]["lr"] = 1e-3
    good = dict(o.state[ps[0]])
    o.state[ps[0]]["momentum_buffer"] = torch.zeros(4, 3)
    _refused(lambda: spec.prepare("policy"), "parameter 0", "momentum_buffer", "'step' and 'square_avg' alone")
    for bad, word in ((torch.zeros(4, 3, dtype=torch.float64), "square_avg"), (torch.zeros(3, 4), "square_avg"),
                      (torch.zeros(4, 6)[:, ::2], "square_avg"), (torch.zeros(4, 3, device="meta"), "square_avg")):
        o.state[ps[0]].clear()
        o.state[ps[0]].update(good, square_avg=bad)
        _refused(lambda: spec.prepare("policy"), "parameter 0", f"state[{word!r}]", "float32 contiguous tensor like the parameter")
    o.state[ps[0]].clear()
    o.state[ps[0]].update(good, step=torch.zeros((), device="meta"))
    _refused(lambda: spec.prepare("policy"), "state['step'] is not a CPU tensor")
    o.state[ps[0]].clear()
    o.state[ps[0]].update(good)
    spec.prepare("policy")


def test_messages_that_stay():
    """The refusals of other optimiser types and of objects that are no SB3 model: the words the existing tests match."""
    from reinforcementlearning4meshgeneration_amd.optim_step import FusedOptimStep, OptimStepSpec as Spec
    _refused(lambda: Spec(critic=_opt(cls=torch.optim.SGD)[1]), "the critic optimiser", "torch.optim.sgd.SGD", "not torch.optim.Adam")
    _refused(lambda: Spec(critic=_opt(cls=torch.optim.AdamW)[1]), "torch.optim.adamw.AdamW", "not torch.optim.Adam")
    _refused(lambda: Spec(policy=_opt(cls=torch.optim.SGD)[1]), "the policy optimiser", "torch.optim.sgd.SGD", "not torch.optim.Adam")
    _refused(lambda: Spec.from_sb3(types.SimpleNamespace(policy=None)), "not an SB3 SAC, TD3 or DDPG model")
    _refused(lambda: Spec.from_sb3(types.SimpleNamespace()), "not an SB3 SAC, TD3 or DDPG model")
    _refused(lambda: Spec(critic=_opt(amsgrad=True)[1]), "amsgrad=True", "torch.optim.Adam with one param group")
    # "nothing bound": policy_step on an off-policy binding, critic_step on an on-policy one
    ps, o = _opt()
    _refused(lambda: Spec(critic=o).prepare("policy"), "nothing bound for 'policy'", "no policy optimiser")
    _refused(lambda: Spec(policy=o).prepare("critic"), "nothing bound for 'critic'", "no critic optimiser")
    _refused(lambda: Spec(policy=o).prepare("actor"), "no actor optimisers")
    _refused(lambda: Spec(policy=o).prepare("polyak"), "no Polyak pairs")
    assert callable(FusedOptimStep.policy_step) and callable(FusedOptimStep.on_policy)


# ----------------------------------------------------------------------------------------------------------- 5. from_sb3
def _with_optimizers(m, kind):
    """rl_stubs' SAC / TD3 models carry no optimisers: give them SB3's."""
    def params(x):
        parts = list(getattr(x, "q_networks", [])) or [getattr(x, k) for k in ("latent_pi", "mu", "log_std") if hasattr(x, k)]
        return [p for part in parts for p in part.parameters()]
    m.actor.optimizer = torch.optim.Adam(params(m.actor), lr=3e-4)
    m.critic.optimizer = torch.optim.Adam(params(m.critic), lr=3e-4)
    m.tau = 0.005
    if kind == "sac":
        m.ent_coef_optimizer = torch.optim.Adam([m.log_ent_coef], lr=3e-4)
    return m


def test_from_sb3_routes_the_four_model_shapes():
    from reinforcementlearning4meshgeneration_amd import optim_step as M
    for kind, op, n_blocks in (("ppo", M.ADAM, 1), ("a2c", M.RMSPROP, 1)):
        model, params = S.model(kind)
        for obj in (model, model.policy):                                       # the model, or its ActorCriticPolicy
            s = M.OptimStepSpec.from_sb3(obj)
            assert s.policy is model.policy.optimizer and s.critic is None and s.actor == [] and s.pairs == []
            seg = s.segments("policy")
            assert [x.op for x in seg] == [op] * 13 and all(x.param is p for x, p in zip(seg, params))
            assert all(s.segments(k) == [] for k in ("critic", "actor", "actor_polyak", "polyak"))
            _refused(lambda: s.prepare("critic"), "nothing bound", "no critic optimiser")
    model, _ = S.model("a2c")
    model.policy.optimizer = RMSpropTFLike(model.policy.optimizer.param_groups[0]["params"], lr=7e-4)
    _refused(lambda: M.OptimStepSpec.from_sb3(model), "the policy optimiser", "RMSpropTFLike", "not torch.optim.Adam")
    model, _ = S.model("ppo")
    model.policy.optimizer = None                                               # no optimiser: not the on-policy route
    _refused(lambda: M.OptimStepSpec.from_sb3(model), "not an SB3 SAC, TD3 or DDPG model")
    sac = _with_optimizers(rl_stubs.sac_model(H=16, nl=2), "sac")
    s = M.OptimStepSpec.from_sb3(sac)
    assert s.policy is None and s.critic is sac.critic.optimizer and s.actor == [sac.actor.optimizer, sac.ent_coef_optimizer]
    assert s.segments("policy") == [] and len(s.pairs) == 12
    _refused(lambda: s.prepare("policy"), "nothing bound for 'policy'")
    td3 = _with_optimizers(rl_stubs.td3_model(H=16, nl=2), "td3")
    td3.actor.mu = td3.actor.mu                                                  # (parameters through .mu: no parameters())
    s = M.OptimStepSpec.from_sb3(td3)
    assert s.policy is None and s.critic is td3.critic.optimizer and s.actor == [td3.actor.optimizer] and len(s.pairs) == 12 + 6
    _refused(lambda: s.prepare("policy"), "nothing bound for 'policy'")
    # a SAC model whose .policy is SB3's SACPolicy (no mlp_extractor) still takes the off-policy route
    sac.policy = types.SimpleNamespace(actor=sac.actor, critic=sac.critic, optimizer=None)
    assert M.OptimStepSpec.from_sb3(sac).critic is sac.critic.optimizer


def test_no_cpu_fallback():
    from reinforcementlearning4meshgeneration_amd import _capi
    from reinforcementlearning4meshgeneration_amd.optim_step import FusedOptimStep, OptimStepSpec
    spec = OptimStepSpec(policy=_rms()[1])
    with pytest.raises(ValueError, match="is on cpu"):
        spec.check_device(torch.device("cuda", 0))
    if not torch.cuda.is_available():
        with pytest.raises(_capi.MeshEnvError):
            FusedOptimStep.on_policy(_rms()[1])
    assert copy.copy(spec.policy) is not None
