"""Host only: the fp64 restatement of the SAC actor / entropy-coefficient kernel (tests/actor_grad_ref.py) against torch
float64 autograd of SB3's statements; its bound against a second fp32 evaluation and against named mistakes; the conditions
of every case the GPU test uses; ActorGradSpec on SB3-shaped stub models."""
import copy
import types

import numpy as np
import pytest
import torch

import actor_grad_ref as A
import policy_ref as R
import td_target_ref as T

GPU_BS = (1, 15, 16, 17, 100, 256, 4101)          # tests/test_gpu_actor_grad.py
STRESS_MAX_B = 256
LEC = -0.5                                        # log_ent_coef of the cases: ent_coef = 0.61


@pytest.fixture(scope="module")
def rows():
    return R.input_rows()


def _torch_f64(m, obs, eps, log_ent_coef, target_entropy=-3.0):
    """SB3's statements transcribed in float64 on copies of the CPU modules, torch.distributions.Normal and autograd."""
    d = lambda l: copy.deepcopy(l).double()   # noqa: E731
    lin, mu, ls = [d(l) for l in m["lin"]], d(m["mu"]), d(m["ls"])
    qs = [[d(l) for l in m[f"q{c}"]] for c in (1, 2)]
    x, e = torch.from_numpy(obs).double(), torch.from_numpy(eps).double()
    lec = torch.tensor([float(np.float32(log_ent_coef))], dtype=torch.float64, requires_grad=True)
    h = x
    for l in lin:
        h = torch.relu(l(h))
    mean, log_std = mu(h), torch.clamp(ls(h), -20.0, 2.0)
    dist = torch.distributions.Normal(mean, log_std.exp())
    g = mean + log_std.exp() * e                      # rsample with the shared eps
    a = torch.tanh(g)
    log_prob = dist.log_prob(g).sum(dim=1) - torch.log(1.0 - a ** 2 + 1e-6).sum(dim=1)
    ent_coef = torch.exp(lec.detach())
    ent_coef_loss = -(lec * (log_prob + target_entropy).detach()).mean()
    a.retain_grad()
    xin = torch.cat([x, a], dim=1)
    qv = []
    for q in qs:
        hc = xin
        for l in q[:-1]:
            hc = torch.relu(l(hc))
        qv.append(q[-1](hc))
    min_q, _ = torch.min(torch.cat(qv, dim=1), dim=1, keepdim=True)
    actor_loss = (ent_coef * log_prob.reshape(-1, 1) - min_q).mean()
    actor_loss.backward()
    ent_coef_loss.backward()
    out = {"actor_loss": actor_loss.detach().numpy(), "ent_coef_loss": ent_coef_loss.detach().numpy(), "ent.grad": lec.grad.numpy(),
           "actions_pi": a.detach().numpy(), "log_prob": log_prob.detach().numpy(), "q1_pi": qv[0].detach().numpy()[:, 0],
           "q2_pi": qv[1].detach().numpy()[:, 0], "mu.w": mu.weight.grad.numpy(), "mu.b": mu.bias.grad.numpy(),
           "ls.w": ls.weight.grad.numpy(), "ls.b": ls.bias.grad.numpy()}
    for i, l in enumerate(lin):
        out[f"a.w{i}"], out[f"a.b{i}"] = l.weight.grad.numpy(), l.bias.grad.numpy()
    return out


# ----------------------------------------------------------------------------------------------------------- 1. autograd
@pytest.mark.parametrize("B", [1, 17, 100])
def test_restatement_equals_float64_autograd(rows, B):
    """Default modules only: on the stress set std reaches exp(-20), and the pair of the Normal log-prob that autograd
    leaves uncancelled (eps / std ~ 1e9 each) costs float64 autograd itself 1e-7 of d_mu -- the closed form has no such term."""
    m = T.sac_modules()
    obs, eps = A.batch(B, rows)
    ref, _ = A.actor_grad(m, obs, eps, log_ent_coef=LEC)
    want = _torch_f64(m, obs, eps, LEC)
    for k, v in want.items():
        r = ref[k][0]
        scale = max(float(np.abs(r).max()), float(np.abs(v).max()), 1e-30)
        diff = float(np.abs(v.reshape(r.shape) - r).max())
        assert diff <= 1e-9 * scale, (k, diff, scale)


# ----------------------------------------------------------------------------------------------------------- 2. admits fp32
@pytest.mark.parametrize("B", [17, 100, 256])
def test_bound_admits_a_pairwise_fp32_evaluation(rows, B):
    m = T.sac_modules()
    obs, eps = A.batch(B, rows)
    got = A.actor_grad_f32(m, obs, eps, log_ent_coef=LEC)
    ref, info = A.actor_grad(m, obs, eps, log_ent_coef=LEC, other=got)
    A.assert_conditions(info, f"B={B}")
    A.assert_choices(info, got, f"B={B}")
    worst = {}
    A.assert_all_within(got, ref, f"B={B} fp32", worst)
    assert set(worst) == set(ref) and max(worst.values()) > 0.0          # not a comparison of the reference with itself
    # a fixed coefficient: no ent_coef outputs
    got = A.actor_grad_f32(m, obs, eps, ent_coef=0.2)
    ref, info = A.actor_grad(m, obs, eps, ent_coef=0.2, other=got)
    assert "ent.grad" not in ref and "ent_coef_loss" not in ref
    A.assert_all_within(got, ref, f"B={B} fp32 fixed ent_coef")


# ----------------------------------------------------------------------------------------------------------- 3. rejects mistakes
@pytest.mark.parametrize("mutant", A.MUTANTS)
def test_bound_rejects_mistakes(rows, mutant):
    B = 17 if mutant == "tail_rows" else 100
    m = T.sac_modules(stress=mutant in A.STRESS_MUTANTS)
    obs, eps = A.batch(B, rows)
    ref, _ = A.actor_grad(m, obs, eps, log_ent_coef=LEC)
    bad, _ = A.actor_grad(m, obs, eps, log_ent_coef=LEC, mutant=mutant)
    out = A.outside({k: v[0] for k, v in bad.items()}, ref)
    assert out, f"the bound admits the mutant {mutant}"
    assert not A.outside({k: v[0] for k, v in ref.items()}, ref)


# ----------------------------------------------------------------------------------------------------------- 4. the conditions
@pytest.mark.parametrize("stress", [False, True], ids=["default", "stress"])
def test_conditions_of_the_gpu_cases(rows, stress):
    m = T.sac_modules(stress=stress)
    for B in GPU_BS:
        if stress and B > STRESS_MAX_B:
            continue
        obs, eps = A.batch(B, rows)
        ref, info = A.actor_grad(m, obs, eps, log_ent_coef=LEC)
        print(f"{'stress' if stress else 'default'} B={B}: {A.describe(info)}")
        A.assert_conditions(info, f"B={B}", stress=stress)
        if stress:
            assert (ref["d_log_std"][0][:, [0, 2]] == 0).all() and (ref["d_log_std"][1][:, [0, 2]] == 0).all()
            assert float(np.abs(ref["actions_pi"][0]).max()) > 0.999          # tanh saturates


def test_eager_pair_allowance_is_small_on_the_default_modules(rows):
    """std in [0.9, 1.3] there: the allowance for eager's uncancelled eps^2 pair stays a few u of alpha / B per unit eps."""
    m = T.sac_modules()
    obs, eps = A.batch(256, rows)
    _, info = A.actor_grad(m, obs, eps, log_ent_coef=LEC)
    std = info["std"][0]
    assert 0.9 <= std.min() and std.max() <= 1.3
    a_mu, a_ls = A.eager_pair_allowance(info, eps)
    ae = np.abs(eps.astype(np.float64))
    k = A.EAGER_PAIR_ROUNDINGS * R.U * info["alpha"][0] / 256
    # with std >= 0.9 and |mu| <= 1 here: (|mu| + std |eps|) / std <= 1.2 + |eps|
    assert a_mu.shape == (256, 3) and (a_mu >= 0).all() and (a_ls <= 1.01 * k * (1.2 + ae) * ae + 1e-300).all()


# ----------------------------------------------------------------------------------------------------------- 5. ActorGradSpec
class FlattenExtractor(torch.nn.Module):
    pass


class NatureCNN(torch.nn.Module):
    pass


def _q(Hq=128, nl=3):
    dims = [21] + [Hq] * nl
    mods = [x for i in range(nl) for x in (torch.nn.Linear(dims[i], dims[i + 1]), torch.nn.ReLU())]
    return torch.nn.Sequential(*mods, torch.nn.Linear(Hq, 1))


def _critic(Hq=128, nl=3, n=2):
    return types.SimpleNamespace(q_networks=[_q(Hq, nl) for _ in range(n)], n_critics=n, features_extractor=FlattenExtractor(),
                                 share_features_extractor=False)


def _sac_model(Ha=128, nl=3, act=torch.nn.ReLU, learned=True, **kw):
    dims = [18] + [Ha] * nl
    latent = torch.nn.Sequential(*[x for i in range(nl) for x in (torch.nn.Linear(dims[i], dims[i + 1]), act())])
    actor = types.SimpleNamespace(latent_pi=latent, mu=torch.nn.Linear(Ha, 3), log_std=torch.nn.Linear(Ha, 3), use_sde=False,
                                  features_extractor=FlattenExtractor())
    critic = _critic(**kw)
    m = types.SimpleNamespace(actor=actor, critic=critic, critic_target=copy.deepcopy(critic), gamma=0.99, log_ent_coef=None,
                              ent_coef_tensor=None, target_entropy=-3.0)
    if learned:
        m.log_ent_coef = torch.log(torch.ones(1) * 1.0).requires_grad_(True)
    else:
        m.ent_coef_tensor = torch.tensor(0.1)
    return m


def _td3_model(n_critics=2):
    mods = [torch.nn.Linear(18, 256), torch.nn.ReLU(), torch.nn.Linear(256, 256), torch.nn.ReLU()]
    actor = types.SimpleNamespace(mu=torch.nn.Sequential(*mods, torch.nn.Linear(256, 3), torch.nn.Tanh()),
                                  features_extractor=FlattenExtractor())
    critic = _critic(256, 2, n_critics)
    return types.SimpleNamespace(actor_target=actor, actor=actor, critic=critic, critic_target=copy.deepcopy(critic), gamma=0.98)


def test_spec_accepts_an_sb3_shaped_model_and_lays_out_the_buffer():
    from reinforcementlearning4meshgeneration_amd.actor_grad import ActorGradSpec
    m = _sac_model()
    s = ActorGradSpec.from_sb3(m)
    assert len(s.actor) == 10 and len(s.q1) == 8 and len(s.q2) == 8 and s.log_ent_coef is m.log_ent_coef
    assert s.actor[0] is m.actor.latent_pi[0].weight and s.actor[6] is m.actor.mu.weight and s.actor[9] is m.actor.log_std.bias
    assert s.q1[0] is m.critic.q_networks[0][0].weight and s.q2[7] is m.critic.q_networks[1][6].bias     # the LIVE critics
    assert s.q1[0] is not m.critic_target.q_networks[0][0].weight and s.target_entropy == -3.0
    off = [at for _, at in s.offsets()]
    assert len(off) == 11 and off[:3] == [0, 128 * 18, 128 * 18 + 128]
    assert off[6:] == [35456, 35840, 35843, 36227, 36230] and s.ent_offset == 36230 and s.n_grad == 36288
    assert s.offsets()[10][0] is m.log_ent_coef
    s = ActorGradSpec.from_sb3(_sac_model(learned=False))
    assert s.log_ent_coef is None and abs(s.ent_coef - 0.1) < 1e-7 and len(s.offsets()) == 10 and s.n_grad == 36288
    t = T.sac_modules()
    s = ActorGradSpec.sac(t["lin"], t["mu"], t["ls"], t["q1"], t["q2"], ent_coef=0.2, target_entropy=-2.5)
    assert s.actor[0] is t["lin"][0].weight and s.target_entropy == -2.5


def _refused(model, *words):
    from reinforcementlearning4meshgeneration_amd.actor_grad import ActorGradSpec
    with pytest.raises(ValueError) as e:
        ActorGradSpec.from_sb3(model)
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def test_spec_refusals_name_what_was_found():
    from reinforcementlearning4meshgeneration_amd.actor_grad import ActorGradSpec, FusedActorGrad
    _refused(_td3_model(), "not yet: SAC only")
    _refused(_td3_model(n_critics=1), "not yet: SAC only")                 # DDPG
    _refused(_sac_model(Ha=256, nl=2), "[256, 256]")                       # other widths
    _refused(_sac_model(Ha=128, nl=2), "[128, 128]")
    _refused(_sac_model(Hq=256, nl=3), "[256, 256, 256]")
    _refused(_sac_model(act=torch.nn.Tanh), "tanh")
    _refused(_sac_model(n=3), "n_critics = 3")
    _refused(_sac_model(n=1), "n_critics = 1")
    m = _sac_model(); m.actor.features_extractor = NatureCNN(); _refused(m, "NatureCNN", "actor.features_extractor")
    m = _sac_model(); m.critic.features_extractor = NatureCNN(); m.critic.share_features_extractor = True
    _refused(m, "NatureCNN", "share_features_extractor")
    m = _sac_model(); m.actor.use_sde = True; _refused(m, "use_sde")
    _refused(types.SimpleNamespace(policy=None), "actor.latent_pi")
    m = _sac_model(); del m.critic; _refused(m, "critic.q_networks")
    m = _sac_model(); m.target_entropy = "auto"; _refused(m, "target_entropy")
    m = _sac_model(); m.actor.mu = m.actor.mu.double(); _refused(m, "float64")
    m = _sac_model(); m.actor.latent_pi[2].weight = torch.nn.Parameter(torch.zeros(128, 256)[:, ::2]); _refused(m, "not contiguous")
    m = _sac_model(); m.critic.q_networks[1] = m.critic.q_networks[1].double(); _refused(m, "float64")
    m = _sac_model(); m.actor.mu.weight = torch.nn.Parameter(torch.zeros(3, 64)); _refused(m, "(3, 64)")
    t = T.sac_modules()
    with pytest.raises(ValueError, match="exactly one"):
        ActorGradSpec.sac(t["lin"], t["mu"], t["ls"], t["q1"], t["q2"])
    with pytest.raises(ValueError, match="exactly one"):
        ActorGradSpec.sac(t["lin"], t["mu"], t["ls"], t["q1"], t["q2"], log_ent_coef=torch.zeros(1), ent_coef=0.1)
    with pytest.raises(ValueError, match="one element"):
        ActorGradSpec.sac(t["lin"], t["mu"], t["ls"], t["q1"], t["q2"], log_ent_coef=torch.zeros(2))
    with pytest.raises(ValueError, match="target_entropy"):
        ActorGradSpec.sac(t["lin"], t["mu"], t["ls"], t["q1"], t["q2"], ent_coef=0.1, target_entropy=float("nan"))
    spec = ActorGradSpec.from_sb3(_sac_model())
    with pytest.raises(ValueError, match="is on cpu"):
        spec.check_device(torch.device("cuda", 0))
    if not torch.cuda.is_available():
        from reinforcementlearning4meshgeneration_amd import _capi
        with pytest.raises(_capi.MeshEnvError):      # no CPU fallback
            FusedActorGrad(spec)


def test_exported_lazily_and_declared():
    import reinforcementlearning4meshgeneration_amd as pkg
    from reinforcementlearning4meshgeneration_amd import _capi
    assert pkg.FusedActorGrad.__name__ == "FusedActorGrad" and pkg.ActorGradSpec.__name__ == "ActorGradSpec"
    assert "FusedActorGrad" in pkg.__all__ and "ActorGradSpec" in pkg.__all__
    names = [n for n in _capi.EXPORTS if n.startswith("meshenv_actor_grad_")]
    assert sorted(names) == sorted("meshenv_actor_grad_" + s for s in ("create", "destroy", "set_stream", "last_error", "bind", "backward"))
