"""Host only: the fp64 restatements of DDPG's two gradient statements (tests/ddpg_grad_ref.py) against torch float64 autograd
of SB3's statements; their bounds against two other fp32 evaluations and against named mistakes; the conditions of every case
the GPU test uses; DDPGGradSpec on the DDPG stand-in and every refusal; the exports of the header of its own."""
import os
import re
import types

import numpy as np
import pytest
import torch

import ddpg_grad_ref as G
import ddpg_ref as D
import policy_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CRITIC_SETS = (None, "critic_w6")
ACTOR_SETS = (None, "actor_w6", "head")


@pytest.fixture(scope="module")
def rows():
    return R.input_rows()


def _close(want, ref, keys=None):
    for k in keys or ref:
        r, v = ref[k][0], np.asarray(want[k], np.float64)
        scale = max(float(np.abs(r).max()), float(np.abs(v).max()), 1e-30)
        diff = float(np.abs(v.reshape(r.shape) - r).max())
        assert diff <= 1e-9 * scale, (k, diff, scale)


# ----------------------------------------------------------------------------------------------------------- 1. autograd
@pytest.mark.parametrize("stress", CRITIC_SETS, ids=str)
@pytest.mark.parametrize("loss_scale", G.LOSS_SCALES)
@pytest.mark.parametrize("B", [1, 17, 100])
def test_critic_restatement_equals_float64_autograd(rows, B, loss_scale, stress):
    m = G.model(stress)
    obs, act, y = G.batch(B, rows)
    ref, _ = G.critic_grad(m, obs, act, y, loss_scale)
    want, _ = G.critic_torch(m, obs, act, y, loss_scale)
    assert set(want) == set(ref)
    _close(want, ref)


@pytest.mark.parametrize("stress", ACTOR_SETS, ids=str)
@pytest.mark.parametrize("B", [1, 17, 100])
def test_actor_restatement_equals_float64_autograd(rows, B, stress):
    m = G.model(stress)
    obs, _, _ = G.batch(B, rows)
    ref, _ = G.actor_grad(m, obs)
    want = G.actor_torch(m, obs)
    assert set(ref) <= set(want)
    _close(want, ref)


def test_rounding_counts_are_the_headers():
    assert G.FORWARD_M == D.M_LAYER == (6, 54, 42) and (G.DA2_CHAIN, G.DA1_CHAIN, G.HEAD_CHAIN) == (41, 53, 3)
    assert [G.reduction_roundings(B) for B in (1, 16, 17, 100, 256, 4096, 4101, 65536)] == [16, 16, 32, 65, 67, 127, 131, 1087]   # 4101: 257 tiles, T = 5, 52 chunks
    src = open(os.path.join(ROOT, "reinforcementlearning4meshgeneration_amd", "csrc", "meshenv_wide_grad.h")).read()
    for words in ("4 + 1 + 1 = 6", "52 + 1 + 1 = 54", "40 + 1 + 1 = 42", "40 + 1 = 41", "52 + 1 = 53", "then two fmaf",
                  "T = max(4, ceil(tiles / 64))", "chunks - 1 additions", "kWgMaxChunks = 64, kWgMinChunkTiles = 4"):
        assert words in src, words


# ----------------------------------------------------------------------------------------------------------- 2. admits fp32
@pytest.mark.parametrize("stress", CRITIC_SETS, ids=str)
def test_critic_bound_admits_two_other_fp32_orders(rows, stress):
    """At every B of the GPU test: the condition from the reference alone, then numpy's pairwise float32 evaluation and eager
    torch float32 on the CPU inside the bound."""
    m = G.model(stress)
    top = 0.0
    for B in G.GPU_BS:
        obs, act, y = G.batch(B, rows)
        for name, (got, acts) in (("pairwise", G.critic_grad_f32(m, obs, act, y)),
                                  ("torch32", G.critic_torch(m, obs, act, y, dtype=torch.float32))):
            what = f"critic {stress} B={B} {name}"
            ref, info = G.critic_grad(m, obs, act, y, other_acts=acts)
            G.assert_critic_conditions(info, what)
            G.assert_masks(info["ambiguous"], info["mask"], acts, what)
            worst = {}
            G.assert_all_within(got, ref, what, worst)
            assert set(worst) == set(ref) and 0.0 < max(worst.values()) < 1.0, worst
            top = max(top, info["share"])
    print(f"critic {stress}: worst ambiguous share {top:.1e}")


@pytest.mark.parametrize("stress", ACTOR_SETS, ids=str)
def test_actor_bound_admits_two_other_fp32_orders(rows, stress):
    m = G.model(stress)
    top_a = top_c = 0.0
    for B in G.GPU_BS:
        obs, _, _ = G.batch(B, rows)
        for name, got in (("pairwise", G.actor_grad_f32(m, obs)), ("torch32", G.actor_torch(m, obs, dtype=torch.float32))):
            what = f"actor {stress} B={B} {name}"
            ref, info = G.actor_grad(m, obs, other=got)
            G.assert_actor_conditions(info, what, head_stress=stress == "head")
            G.assert_actor_choices(info, got, what)
            worst = {}
            G.assert_all_within(got, ref, what, worst)
            assert set(worst) == set(ref) and 0.0 < max(worst.values()) < 1.0, worst
            top_a, top_c = max(top_a, info["actor_share"]), max(top_c, info["critic_share"])
        if stress == "head":
            a = ref["actions_pi"][0]
            # saturated (|pre| > 8: 1 - tanh^2 < 4.6e-7, inside the rounding of a a), and not
            assert (1.0 - a[:, [0, 2]] ** 2 < 4.6e-7).all() and (np.abs(a[:, 1]) < 0.9999).any()
    print(f"actor {stress}: worst ambiguous shares actor {top_a:.1e} critic {top_c:.1e}")


# ----------------------------------------------------------------------------------------------------------- 3. rejects mistakes
@pytest.mark.parametrize("mutant", G.CRITIC_MUTANTS)
def test_critic_bound_rejects_mistakes(rows, mutant):
    B = 17 if mutant == "tail_rows" else 100
    m = G.model()
    obs, act, y = G.batch(B, rows)
    ref, _ = G.critic_grad(m, obs, act, y)
    bad, _ = G.critic_grad(m, obs, act, y, mutant=mutant)
    assert G.outside({k: v[0] for k, v in bad.items()}, ref), f"the bound admits the mutant {mutant}"
    assert not G.outside({k: v[0] for k, v in ref.items()}, ref)


@pytest.mark.parametrize("mutant", G.ACTOR_MUTANTS)
def test_actor_bound_rejects_mistakes(rows, mutant):
    B = 17 if mutant == "tail_rows" else 100
    m = G.model("head" if mutant in G.STRESS_MUTANTS else None)
    obs, _, _ = G.batch(B, rows)
    ref, _ = G.actor_grad(m, obs)
    bad, _ = G.actor_grad(m, obs, mutant=mutant)
    out = G.outside({k: v[0] for k, v in bad.items()}, ref)
    assert out, f"the bound admits the mutant {mutant}"
    if mutant == "critic_grad_leak":
        assert set(out) == {"c.w2", "c.b2"}
    assert not G.outside({k: v[0] for k, v in ref.items()}, ref)


@pytest.mark.parametrize("mutant", G.NET_MUTANTS)
def test_actor_bound_rejects_the_padding_mistakes_in_the_actor_too(rows, mutant):
    """The same four mistakes in the ACTOR's layers (the critic statement's list has them in the critic's)."""
    m = G.model()
    obs, _, _ = G.batch(100, rows)
    ref, _ = G.actor_grad(m, obs)
    bad = G.model()
    with torch.no_grad():
        mu = bad.actor.mu
        if mutant == "drop_k399_layer2":
            mu[2].weight[:, 399] = 0.0
        elif mutant == "drop_n299_layer2":
            mu[2].weight[299] = 0.0
            mu[2].bias[299] = -1.0
        elif mutant == "drop_k299_head":
            mu[4].weight[:, 299] = 0.0
        else:
            mu[2].bias[288:300] = torch.cat([mu[2].bias[289:300].clone(), torch.zeros(1)])
    got, _ = G.actor_grad(bad, obs)
    assert G.outside({k: v[0] for k, v in got.items()}, ref), f"the bound admits the mutant {mutant}"


# ----------------------------------------------------------------------------------------------------------- 4. DDPGGradSpec
def _spec(model, **kw):
    from reinforcementlearning4meshgeneration_amd.ddpg_grad import DDPGGradSpec
    return DDPGGradSpec.from_sb3(model, **kw)


def test_spec_binds_the_live_tensors_and_lays_out_the_buffer():
    from reinforcementlearning4meshgeneration_amd import _capi
    from reinforcementlearning4meshgeneration_amd.ddpg_grad import DDPGGradSpec
    m = G.model()
    s = _spec(m)
    mu, q = m.actor.mu, m.critic.q_networks[0]
    assert len(s.actor) == 6 and len(s.q1) == 6 and len(s.tensors()) == 12 and s.loss_scale == 1.0
    for got, want in zip(s.actor, (mu[0].weight, mu[0].bias, mu[2].weight, mu[2].bias, mu[4].weight, mu[4].bias)):
        assert got is want
    for got, want in zip(s.q1, (q[0].weight, q[0].bias, q[2].weight, q[2].bias, q[4].weight, q[4].bias)):
        assert got is want
    assert s.actor[0] is not m.actor_target.mu[0].weight and s.q1[0] is not m.critic_target.q_networks[0][0].weight   # LIVE
    assert [at for _, at in s.actor_offsets()] == [0, 7200, 7600, 127600, 127900, 128800]
    assert [at - s.n_actor for _, at in s.critic_offsets()] == [0, 8400, 8800, 128800, 129100, 129400]
    assert [p for p, _ in s.offsets()] == s.actor + s.q1
    assert sum(p.numel() for p in s.actor) == 128803 and sum(p.numel() for p in s.q1) == 129401
    assert (s.n_actor, s.n_critic, s.n_grad) == (128832, 129408, 258240)
    assert (_capi.DDPG_GRAD_ACTOR_FLOATS, _capi.DDPG_GRAD_CRITIC_FLOATS, _capi.DDPG_GRAD_MAX_ROWS) == (s.n_actor, s.n_critic, G.MAX_ROWS)
    header = open(os.path.join(ROOT, "include", "meshenv_ddpg_grad.h")).read()
    for line in ("#define MESHENV_DDPG_GRAD_ACTOR_FLOATS 128832", "#define MESHENV_DDPG_GRAD_CRITIC_FLOATS 129408",
                 "#define MESHENV_DDPG_GRAD_MAX_ROWS 65536"):
        assert line in header, line
    s2 = DDPGGradSpec.ddpg([mu[0], mu[2]], mu[4], q, loss_scale=0.5)
    assert s2.actor[4] is mu[4].weight and s2.q1[4] is q[4].weight and s2.loss_scale == 0.5 and s2.n_grad == s.n_grad


def _refused(model, *words, **kw):
    from reinforcementlearning4meshgeneration_amd.sb3_nets import SUPPORTED
    with pytest.raises(ValueError) as e:
        _spec(model, **kw)
    for w in words + (SUPPORTED,):
        assert w in str(e.value), (w, str(e.value))


def test_spec_refusals_use_the_recognisers_words():
    import rl_stubs
    from reinforcementlearning4meshgeneration_amd import sb3_nets as N
    from reinforcementlearning4meshgeneration_amd.ddpg_grad import DDPGGradSpec, FusedDDPGGrad, check_batch
    assert "FusedDDPGGrad" in N.SUPPORTED and "[400, 300]" in N.SUPPORTED and "[256, 256]" in N.SUPPORTED
    for bad in (2.0, 0.25, 0.0, float("nan"), None, "1"):
        _refused(G.model(), "loss_scale", **dict(loss_scale=bad))
    _refused(rl_stubs.td3_model(), "not a DDPG model")                              # TD3: twin [256, 256]
    _refused(D.ddpg_model(widths=(256, 256)), "not a DDPG model")                   # other widths
    _refused(D.ddpg_model(critic_widths=(400, 400)), "not a DDPG model")
    _refused(D.ddpg_model(n_critics=2), "not a DDPG model")
    _refused(D.ddpg_model(act=torch.nn.Tanh), "tanh")                               # activations
    _refused(types.SimpleNamespace(policy=None), "not a DDPG model")
    m = D.ddpg_model(); m.actor.mu = m.actor.mu.double(); _refused(m, "float64")    # dtype
    m = D.ddpg_model(); m.critic.q_networks[0] = m.critic.q_networks[0].double(); _refused(m, "float64")
    m = D.ddpg_model(); m.actor.mu[2].weight = torch.nn.Parameter(torch.zeros(300, 800)[:, ::2]); _refused(m, "not contiguous")
    m = D.ddpg_model(); m.critic.q_networks[0][4].weight = torch.nn.Parameter(torch.zeros(2, 300)); _refused(m, "(2, 300)")
    m = D.ddpg_model(); m.actor.mu[-1] = torch.nn.Sigmoid(); _refused(m, "Sigmoid", "Tanh")
    with pytest.raises(ValueError) as e:                                             # a batch above the limit
        check_batch(G.MAX_ROWS + 1)
    assert "65537" in str(e.value) and "65536" in str(e.value) and N.SUPPORTED in str(e.value)
    assert check_batch(G.MAX_ROWS) == G.MAX_ROWS
    spec = DDPGGradSpec.from_sb3(G.model())
    with pytest.raises(ValueError, match="is on cpu"):                               # device
        spec.check_device(torch.device("cuda", 0))
    if not torch.cuda.is_available():
        from reinforcementlearning4meshgeneration_amd import _capi
        with pytest.raises(_capi.MeshEnvError):      # no CPU fallback
            FusedDDPGGrad(spec)


def test_the_other_gradient_classes_still_refuse_ddpg():
    from reinforcementlearning4meshgeneration_amd.critic_grad import CriticGradSpec
    from reinforcementlearning4meshgeneration_amd.td3_actor_grad import TD3ActorGradSpec
    for cls in (CriticGradSpec, TD3ActorGradSpec):
        with pytest.raises(ValueError):
            cls.from_sb3(G.model())


# ----------------------------------------------------------------------------------------------------------- 5. packaging
def test_exported_lazily_declared_and_built():
    import reinforcementlearning4meshgeneration_amd as pkg
    from reinforcementlearning4meshgeneration_amd import _capi
    assert pkg.FusedDDPGGrad.__name__ == "FusedDDPGGrad" and pkg.DDPGGradSpec.__name__ == "DDPGGradSpec"
    assert "FusedDDPGGrad" in pkg.__all__ and "DDPGGradSpec" in pkg.__all__
    names = _capi.EXPORTS_DDPG_GRAD
    assert sorted(names) == sorted("meshenv_ddpg_grad_" + s for s in ("create", "destroy", "set_stream", "last_error", "bind",
                                                                      "critic_backward", "actor_backward"))
