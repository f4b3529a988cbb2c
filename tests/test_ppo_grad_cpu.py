"""Host only: the fp64 restatement of the PPO / A2C loss kernels (tests/ppo_grad_ref.py) against torch float64 autograd of
SB3's statement; its bound against a pairwise numpy fp32 evaluation, against eager fp32 torch and against named mistakes; the
conditions of every case the GPU test uses; PPOGradSpec and the ActorCriticPolicy recogniser on SB3-shaped stub models; the
exports of the header of its own."""
import copy
import os
import re
import types

import numpy as np
import pytest
import torch

import policy_ref as R
import ppo_grad_ref as P
from reinforcementlearning4meshgeneration_amd import ppo_grad as _feature   # noqa: F401  every test here needs the feature

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_cache = {}


@pytest.fixture(scope="module")
def rows():
    return R.input_rows()


def _hp(m, **kw):
    kw.setdefault("max_grad_norm", P.MAX_GRAD_NORM)
    return P.hyper(clip_range=None if m["a2c"] else 0.2, **kw)


def _case(case, stress, B, rows, **kw):
    """(modules, batch, hyper, fp32 evaluation, reference, info), computed once per case."""
    key = (case, stress, B, tuple(sorted(kw.items())))
    if key not in _cache:
        m = P.modules(case, stress)
        data, hp = P.batch(m, B, rows), _hp(m, **kw)
        got = P.ppo_grad_f32(m, data, hp)
        ref, info = P.ppo_grad(m, data, hp, other=got)
        _cache[key] = (m, data, hp, got, ref, info)
    return _cache[key]


def _double(m):
    d = {k: v for k, v in m.items() if k in ("act", "H", "a2c")}
    d.update(pi=[copy.deepcopy(l).double() for l in m["pi"]], vf=[copy.deepcopy(l).double() for l in m["vf"]],
             action_net=copy.deepcopy(m["action_net"]).double(), value_net=copy.deepcopy(m["value_net"]).double(),
             log_std=torch.nn.Parameter(m["log_std"].detach().double()))
    return d


# ----------------------------------------------------------------------------------------------------------- 1. autograd
@pytest.mark.parametrize("B", [1, 17, 100])
@pytest.mark.parametrize("case", P.BOTH_SETS)
def test_restatement_equals_float64_autograd(rows, case, B):
    m = P.modules(case)
    data, hp = P.batch(m, B, rows), _hp(m)
    ref, _ = P.ppo_grad(m, data, hp)
    want = P.eager(torch, _double(m), data, hp, dtype=torch.float64)
    for k in (*P.SCALARS, *P.PARTS, *P.GRADS):
        r, v = np.asarray(ref[k][0]), want[k].numpy()
        scale = max(float(np.abs(r).max()), float(np.abs(v).max()), 1e-30)
        diff = float(np.abs(v.reshape(r.shape) - r).max())
        assert diff <= 1e-9 * scale, (k, diff, scale)


# ----------------------------------------------------------------------------------------------------------- 2. admits fp32
@pytest.mark.parametrize("case,stress", [(c, s) for c in P.CASES for s in (False, True) if not s or c in P.BOTH_SETS])
def test_bound_admits_fp32_evaluations_and_the_conditions_hold(rows, case, stress):
    """At every B of the GPU test: the conditions from the reference alone, then the pairwise numpy evaluation and eager fp32
    torch on the CPU inside the bound."""
    for B in P.GPU_BS:
        what = f"{case} {'stress' if stress else 'default'} B={B}"
        m, data, hp, got, ref, info = _case(case, stress, B, rows)
        print(f"{what}: {P.describe(info)}")
        P.assert_conditions(info, what)
        P.assert_choices(info, got, what)
        worst = {}
        P.assert_all_within(P.with_acts(got), ref, f"{what} numpy fp32", worst)
        assert set(worst) == set(ref) and set(P.ACTS) <= set(worst)         # the kept activations of both towers included
        assert max(worst.values()) > 0.0                                    # not a comparison of the reference with itself
        if B <= 256:
            e = P.eager(torch, m, data, hp)
            P.assert_all_within(e, ref, f"{what} eager fp32", names=(*P.SCALARS, *P.PARTS, *P.GRADS))


def test_conditions_hold_on_the_clip_launch_and_eager_cases(rows):
    """The further inputs of tests/test_gpu_ppo_grad.py: max_grad_norm firmly above and below the norm, and eager's sizes."""
    for mgn in (50.0, 0.02):
        for case in P.BOTH_SETS:
            _, _, _, got, ref, info = _case(case, False, 256, rows, max_grad_norm=mgn)
            P.assert_conditions(info, f"{case} max_grad_norm={mgn}")
            assert (info["total_norm"] + info["total_norm_bound"] < mgn) if mgn > 1 else (info["total_norm"] - info["total_norm_bound"] > mgn)
            P.assert_all_within(P.with_acts(got), ref, f"{case} max_grad_norm={mgn}")
    for B in (64,):
        for case in P.BOTH_SETS:
            P.assert_conditions(_case(case, False, B, rows)[5], f"{case} B={B}")


# ----------------------------------------------------------------------------------------------------------- 3. rejects mistakes
# mutant -> (case, B, keywords of hyper(), adv_scale).  Every mutant is tried on both weight sets and must leave the bound on
# at least one; the comments say which shows it and why.
MUTANT_CASES = {
    "clamp_ignored": ("ppo-relu128", 100, {}, 1.0),            # both: a fifth of the rows sit on a clipped-and-zeroed edge
    "clip_regardless_of_sign": ("ppo-relu128", 100, {}, 1.0),  # both: rows outside the range whose unclamped product is smaller
    "tie_half": ("ppo-relu128", 100, {}, 1.0),                 # both: every row inside [lo, hi] loses half its gradient
    "biased_std": ("ppo-relu128", 17, {}, 1.0),                # both, at B = 17: sqrt(17 / 16) = 1.03 on every advantage
    "eps_inside_root": ("ppo-relu128", 100, {}, 1e-6),         # both, with advantages of 1e-6: sqrt(var + 1e-8) is 1e-4, not 1e-6
    "normalised_at_b1": ("ppo-relu128", 1, {}, 1.0),           # both: the lone advantage becomes 0
    "old_new_swapped": ("ppo-relu128", 100, {}, 1.0),          # both: ratio becomes its reciprocal
    "dls_minus_one_dropped": ("ppo-relu128", 100, {}, 1.0),    # both: log_std's gradient loses sum c
    "entropy_sign": ("ppo-relu128", 100, {"ent_coef": 0.05}, 1.0),       # both: log_std's gradient and the loss move by 2 ent_coef
    "vf_coef_dropped": ("ppo-relu128", 100, {}, 1.0),          # both: the vf tower's gradients double
    "mse_factor_2_dropped": ("ppo-relu128", 100, {}, 1.0),     # both: they halve
    "per_tensor_clip": ("ppo-relu128", 100, {"max_grad_norm": 0.02}, 1.0),   # both: every tensor scaled by its own norm
    "coef_not_clamped": ("ppo-relu128", 100, {"max_grad_norm": 50.0}, 1.0),  # both: gradients grow by max_grad_norm / norm
}


@pytest.mark.parametrize("mutant", P.MUTANTS)
def test_bound_rejects_mistakes(rows, mutant):
    case, B, kw, scale = MUTANT_CASES[mutant]
    caught = []
    for stress in (False, True):
        m = P.modules(case, stress)
        data, hp = P.batch(m, B, rows, adv_scale=scale), _hp(m, **kw)
        ref, info = P.ppo_grad(m, data, hp)
        bad, _ = P.ppo_grad(m, data, hp, mutant=mutant)
        assert not P.outside({k: v[0] for k, v in ref.items()}, ref)
        if scale != 1.0:                                                    # the bound is still one an fp32 evaluation meets
            P.assert_all_within(P.with_acts(P.ppo_grad_f32(m, data, hp)), P.ppo_grad(m, data, hp, other=P.ppo_grad_f32(m, data, hp))[0], mutant)
        caught.append(bool(P.outside({k: v[0] for k, v in bad.items()}, ref)))
    assert any(caught), f"the bound admits the mutant {mutant} on both weight sets"
    assert set(MUTANT_CASES) == set(P.MUTANTS)


# ----------------------------------------------------------------------------------------------------------- 4. the recogniser
class FlattenExtractor(torch.nn.Module):
    pass


class NatureCNN(torch.nn.Module):
    pass


def _policy(H=128, act=torch.nn.ReLU, Hv=None, act_v=None, **kw):
    Hv, act_v = Hv or H, act_v or act
    seq = lambda h, a: torch.nn.Sequential(torch.nn.Linear(18, h), a(), torch.nn.Linear(h, h), a())   # noqa: E731
    fe = FlattenExtractor()
    p = types.SimpleNamespace(mlp_extractor=types.SimpleNamespace(policy_net=seq(H, act), value_net=seq(Hv, act_v)),
                              action_net=torch.nn.Linear(H, 3), value_net=torch.nn.Linear(Hv, 1),
                              log_std=torch.nn.Parameter(torch.zeros(3)), use_sde=False, squash_output=False,
                              features_extractor=fe, pi_features_extractor=fe, vf_features_extractor=fe,
                              share_features_extractor=True)
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _model(policy=None, **kw):
    return types.SimpleNamespace(policy=policy or _policy(), clip_range_vf=None, **kw)


def _refused(model, *words):
    from reinforcementlearning4meshgeneration_amd.ppo_grad import PPOGradSpec
    with pytest.raises(ValueError) as e:
        PPOGradSpec.from_sb3(model)
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def test_spec_accepts_ppo_and_a2c_and_lays_out_the_buffer():
    from reinforcementlearning4meshgeneration_amd import _capi
    from reinforcementlearning4meshgeneration_amd.ppo_grad import PPOGradSpec
    for H, act, name in ((128, torch.nn.ReLU, "relu"), (64, torch.nn.Tanh, "tanh")):
        pol = _policy(H, act)
        for model in (_model(pol), pol):                                    # an algorithm object, and the policy itself
            s = PPOGradSpec.from_sb3(model)
            assert (s.hidden, s.activation, len(s.params)) == (H, name, 13)
            assert s.params[0] is pol.mlp_extractor.policy_net[0].weight and s.params[4] is pol.action_net.weight
            assert s.params[6] is pol.mlp_extractor.value_net[0].weight and s.params[11] is pol.value_net.bias and s.params[12] is pol.log_std
            assert s.n_grad == _capi.PPO_GRAD_FLOATS[H] and [p for p, _ in s.offsets()] == s.params
    assert [at for _, at in s.offsets()] == [0, 1152, 1216, 5312, 5376, 5568, 5571, 6723, 6787, 10883, 10947, 11011, 11012]
    m = P.modules("ppo-relu128")
    s = PPOGradSpec.actor_critic(m["pi"], m["vf"], m["action_net"], m["value_net"], m["log_std"], "relu")
    assert s.params == P.params(m) and s.n_grad == 38464
    header = open(os.path.join(ROOT, "include", "meshenv_ppo_grad.h")).read()
    assert "#define MESHENV_PPO_GRAD_FLOATS_64 11072" in header and "#define MESHENV_PPO_GRAD_FLOATS_128 38464" in header


def test_refuses_gsde():
    _refused(_model(_policy(use_sde=True)), "use_sde=True", "gSDE")


def test_refuses_squash_output():
    _refused(_model(_policy(squash_output=True)), "squash_output=True")


def test_refuses_a_non_flatten_features_extractor():
    _refused(_model(_policy(features_extractor=NatureCNN())), "NatureCNN", "features_extractor")


def test_refuses_unshared_differing_extractors():
    class Other(FlattenExtractor):
        pass
    Other.__name__ = "FlattenExtractor"                                      # passes the name check; still another class
    _refused(_model(_policy(share_features_extractor=False, vf_features_extractor=Other())), "share_features_extractor=False", "differing")
    from reinforcementlearning4meshgeneration_amd.ppo_grad import PPOGradSpec
    PPOGradSpec.from_sb3(_model(_policy(share_features_extractor=False, vf_features_extractor=FlattenExtractor())))   # two of the same: fine


def test_refuses_towers_of_different_width():
    _refused(_model(_policy(128, Hv=64)), "pi width 128 and vf width 64 differ")


def test_refuses_mixed_activations():
    _refused(_model(_policy(act_v=torch.nn.Tanh)), "mixed activations ['relu', 'tanh']")


def test_refuses_width_256_and_other_widths():
    _refused(_model(_policy(256)), "width 256 is not supported", "column split")
    _refused(_model(_policy(96)), "hidden width 96")


def test_refuses_a_clipped_value_loss():
    m = _model()
    m.clip_range_vf = 0.2
    _refused(m, "clip_range_vf = 0.2", "must be None")


def test_refuses_what_is_not_an_actor_critic_policy_or_not_bindable():
    _refused(types.SimpleNamespace(actor=None), "no mlp_extractor")
    p = _policy(); p.action_net = p.action_net.double(); _refused(_model(p), "action_net.weight", "float64")
    p = _policy(); p.log_std = torch.nn.Parameter(torch.zeros(3, 3)); _refused(_model(p), "log_std", "(3, 3)")
    p = _policy(); p.mlp_extractor.policy_net[2].weight = torch.nn.Parameter(torch.zeros(128, 256)[:, ::2]); _refused(_model(p), "not contiguous")
    p = _policy(); p.mlp_extractor.policy_net = torch.nn.Sequential(torch.nn.Linear(18, 128), torch.nn.ReLU()); _refused(_model(p), "pi tower")
    p = _policy(act=torch.nn.ELU); _refused(_model(p), "activation 'elu'")


def test_no_cpu_fallback_and_device_check():
    from reinforcementlearning4meshgeneration_amd import _capi
    from reinforcementlearning4meshgeneration_amd.ppo_grad import FusedPPOGrad, PPOGradSpec
    spec = PPOGradSpec.from_sb3(_model())
    with pytest.raises(ValueError, match="is on cpu"):
        spec.check_device(torch.device("cuda", 0))
    if not torch.cuda.is_available():
        with pytest.raises(_capi.MeshEnvError):
            FusedPPOGrad(spec)


# ----------------------------------------------------------------------------------------------------------- 5. packaging
def test_exported_lazily_declared_and_built():
    import reinforcementlearning4meshgeneration_amd as pkg
    from reinforcementlearning4meshgeneration_amd import _capi
    assert pkg.FusedPPOGrad.__name__ == "FusedPPOGrad" and pkg.PPOGradSpec.__name__ == "PPOGradSpec"
    assert "FusedPPOGrad" in pkg.__all__ and "PPOGradSpec" in pkg.__all__ and hasattr(pkg.FusedPolicy, "bind_live") and hasattr(pkg.FusedPolicy, "refresh")
    names = _capi.EXPORTS_PPO_GRAD
    want = ["meshenv_ppo_grad_" + s for s in ("create", "destroy", "set_stream", "last_error", "bind", "backward")] + \
           ["meshenv_policy_bind", "meshenv_policy_refresh"]
    assert sorted(names) == sorted(want) and len(names) == 8
    L = _capi.load()
    assert L.meshenv_ppo_grad_bind(None, 128, 0, None, 13, None, 38464) == _capi.E_ARG and L.meshenv_policy_refresh(None) == _capi.E_ARG
