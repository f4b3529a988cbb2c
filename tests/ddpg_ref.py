"""A DDPG stand-in as SB3 2.x lays the model out, and host-only fp64 restatements of the two [400, 300] kernels
(csrc/meshenv_wide.h: k_wide_policy, k_wide_target) with a per-element bound on the kernels' fp32 error, by the rules at
the top of tests/policy_ref.py.  Shared by tests/test_ddpg_cpu.py and tests/test_gpu_ddpg.py; nothing here touches a device.

The bound of a dense layer is ``gamma_m (|W| (|x| + e_x) + |b|) + |W| e_x`` (policy_ref.layer), with m the number of
roundings on the longest path of the kernel's own accumulation order, which csrc/meshenv_wide.h writes down: two
accumulators, acc0 over the even k-groups and acc1 over the odd ones, four fused MFMA steps per group, then
(acc0 + acc1) + bias.  With G groups the longer chain has ceil(G / 2) of them:

  layer 1   K_pad = 32,  G = 2    m = 4 * 1  + 1 join + 1 bias =  6
  layer 2   K_pad = 400, G = 25   m = 4 * 13 + 1      + 1      = 54
  head      K_pad = 304, G = 19   m = 4 * 10 + 1      + 1      = 42

(never more than K_pad + 2).  policy_ref.layer takes the layer's K and uses gamma(K // 2 + 2): it is called with the K that
gives the m above, 2 (m - 2).  The ULP allowances are policy_ref.ULP.

The rest of each chain is the sibling's: the deterministic kind of policy_ref.policy_forward (tanh, sigma * eps, the clamp,
the four-operation rescale) and td_target_ref.td3_target with one critic (no minimum: the bound of q is the critic's own).
"""
from __future__ import annotations

import copy
import types

import numpy as np

import policy_ref as R
import rl_stubs
import td_target_ref as T
from policy_ref import U, _f64, _np32, _rescale, tanh_err

WIDTHS = (400, 300)
M_LAYER = (6, 54, 42)              # roundings on the longest path: layer 1, layer 2, head
K_PAD = (32, 400, 304)
assert all(m <= k + 2 for m, k in zip(M_LAYER, K_PAD))
ROWS = 16                          # rows per workgroup of both kernels (kWideRows): the sizes around it are test sizes
SIGMA = 0.1
NET_MUTANTS = ("drop_n299_layer2", "drop_k399_layer2", "drop_k299_head", "swap_k_layer2", "bias_next_neuron_tile18", "tf32")
TARGET_MUTANTS = ("cat_action_obs", "box_action", "drop_not_done", "noise_clip_0.5")


# ----------------------------------------------------------------------------------------------------------- the stand-in
def _seq(n_in, widths, n_out, act, tail=()):
    """What SB3's create_mlp builds: Linear, act, ..., Linear(widths[-1], n_out), then `tail`."""
    import torch
    dims = [n_in, *widths]
    mods = [m for i in range(len(widths)) for m in (torch.nn.Linear(dims[i], dims[i + 1]), act())]
    return torch.nn.Sequential(*mods, torch.nn.Linear(widths[-1], n_out), *tail)


def ddpg_model(seed=47, head_scale=1.0, widths=WIDTHS, critic_widths=None, n_critics=1, act=None):
    """An SB3-2.x-shaped DDPG model (SimpleNamespaces, as rl_stubs.td3_model): actor / actor_target with
    mu = Sequential(Linear(18, 400), ReLU, Linear(400, 300), ReLU, Linear(300, 3), Tanh), critic / critic_target with ONE
    q_network 21 -> 400 -> 300 -> 1 and n_critics = 1; SB3's DDPG constants.  torch's default init; head_scale multiplies
    the action head (x 6: actions reach the clamps).  The other arguments build what the recogniser must refuse."""
    import torch
    act = act or torch.nn.ReLU
    critic_widths = critic_widths or widths
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        def actor():
            a = types.SimpleNamespace(mu=_seq(18, widths, 3, act, (torch.nn.Tanh(),)), features_extractor=rl_stubs._extractor())
            with torch.no_grad():
                a.mu[-2].weight.mul_(head_scale)
            return a
        critic = types.SimpleNamespace(q_networks=[_seq(21, critic_widths, 1, act) for _ in range(n_critics)], n_critics=n_critics,
                                       features_extractor=rl_stubs._extractor(), share_features_extractor=False)
        a = actor()
        return types.SimpleNamespace(actor=a, actor_target=copy.deepcopy(a), critic=critic, critic_target=copy.deepcopy(critic),
                                     gamma=0.99, target_policy_noise=0.1, target_noise_clip=0.0)


def to_cuda(model):
    for part in (model.actor, model.actor_target):
        part.mu = part.mu.cuda()
    for part in (model.critic, model.critic_target):
        part.q_networks = [q.cuda() for q in part.q_networks]
    return model


def _linears(seq):
    return [m for m in seq if type(m).__name__ == "Linear"]


def actor_layers(model, target=False):
    """[(W, b)] * 3 float32 of model.actor (or actor_target)."""
    return [(_np32(l.weight), _np32(l.bias)) for l in _linears((model.actor_target if target else model.actor).mu)]


def critic_layers(model, target=True):
    return [(_np32(l.weight), _np32(l.bias)) for l in _linears((model.critic_target if target else model.critic).q_networks[0])]


def live_tensors(model):
    """Every live parameter the two fused classes bind: the actor's, actor_target's and critic_target's."""
    out = []
    for seq in (model.actor.mu, model.actor_target.mu, model.critic_target.q_networks[0]):
        for l in _linears(seq):
            out += [l.weight, l.bias]
    return out


# ----------------------------------------------------------------------------------------------------------- the network
def _layer(x, ex, W, b, act, i, rnd=None):
    return R.layer(x, ex, W, b, act, 2 * (M_LAYER[i] - 2), rnd)


def net(x, ex, layers, mutant=None):
    """18 (or 21) -> 400 -> 300 -> n_out: fp64 head output and its bound.  mutant: one of NET_MUTANTS."""
    (w1, b1), (w2, b2), (wh, bh) = layers
    rnd = R.tf32 if mutant == "tf32" else None
    if mutant == "drop_k399_layer2":
        w2 = w2.copy(); w2[:, 399] = 0.0
    elif mutant == "swap_k_layer2":
        w2 = w2.copy(); w2[:, [1, 4]] = w2[:, [4, 1]]
    elif mutant == "bias_next_neuron_tile18":      # tile 18 = neurons 288..303; the padded bias of neuron 300 is zero
        b2 = b2.copy(); b2[288:300] = np.concatenate([b2[289:300], [0.0]])
    elif mutant == "drop_k299_head":
        wh = wh.copy(); wh[:, 299] = 0.0
    h, e = _layer(x, ex, w1, b1, "relu", 0, rnd)
    h, e = _layer(h, e, w2, b2, "relu", 1, rnd)
    if mutant == "drop_n299_layer2":
        h = h.copy(); h[:, 299] = 0.0
    return _layer(h, e, wh, bh, None, 2, rnd)


# ----------------------------------------------------------------------------------------------------------- k_wide_policy
def policy_forward(layers, obs, eps=None, sigma=SIGMA, low=R.ACTION_LOW, high=R.ACTION_HIGH, mutant=None):
    """eps None: the launch without noise.  Returns {mean, unclipped, buffer_actions, actions: (ref, bound)}."""
    x = _f64(obs)
    mean, em = net(x, np.zeros_like(x), layers, mutant)
    s, es = np.tanh(mean), tanh_err(mean, em)
    if eps is not None:
        sig, e = _f64(np.broadcast_to(np.float32(sigma), (3,))), _f64(eps)
        es = es + R.gamma(2) * (np.abs(s) + es + sig * np.abs(e))
        s = s + sig * e
    out = {"mean": (mean, em), "unclipped": (s, es)}
    s = np.clip(s, -1.0, 1.0)
    out.update(buffer_actions=(s, es), actions=_rescale(s, es, low, high))
    return out


# ----------------------------------------------------------------------------------------------------------- k_wide_target
def target(actor, critic, obs, rewards, dones, eps=None, gamma_=0.99, policy_noise=0.1, noise_clip=0.0, mutant=None):
    """SB3's TD3.train block with n_critics = 1.  Returns {target, next_actions, q1, unclipped: (ref, bound)}."""
    x = _f64(obs)
    n = x.shape[0]
    net_mutant = mutant if mutant in NET_MUTANTS else None
    mean, em = net(x, np.zeros_like(x), actor, net_mutant)
    s, es = np.tanh(mean), tanh_err(mean, em)
    ep = _f64(eps) if eps is not None else np.zeros((n, 3))
    pn, nc = float(np.float32(policy_noise)), float(np.float32(0.5 if mutant == "noise_clip_0.5" else noise_clip))
    nz = pn * ep
    enz = U * np.abs(nz)
    nz = np.clip(nz, -nc, nc)
    un = s + nz
    ea = es + enz + U * (np.abs(s) + es + np.abs(nz) + enz)
    a = np.clip(un, -1.0, 1.0)
    out = {"next_actions": (a, ea), "unclipped": (un, ea)}
    ain = a
    if mutant == "box_action":
        lo, hi = _f64(R.ACTION_LOW), _f64(R.ACTION_HIGH)
        ain = lo + 0.5 * (a + 1.0) * (hi - lo)
    if mutant == "cat_action_obs":
        xin, exin = np.concatenate([ain, x], axis=1), np.concatenate([ea, np.zeros_like(x)], axis=1)
    else:
        xin, exin = np.concatenate([x, ain], axis=1), np.concatenate([np.zeros_like(x), ea], axis=1)
    q, eq = net(xin, exin, critic, net_mutant)
    q1 = (q[:, 0], eq[:, 0])
    T._finish(out, q1, q1, None, None, rewards, dones, gamma_, mutant)     # min(q, q) = q, max(e, e) = e
    del out["q2"]
    return out


# ----------------------------------------------------------------------------------------------------------- fp32 restatements
def seq_linear(x, W, b, relu=False):
    """fp32 y = sum_k W[:, k] x[:, k] + b, products rounded and summed one k at a time (another order than the kernel's)."""
    acc = np.zeros((x.shape[0], W.shape[0]), np.float32)
    for k in range(W.shape[1]):
        acc = acc + x[:, k:k + 1] * W[None, :, k]
    acc = acc + b
    return np.maximum(acc, np.float32(0)) if relu else acc


def pair_linear(x, W, b, relu=False):
    """fp32 with numpy's pairwise summation over k (td_target_ref._dense32)."""
    y = T._dense32(x, W, b)
    return np.maximum(y, np.float32(0)) if relu else y


def net_f32(x, layers, linear):
    (w1, b1), (w2, b2), (wh, bh) = layers
    return linear(linear(linear(np.asarray(x, np.float32), w1, b1, True), w2, b2, True), wh, bh)


def policy_f32(layers, obs, eps, linear, sigma=SIGMA):
    f = np.float32
    s = np.tanh(net_f32(obs, layers, linear))
    if eps is not None:
        s = np.clip(s + f(sigma) * np.asarray(eps, f), f(-1), f(1))
    return dict(buffer_actions=s, actions=R.ACTION_LOW + f(0.5) * (s + f(1)) * (R.ACTION_HIGH - R.ACTION_LOW))


def target_f32(actor, critic, obs, rewards, dones, eps, linear, gamma_=0.99, policy_noise=0.1, noise_clip=0.0):
    f = np.float32
    x = np.asarray(obs, f)
    ep = np.asarray(eps, f) if eps is not None else np.zeros((len(x), 3), f)
    nz = np.clip(f(policy_noise) * ep, -f(noise_clip), f(noise_clip))
    a = np.clip(np.tanh(net_f32(x, actor, linear)) + nz, f(-1), f(1))
    q = net_f32(np.concatenate([x, a], axis=1), critic, linear)[:, 0]
    r, d = np.asarray(rewards, f).reshape(-1), np.asarray(dones, f).reshape(-1)
    return dict(next_actions=a, q1=q, target=r + ((f(1) - d) * f(gamma_)) * q)


OUTPUTS = ("target", "next_actions", "q1", "actions", "buffer_actions")


def assert_all_within(got, ref, what, worst=None):
    for k in OUTPUTS:
        if k in got and k in ref:
            v = got[k]
            v = v.cpu().numpy() if hasattr(v, "cpu") else v
            r = R.assert_within(np.asarray(v).reshape(ref[k][0].shape), ref[k], f"{what} {k}")
            if worst is not None:
                worst[k] = max(worst.get(k, 0.0), r)
