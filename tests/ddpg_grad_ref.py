"""Host-only fp64 restatements of DDPG's two gradient statements at [400, 300] (csrc/meshenv_wide_grad.h: k_wgrad_critic_rows,
k_wgrad_actor_rows, k_wgrad_weights, k_wgrad_reduce) with manual backpropagation and a per-element bound on the kernels' fp32
error, by the rules at the top of tests/policy_ref.py and built the way critic_grad_ref.py and td3_actor_grad_ref.py build
theirs.  Shared by tests/test_ddpg_grad_cpu.py and tests/test_gpu_ddpg_grad.py; nothing here touches a device.

``critic_grad(model, obs, actions, y, loss_scale)`` returns ``({name: (ref, bound)}, info)`` for ``critic_loss``, ``q1`` and the
gradients ``c.w{l}`` / ``c.b{l}`` (l = 0, 1 the hidden layers, 2 the output layer; torch's shapes) of

    critic_loss = loss_scale * 2 * mean(0.5 (Q1(cat(obs, actions)) - y)^2);  zero_grad();  critic_loss.backward()

``actor_grad(model, obs)`` likewise for ``actor_loss``, the parts ``actions_pi``, ``q1_pi``, ``dq_da``, ``d_pre``, the gradients
``a.w{l}`` / ``a.b{l}`` (l = 0, 1), ``mu.w``, ``mu.b`` of

    actor_loss = -Q1(cat(obs, tanh(mu(obs)))).mean();  zero_grad();  actor_loss.backward()

and ``c.w2`` / ``c.b2``: what the call ADDS to the critic's output-layer gradient, which is exactly nothing (ref 0, bound 0).

The chains, in the kernels' order (u = 2^-24, gamma_m = m u / (1 - m u); the header of csrc/meshenv_wide_grad.h writes the
orders down and ``FORWARD_M``, ``DA2_CHAIN``, ``DA1_CHAIN``, ``HEAD_CHAIN`` and ``reduction_roundings`` restate them):

  a_l, q, pre  policy_ref.layer with the forward's rounding counts FORWARD_M = (6, 54, 42): two accumulators over the even /
               odd 16-groups of k, their sum, the bias (the counts of meshenv_wide.h and ddpg_ref.M_LAYER); ReLU by relu_err
  a            tanhf(pre): tanh_err
  d = q - y    one rounding;  dq = (2 loss_scale) * (d / B): one rounding, the scaling is exact;  d2 = d * d
  critic_loss  loss_scale * (S / B), S the batch sum of d2: one u for the division
  dz_2         critic: mask_2 * (dq * w_out), one rounding;  actor's critic pass: mask_2 * w_out, exact
  da_1         dz_2 W_2 over 19 groups of 16 neurons, 10 in the longer accumulator: gamma_41 (DA2_CHAIN)
  dQ/da        dz_1 W_1[:, 18..20] over 25 groups, 13 in the longer accumulator: gamma_53 (DA1_CHAIN)
  d_pre        (-(dQ/da / B)) * (1 - a a): one rounding, mul, add, mul (td3_actor_grad_ref's)
  actor dz_2   mask_2 * sum_i d_pre[i] W_3[i]: one product and two fmaf, gamma_3 (HEAD_CHAIN)
  actor_loss   -(S / B), S the batch sum of q

Batch sums (dW, db, S): one accumulator per chunk of T = max(4, ceil(tiles / 64)) row tiles (tiles = ceil(B / 16)), one
rounding per row, at most min(16 T, 16 tiles); then the chunks' partial sums added in index order, chunks - 1 additions:
m = reduction_roundings(B) (B = 1..16: 16; 100: 65; 256: 67; 4096: 127; 4101: 131; 65 536: 1087), |fl(sum) - sum| <= gamma_m
sum |terms| with |terms| at |x| + e_x.  Rows past B contribute exactly 0.

ReLU masks: an AMBIGUOUS (sample, neuron) pair (|z_ref| <= e_z) takes the mask of the evaluation the reference is compared
with, as in the siblings; the shares are capped from the reference alone, before any comparison, at the siblings' caps.
"""
from __future__ import annotations

import numpy as np

import ddpg_ref as D
import policy_ref as R
import td_target_ref as T
from actor_grad_ref import _add, _host, _mul, _sum
from critic_grad_ref import _bsum, _bsum32, batch  # noqa: F401  (batch: the inputs)
from policy_ref import U, _f64, gamma, relu_err, tanh_err

FORWARD_M = (6, 54, 42)              # roundings on the longest path: layer 1, layer 2, head
DA2_CHAIN = 41                       # da_1 = dz_2 W_2: 19 groups, 10 of them (40 fma) in acc0, then acc0 + acc1
DA1_CHAIN = 53                       # dQ/da = dz_1 W_1: 25 groups, 13 of them (52 fma) in acc0, then acc0 + acc1
HEAD_CHAIN = 3                       # dz_2 of the actor: one product and two fmaf
CHUNK_MIN_TILES, MAX_CHUNKS = 4, 64
MAX_ROWS = 65536
LOSS_SCALES = (1.0, 0.5)
MAX_CRITIC_STATEMENT_SHARE = 2e-4    # critic_grad_ref.MAX_AMBIGUOUS_SHARE
MAX_ACTOR_SHARE = 2e-4               # actor_grad_ref.MAX_ACTOR_SHARE: the actor's layers in the actor statement
MAX_CRITIC_SHARE = 1.5e-3            # actor_grad_ref.MAX_CRITIC_SHARE: the critic's layers in the actor statement
STRESS_BIAS = (12.0, 0.0, -12.0)     # added to mu.bias of ddpg_model(head_scale=8.0)
# |pre| - e_pre on components 0 and 2 of the head-saturation set.  The [300]-wide head spreads pre more than the sibling's
# [256] does (its rows reach down to 8.4 where td3_actor_grad_ref's stay above 9), so the condition is stated from what it is
# for: 1 - tanh(8)^2 = 4.5e-7 lies below 8 ulp = 9.5e-7, the least the bound of a a can be (2 e_a, tanhf's 4 ulp), so fp32's
# s = 1 - a a is rounding noise there and jacobian_from_pre (1 - 64 = -63 in its place) cannot pass.
STRESS_MIN_PRE = 8.0
GPU_BS = (1, 15, 16, 17, 33, 100, 256, 4101)
NET_MUTANTS = ("drop_n299_layer2", "drop_k399_layer2", "drop_k299_head", "bias_next_neuron_tile18")
CRITIC_MUTANTS = ("sum_for_mean", "loss_scale_x2", "mask_from_above", "dw_transposed", "cat_action_obs", "target_sign", "tail_rows",
                  "db_zero") + NET_MUTANTS
ACTOR_MUTANTS = ("drop_tanh_jacobian", "sign_of_q", "jacobian_from_pre", "critic_grad_leak", "sum_for_mean", "cat_action_obs",
                 "mask_from_above", "tail_rows")
STRESS_MUTANTS = ("jacobian_from_pre",)      # shows only where tanh saturates (td3_actor_grad_ref.STRESS_MUTANTS)
CRITIC_GRADS = ("c.w0", "c.b0", "c.w1", "c.b1", "c.w2", "c.b2")
ACTOR_GRADS = ("a.w0", "a.b0", "a.w1", "a.b1", "mu.w", "mu.b")
PARTS = ("actions_pi", "q1_pi", "dq_da", "d_pre")
assert FORWARD_M == D.M_LAYER


def reduction_roundings(B):
    """m of the docstring: roundings on the longest path of a batch sum of k_wgrad_weights + k_wgrad_reduce."""
    tiles = (B + 15) // 16
    T_ = max(CHUNK_MIN_TILES, -(-tiles // MAX_CHUNKS))
    chunks = -(-tiles // T_)
    return min(16 * T_, 16 * tiles) + chunks - 1


# ----------------------------------------------------------------------------------------------------------- inputs
def model(stress=None, seed=47, lr=1e-3, tau=0.005):
    """ddpg_ref.ddpg_model() with torch.optim.Adam optimisers on the live actor and critic and SB3's tau.  stress: None,
    "critic_w6" / "actor_w6" (the first layer's weights x 6 of the critic / the actor: large pre-activations, many neurons
    clipped), or "head" (head_scale = 8 and (+12, 0, -12) added to mu.bias: components 0 and 2 of tanh saturate)."""
    import torch
    m = D.ddpg_model(seed=seed, head_scale=8.0 if stress == "head" else 1.0)
    with torch.no_grad():
        if stress == "head":
            m.actor.mu[-2].bias.add_(torch.tensor(STRESS_BIAS))
        elif stress == "critic_w6":
            m.critic.q_networks[0][0].weight.mul_(6.0)
        elif stress == "actor_w6":
            m.actor.mu[0].weight.mul_(6.0)
        elif stress is not None:
            raise ValueError(stress)
    attach_optimizers(m, lr, tau)
    return m


def attach_optimizers(m, lr=1e-3, tau=0.005):
    """The optimisers SB3 gives a DDPG model (Adam on the live networks) and its Polyak coefficient; after to_cuda() again."""
    import torch
    m.actor.optimizer = torch.optim.Adam(list(m.actor.mu.parameters()), lr=lr)
    m.critic.optimizer = torch.optim.Adam([p for q in m.critic.q_networks for p in q.parameters()], lr=lr)
    m.tau = tau
    return m


def live_layers(m):
    """([(W, b)] * 3 of the live actor, of the live critic), float32."""
    return D.actor_layers(m), D.critic_layers(m, target=False)


# ----------------------------------------------------------------------------------------------------------- pieces
def _layer(x, ex, W, b, i):
    return R.layer(x, ex, W, b, None, 2 * (FORWARD_M[i] - 2))


def _net_mutant(layers, mutant):
    (w1, b1), (w2, b2), (wh, bh) = layers
    if mutant == "drop_k399_layer2":
        w2 = w2.copy(); w2[:, 399] = 0.0
    elif mutant == "bias_next_neuron_tile18":      # tile 18 = neurons 288..303; the padded bias of neuron 300 is zero
        b2 = b2.copy(); b2[288:300] = np.concatenate([b2[289:300], [0.0]])
    elif mutant == "drop_k299_head":
        wh = wh.copy(); wh[:, 299] = 0.0
    return [(w1, b1), (w2, b2), (wh, bh)]


def _hidden(layers, x, ex, mutant=None):
    """[(z, ez, a, ea)] of the two ReLU layers."""
    hid, h, e = [], x, ex
    for i, (W, b) in enumerate(layers[:2]):
        z, ez = _layer(h, e, W, b, i)
        if i == 1 and mutant == "drop_n299_layer2":
            z = z.copy(); z[:, 299] = -1.0
        h, e = np.maximum(z, 0.0), relu_err(z, ez)
        hid.append((z, ez, h, e))
    return hid


def _masks(hid, other_acts):
    amb = [np.abs(z) <= ez for z, ez, _, _ in hid]
    own = [z > 0 for z, _, _, _ in hid]
    use = own if other_acts is None else [np.where(a, _host(o)[:len(a)] > 0, k) for a, k, o in zip(amb, own, other_acts)]
    return amb, own, [k.astype(np.float64) for k in use]


def _back(dz, edz, W, chain):
    """da = dz W as the kernel's two fma chains and their sum."""
    W = _f64(W)
    return dz @ W, edz @ np.abs(W) + gamma(chain) * ((np.abs(dz) + edz) @ np.abs(W))


def _share(ambs):
    return sum(int(v.sum()) for v in ambs) / sum(v.size for v in ambs)


# ----------------------------------------------------------------------------------------------------------- the critic statement
def critic_grad(m, obs, actions, y, loss_scale=1.0, other_acts=None, mutant=None):
    """m: model().  other_acts: the two post-ReLU activations [B, 400], [B, 300] of the evaluation this reference is compared
    with (its mask is taken on the ambiguous pairs), or None."""
    o, a, yy = _f64(np.asarray(obs, np.float32)), _f64(np.asarray(actions, np.float32)), _f64(np.asarray(y, np.float32)).reshape(-1)
    B = o.shape[0]
    x = np.concatenate([a, o], axis=1) if mutant == "cat_action_obs" else np.concatenate([o, a], axis=1)
    if mutant == "tail_rows":        # the rows of the last tile past B treated as samples (zero input, zero target)
        pad = (-B) % 16
        x, yy = np.concatenate([x, np.zeros((pad, 21))]), np.concatenate([yy, np.zeros(pad)])
        other_acts = None
    mm = reduction_roundings(B)
    ls = float(loss_scale) * (2.0 if mutant == "loss_scale_x2" else 1.0)
    div = 1.0 if mutant == "sum_for_mean" else float(B)
    L = _net_mutant(live_layers(m)[1], mutant)
    hid = _hidden(L, x, np.zeros_like(x), mutant)
    amb, own, mk = _masks(hid, other_acts)
    q, eq = _layer(hid[1][2], hid[1][3], *L[2], 2)
    q, eq = q[:, 0], eq[:, 0]
    d = q + yy if mutant == "target_sign" else q - yy
    e_d = eq + U * (np.abs(d) + eq)
    dq, e_dq = 2.0 * ls * d / div, 2.0 * ls * (e_d + U * (np.abs(d) + e_d)) / div
    d2 = d * d
    e_d2 = 2.0 * np.abs(d) * e_d + e_d * e_d + U * (np.abs(d) + e_d) ** 2
    S, eS = d2.sum(), e_d2.sum() + gamma(mm) * (d2 + e_d2).sum()
    out = {"critic_loss": (np.array(ls * S / div), np.array(ls * (eS / div + U * (S + eS) / div))), "q1": (q[:B], eq[:B])}
    acts = [(x, np.zeros_like(x))] + [(h, e) for _, _, h, e in hid]
    wh = _f64(L[2][0])[0]
    out["c.w2"] = _bsum(dq[:, None], e_dq[:, None], *acts[2], mm)
    out["c.b2"] = _sum(dq[:, None], e_dq[:, None], mm, axis=0)
    dz = mk[1] * (dq[:, None] * wh[None])
    edz = mk[1] * (e_dq[:, None] * np.abs(wh)[None] + U * (np.abs(dq) + e_dq)[:, None] * np.abs(wh)[None])
    for l in (1, 0):
        w, ew = _bsum(dz, edz, *acts[l], mm)
        if mutant == "dw_transposed" and l == 1:       # written [in][out] into the [out][in] tensor
            w = np.ascontiguousarray(w.T).reshape(w.shape)
        out[f"c.w{l}"] = (w, ew)
        out[f"c.b{l}"] = _sum(dz, edz, mm, axis=0)
        if l == 0:
            break
        da, eda = _back(dz, edz, L[1][0], DA2_CHAIN)
        k = mk[0]
        if mutant == "mask_from_above":                # layer 2's mask where layer 1's belongs (its first 300 neurons)
            k = np.concatenate([mk[1], np.ones((len(da), 100))], axis=1)
        dz, edz = k * da, k * eda
    if mutant == "db_zero":
        for name in ("c.b0", "c.b1", "c.b2"):
            out[name] = (np.zeros_like(out[name][0]), out[name][1])
    info = dict(ambiguous=amb, mask=own, share=_share(amb), B=B)
    return out, info


def assert_critic_conditions(info, what):
    """The condition on the test case: stated from the reference alone, before any comparison."""
    assert info["share"] <= MAX_CRITIC_STATEMENT_SHARE, f"{what}: ReLU ambiguous share {info['share']:.2e} > {MAX_CRITIC_STATEMENT_SHARE}"


def assert_masks(ambs, masks, acts, what):
    """Off the ambiguous pairs the compared evaluation's ReLU masks equal the reference's."""
    for l, (amb, mk, act) in enumerate(zip(ambs, masks, acts)):
        bad = ((_host(act) > 0) != mk) & ~amb
        assert not bad.any(), f"{what}: layer {l}: {int(bad.sum())} masks differ off the ambiguous pairs, first {tuple(np.argwhere(bad)[0])}"


# ----------------------------------------------------------------------------------------------------------- the actor statement
def actor_grad(m, obs, other=None, mutant=None):
    """m: model().  other: dict with acts, acts1 ([B, 400] and [B, 300] each) of the evaluation this reference is compared
    with, or None (the reference's own masks everywhere)."""
    obs = np.asarray(obs, np.float32)
    B = obs.shape[0]
    if mutant == "tail_rows":        # the rows of the last tile past B treated as samples (zero observation)
        obs = np.concatenate([obs, np.zeros(((-B) % 16, 18), np.float32)])
        other = None
    mm = reduction_roundings(B)
    div = 1.0 if mutant == "sum_for_mean" else float(B)
    x = _f64(obs)
    LA, Lc = live_layers(m)

    # ---- the actor
    hid_a = _hidden(LA, x, np.zeros_like(x))
    amb_a, own_a, mk_a = _masks(hid_a, None if other is None else other["acts"])
    W3 = LA[2][0]
    pre, epre = _layer(hid_a[1][2], hid_a[1][3], *LA[2], 2)
    a, ea = np.tanh(pre), tanh_err(pre, epre)

    # ---- the critic: forward, q, dQ/da from dq = 1
    if mutant == "cat_action_obs":
        xin, exin, cols = np.concatenate([a, x], axis=1), np.concatenate([ea, np.zeros_like(x)], axis=1), slice(0, 3)
    else:
        xin, exin, cols = np.concatenate([x, a], axis=1), np.concatenate([np.zeros_like(x), ea], axis=1), slice(18, 21)
    hid_c = _hidden(Lc, xin, exin)
    amb_c, own_c, mk_c = _masks(hid_c, None if other is None else other["acts1"])
    qv, eq = _layer(hid_c[1][2], hid_c[1][3], *Lc[2], 2)
    qv, eq = qv[:, 0], eq[:, 0]
    dz, edz = mk_c[1] * _f64(Lc[2][0])[0][None], np.zeros_like(mk_c[1])
    da, eda = _back(dz, edz, Lc[1][0], DA2_CHAIN)
    dz, edz = mk_c[0] * da, mk_c[0] * eda
    dq = _back(dz, edz, _f64(Lc[0][0])[:, cols], DA1_CHAIN)

    # ---- the head gradient
    dla = (-dq[0] / div, (dq[1] + U * (np.abs(dq[0]) + dq[1])) / div)
    if mutant == "sign_of_q":
        dla = (-dla[0], dla[1])
    A_ = (pre, epre) if mutant == "jacobian_from_pre" else (a, ea)
    s = _add((np.ones_like(a), np.zeros_like(a)), tuple(v * k for v, k in zip(_mul(A_, A_), (-1.0, 1.0))))
    d_pre = dla if mutant == "drop_tanh_jacobian" else _mul(dla, s)
    dh, edh = d_pre

    # ---- the loss
    S = _sum(qv, eq, mm)
    sign = 1.0 if mutant == "sign_of_q" else -1.0
    out = {"actor_loss": (np.array(sign * S[0] / div), np.array(S[1] / div + U * (abs(S[0]) + S[1]) / div))}

    # ---- the actor's backward pass
    a2, ea2 = hid_a[1][2], hid_a[1][3]
    out["mu.w"] = _bsum(dh, edh, a2, ea2, mm)
    out["mu.b"] = _sum(dh, edh, mm, axis=0)
    W64 = _f64(W3)
    da, eda = dh @ W64, edh @ np.abs(W64) + gamma(HEAD_CHAIN) * ((np.abs(dh) + edh) @ np.abs(W64))
    dz, edz = mk_a[1] * da, mk_a[1] * eda
    acts = [(x, np.zeros_like(x))] + [(h, e) for _, _, h, e in hid_a]
    for l in (1, 0):
        out[f"a.w{l}"] = _bsum(dz, edz, *acts[l], mm)
        out[f"a.b{l}"] = _sum(dz, edz, mm, axis=0)
        if l == 0:
            break
        da, eda = _back(dz, edz, LA[1][0], DA2_CHAIN)
        k = mk_a[0]
        if mutant == "mask_from_above":
            k = np.concatenate([mk_a[1], np.ones((len(da), 100))], axis=1)
        dz, edz = k * da, k * eda
    cut = slice(0, B)
    out.update(actions_pi=(a[cut], ea[cut]), q1_pi=(qv[cut], eq[cut]), dq_da=(dq[0][cut], dq[1][cut]), d_pre=(dh[cut], edh[cut]))
    # what the call adds to the critic's output-layer gradient: nothing.  The mutant: what actor_loss.backward() adds in eager
    leak_w, leak_b = np.zeros((1, 300)), np.zeros(1)
    if mutant == "critic_grad_leak":
        leak_w, leak_b = -hid_c[1][2][cut].sum(axis=0)[None] / div, np.array([-B / div])
    out["c.w2"], out["c.b2"] = (leak_w, np.zeros((1, 300))), (leak_b, np.zeros(1))

    info = dict(ambiguous_actor=amb_a, mask_actor=own_a, ambiguous_critic=amb_c, mask_critic=own_c, actor_share=_share(amb_a),
                critic_share=_share(amb_c), pre=(pre[cut], epre[cut]), B=B)
    return out, info


def assert_actor_conditions(info, what, head_stress=False):
    """The conditions on the test case: stated from the reference alone, before any comparison."""
    assert info["actor_share"] <= MAX_ACTOR_SHARE, f"{what}: actor ReLU ambiguous share {info['actor_share']:.2e} > {MAX_ACTOR_SHARE}"
    assert info["critic_share"] <= MAX_CRITIC_SHARE, f"{what}: critic ReLU ambiguous share {info['critic_share']:.2e} > {MAX_CRITIC_SHARE}"
    if head_stress:
        pre, epre = info["pre"]
        firm = np.abs(pre[:, [0, 2]]) - epre[:, [0, 2]]
        assert (firm > STRESS_MIN_PRE).all(), f"{what}: tanh is not firmly saturated on components 0 and 2 (min {firm.min():.3f})"


def assert_actor_choices(info, parts, what):
    assert_masks(info["ambiguous_actor"], info["mask_actor"], parts["acts"], f"{what} actor")
    assert_masks(info["ambiguous_critic"], info["mask_critic"], parts["acts1"], f"{what} critic")


def assert_all_within(got, ref, what, worst=None):
    """Every output of ref within its bound (got: name -> array or tensor); worst: dict of the largest ratio per output."""
    for k, rb in ref.items():
        r = R.assert_within(_host(got[k]).reshape(rb[0].shape), rb, f"{what} {k}")
        if worst is not None:
            worst[k] = max(worst.get(k, 0.0), r)


def outside(got, ref):
    """Names of the outputs of got (name -> array) with an element outside ref's bound."""
    return [k for k, rb in ref.items() if k in got and R.ratio(np.asarray(got[k]).reshape(rb[0].shape), rb)[1].any()]


# ----------------------------------------------------------------------------------------------------------- fp32: numpy pairwise
def _fwd32(layers, x):
    acts, h = [], x
    for W, b in layers[:2]:
        h = np.maximum(T._dense32(h, W, b), np.float32(0))
        acts.append(h)
    return acts, T._dense32(h, *layers[2])


def _bwd32(out, prefix, layers, acts_in, dz):
    """dW_2, db_2, da_1, dz_1, dW_1, db_1 in float32 from dz_2 [B, 300]; acts_in = [x, a_1]."""
    f = np.float32
    for l in (1, 0):
        out[f"{prefix}w{l}"] = _bsum32(dz, acts_in[l])
        out[f"{prefix}b{l}"] = np.ascontiguousarray(dz.T).sum(axis=1, dtype=f)
        if l == 0:
            break
        da = T._dense32(dz, np.ascontiguousarray(layers[1][0].T), np.zeros(400, f))
        dz = np.where(acts_in[1] > 0, da, f(0)).astype(f)


def critic_grad_f32(m, obs, actions, y, loss_scale=1.0):
    """The critic statement in numpy float32, every operation rounded to fp32, sums pairwise.  Returns (name -> float32
    array, [a_1, a_2])."""
    f = np.float32
    x = np.concatenate([np.asarray(obs, f), np.asarray(actions, f)], axis=1)
    yy, B = np.asarray(y, f).reshape(-1), f(x.shape[0])
    L = live_layers(m)[1]
    acts, q = _fwd32(L, x)
    q = q[:, 0]
    d = q - yy
    dq = (f(2.0 * loss_scale) * (d / B)).astype(f)
    out = {"critic_loss": np.array(f(loss_scale) * ((d * d).sum(dtype=f) / B), f), "q1": q, "c.w2": _bsum32(dq[:, None], acts[1]),
           "c.b2": np.array([dq.sum(dtype=f)])}
    dz = np.where(acts[1] > 0, dq[:, None] * L[2][0][0][None], f(0)).astype(f)
    _bwd32(out, "c.", L, [x, acts[0]], dz)
    return out, acts


def actor_grad_f32(m, obs):
    """The actor statement in numpy float32, sums pairwise.  Returns name -> float32 array, the parts included (acts, acts1
    as lists)."""
    f = np.float32
    x = np.asarray(obs, f)
    fB = f(x.shape[0])
    LA, Lc = live_layers(m)
    acts, pre = _fwd32(LA, x)
    a = np.tanh(pre)
    ca, q = _fwd32(Lc, np.concatenate([x, a], axis=1))
    q = q[:, 0]
    dz = np.where(ca[1] > 0, Lc[2][0][0][None], f(0)).astype(f)
    da = T._dense32(dz, np.ascontiguousarray(Lc[1][0].T), np.zeros(400, f))
    dz = np.where(ca[0] > 0, da, f(0)).astype(f)
    dq = T._dense32(dz, np.ascontiguousarray(Lc[0][0][:, 18:21].T), np.zeros(3, f))
    dh = ((-(dq / fB)) * (f(1) - a * a)).astype(f)
    out = {"actor_loss": np.array(-(q.sum(dtype=f) / fB), f), "mu.w": _bsum32(dh, acts[1]),
           "mu.b": np.ascontiguousarray(dh.T).sum(axis=1, dtype=f)}
    da = T._dense32(dh, np.ascontiguousarray(LA[2][0].T), np.zeros(300, f))
    dz = np.where(acts[1] > 0, da, f(0)).astype(f)
    _bwd32(out, "a.", LA, [x, acts[0]], dz)
    out.update(actions_pi=a, q1_pi=q, dq_da=dq, d_pre=dh, acts=acts, acts1=ca)
    out["c.w2"], out["c.b2"] = np.zeros((1, 300), f), np.zeros(1, f)
    return out


# ----------------------------------------------------------------------------------------------------------- torch: the literal statements
def _torch_nets(m, dtype, device):
    import copy
    mu = copy.deepcopy(m.actor.mu).to(device=device, dtype=dtype)
    q1 = copy.deepcopy(m.critic.q_networks[0]).to(device=device, dtype=dtype)
    return mu, q1


def critic_torch(m, obs, actions, y, loss_scale=1.0, dtype=None, device="cpu"):
    """SB3's statement with autograd on copies of the modules (float64 by default).  Returns (name -> array, [a_1, a_2])."""
    import torch
    import torch.nn.functional as F
    dtype = dtype or torch.float64
    _, q1 = _torch_nets(m, dtype, device)
    t = lambda v: torch.as_tensor(np.asarray(v, np.float32)).to(device=device, dtype=dtype)   # noqa: E731
    x = torch.cat([t(obs), t(actions)], dim=1)
    a1 = q1[1](q1[0](x))
    a2 = q1[3](q1[2](a1))
    q = q1[4](a2)
    loss = loss_scale * 2 * (0.5 * F.mse_loss(q, t(y).reshape(-1, 1)))
    loss.backward()
    n = lambda v: v.detach().cpu().numpy()   # noqa: E731
    lin = [q1[0], q1[2], q1[4]]
    out = {"critic_loss": n(loss), "q1": n(q)[:, 0]}
    for i, l in enumerate(lin):
        out[f"c.w{i}"], out[f"c.b{i}"] = n(l.weight.grad), n(l.bias.grad)
    return out, [n(a1), n(a2)]


def actor_torch(m, obs, dtype=None, device="cpu"):
    """SB3's statement with autograd on copies of the modules (float64 by default); the critic's gradients, which eager
    accumulates and the kernel does not, are left out: c.w2 / c.b2 are the zeros the kernel adds."""
    import torch
    dtype = dtype or torch.float64
    mu, q1 = _torch_nets(m, dtype, device)
    x = torch.as_tensor(np.asarray(obs, np.float32)).to(device=device, dtype=dtype)
    h1 = mu[1](mu[0](x))
    h2 = mu[3](mu[2](h1))
    pre = mu[4](h2)
    pre.retain_grad()
    a = torch.tanh(pre)
    a.retain_grad()
    c1 = q1[1](q1[0](torch.cat([x, a], dim=1)))
    c2 = q1[3](q1[2](c1))
    q = q1[4](c2)
    loss = -q.mean()
    loss.backward()
    n = lambda v: v.detach().cpu().numpy()   # noqa: E731
    B = x.shape[0]
    out = {"actor_loss": n(loss), "actions_pi": n(a), "q1_pi": n(q)[:, 0], "dq_da": -n(a.grad) * B, "d_pre": n(pre.grad),
           "mu.w": n(mu[4].weight.grad), "mu.b": n(mu[4].bias.grad), "acts": [n(h1), n(h2)], "acts1": [n(c1), n(c2)],
           "c.w2": np.zeros((1, 300)), "c.b2": np.zeros(1)}
    for i, l in enumerate((mu[0], mu[2])):
        out[f"a.w{i}"], out[f"a.b{i}"] = n(l.weight.grad), n(l.bias.grad)
    return out
