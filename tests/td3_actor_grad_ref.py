"""Host-only fp64 restatement of the TD3 / DDPG actor-loss kernel (csrc/meshenv_td3_actor_grad.h: k_td3_actor_grad,
k_td3_actor_grad_reduce) with manual backpropagation and a per-element bound on the kernel's fp32 error, by the rules at the
top of tests/policy_ref.py.  Shared by tests/test_td3_actor_grad_cpu.py and tests/test_gpu_td3_actor_grad.py; nothing here
touches a device.

``td3_actor_grad(m, obs, ...)`` returns ``({name: (ref, bound)}, info)`` for ``actor_loss``, the per-sample parts
``actions_pi``, ``q1_pi``, ``dq_da``, ``d_pre`` and the gradients ``a.w{l}`` / ``a.b{l}`` (l = 0, 1, the actor's hidden
layers), ``mu.w``, ``mu.b`` (torch's [out][in] / [out] shapes), of SB3's

    actor_loss = -critic.q1_forward(obs, actor(obs)).mean();  actor.optimizer.zero_grad();  actor_loss.backward()

The chain, in the kernel's order, each bound built from the one before (u = 2^-24, gamma_m = m u / (1 - m u); "mul" and
"add" below are one fp32 operation: the propagated input errors plus u times the largest result the kernel can form; H = 256):

  a_l         = relu(W_l a_{l-1} + b_l), l = 1, 2     policy_ref.layer: two fma chains of K / 2 terms, their sum, the bias:
                                                      gamma_{K/2+2}, K = 32 for the first layer and H after it; relu_err
  pre         = W_3 a_2 + b_3                         the same, K = H
  a           = tanhf(pre)                            td_target_ref's: the slope 1 - tanh^2 on [pre - e, pre + e], + 4 ulp
  c_l, q      = the first critic on cat(obs, a)       layers again, input error (0, e_a)
  dz_2^q      = mask^q_2 * w_out                      from dq = 1: exact
  da_1^q      = dz_2^q W^q_2                          cg_da: two accumulators, each one fma chain over the H / 2 = 128 neurons
                                                      of its eight 16-groups, then their sum: gamma_{H/2+1} = gamma_129
  dz_1^q      = mask^q_1 * da_1^q                     a select: exact
  dQ/da       = dz_1^q W^q_1[:, 18..20]               the same two chains of 128 and their sum: gamma_129
  dLa         = -(dQ/da / B)                          one rounding (the negation is exact)
  s           = 1 - a a                               mul, add
  d_pre       = dLa s                                 mul
  actor_loss  = -(S / B), S the batch sum of q        BATCH SUM; one u for the division
  dW_3        = d_pre^T a_2,  db_3 = sum_rows d_pre   BATCH SUMS
  da_2        = sum_i d_pre[i] W_3[i]                 one product and two fmaf: gamma_3
  dz_2        = mask_2 * da_2;  dW_2, db_2 (BATCH SUMS);  da_1 = dz_2 W_2 (gamma_129);  dz_1 = mask_1 * da_1;  dW_1, db_1

Batch sums: critic_grad_ref's (k_td3_actor_grad has the same nwg policy, and each of its accumulators -- the MFMA tiles of
dW_1, dW_2, db_2, the fmaf chain of dW_3, the plain adds of db_3 and of S -- takes one rounding per row):
m = reduction_roundings(B) roundings on the longest path, |fl(sum) - sum| <= gamma_m sum |terms| with |terms| taken at
|x| + e_x; rows past B contribute exactly 0.

ReLU masks.  A (sample, neuron) pair is AMBIGUOUS when |z_ref| <= e_z, in the actor and in the critic (whose input carries
the error of the action): either mask is a correct fp32 evaluation there, and the reference takes the mask of the evaluation
it is compared with (``other``: the kernel's return_parts on the GPU, the second fp32 evaluation's on the CPU).  Off them
the mask is z_ref > 0.  ``assert_conditions`` caps both shares from the reference alone, BEFORE anything is compared, at
actor_grad_ref's caps.

Where tanh saturates (the stress set: |pre| > 9 on components 0 and 2) fp32 gives a = +-1 and s = 0 exactly while
s_ref = 1 - tanh^2 ~ 1e-11: the bound of s is that of a a, about 2 e_a >= 8 ulp = 9.5e-7, which covers it, and d_pre is
bounded by |dLa| times that.
"""
from __future__ import annotations

import numpy as np

import policy_ref as R
import td_target_ref as T
from actor_grad_ref import MAX_ACTOR_SHARE, MAX_CRITIC_SHARE, _add, _host, _mul, _sum, batch  # noqa: F401  (batch: the inputs)
from critic_grad_ref import _bsum, _bsum32, reduction_roundings
from policy_ref import U, _f64, _np32, gamma, layer, relu_err, tanh_err

H = 256
BACK_CHAIN = H // 2 + 1              # cg_da: a chain of 128 fma per accumulator, then acc0 + acc1
HEAD_CHAIN = 3                       # dz_2 of the actor: one product and two fmaf
STRESS_BIAS = (12.0, 0.0, -12.0)     # added to mu.bias of td3_modules(head_scale=8.0)
STRESS_MIN_PRE = 9.0                 # |pre| - e_pre on components 0 and 2 of the stress set: 1 - tanh(9)^2 = 6e-8 < u
MUTANTS = ("drop_tanh_jacobian", "sign_of_q", "sum_for_mean", "cat_action_obs", "mask_from_above", "tail_rows", "second_critic",
           "jacobian_from_pre", "critic_mask_dropped")
# shows only where tanh saturates: on the default set |pre| is a few hundredths, and 1 - pre^2 differs from 1 - tanh(pre)^2
# by 2 pre^4 / 3, inside the bound that the layers in front of d_pre leave it
STRESS_MUTANTS = ("jacobian_from_pre",)
GRADS = ("a.w0", "a.b0", "a.w1", "a.b1", "mu.w", "mu.b")
PARTS = ("actions_pi", "q1_pi", "dq_da", "d_pre")


# ----------------------------------------------------------------------------------------------------------- inputs
def modules(stress=False):
    """td_target_ref.td3_modules(); stress: head_scale = 8 and (+12, 0, -12) added to mu.bias, so that components 0 and 2 of
    tanh saturate (1 - a^2 about 1e-11) while component 1 does not."""
    import torch
    if not stress:
        return T.td3_modules()
    m = T.td3_modules(head_scale=8.0)
    with torch.no_grad():
        m["mu"].bias.add_(torch.tensor(STRESS_BIAS))
    return m


# ----------------------------------------------------------------------------------------------------------- pieces
def _hidden(layers, x, ex):
    """[(z, ez, a, ea)] of the ReLU layers."""
    hid, h, e = [], x, ex
    for i, (W, b) in enumerate(layers):
        z, ez = layer(h, e, W, b, None, 32 if i == 0 else H)
        h, e = np.maximum(z, 0.0), relu_err(z, ez)
        hid.append((z, ez, h, e))
    return hid


def _masks(hid, other_acts):
    amb = [np.abs(z) <= ez for z, ez, _, _ in hid]
    own = [z > 0 for z, _, _, _ in hid]
    use = own if other_acts is None else [np.where(a, _host(o)[:len(a)] > 0, k) for a, k, o in zip(amb, own, other_acts)]
    return amb, own, [k.astype(np.float64) for k in use]


def _back(dz, edz, W):
    """da = dz W as the kernel's two fma chains of H / 2 terms and their sum."""
    W = _f64(W)
    return dz @ W, edz @ np.abs(W) + gamma(BACK_CHAIN) * ((np.abs(dz) + edz) @ np.abs(W))


# ----------------------------------------------------------------------------------------------------------- the restatement
def td3_actor_grad(m, obs, other=None, mutant=None):
    """m: modules().  other: dict with acts, acts1 (two [B, 256] each) of the evaluation this reference is compared with, or
    None (the reference's own masks everywhere)."""
    obs = np.asarray(obs, np.float32)
    B = obs.shape[0]
    if mutant == "tail_rows":        # the rows of the last tile past B treated as samples (zero observation)
        obs = np.concatenate([obs, np.zeros(((-B) % 16, 18), np.float32)])
        other = None
    mm = reduction_roundings(B)
    div = 1.0 if mutant == "sum_for_mean" else float(B)
    x = _f64(obs)

    # ---- the actor
    LA = T.layers_of(m["lin"])
    hid_a = _hidden(LA, x, np.zeros_like(x))
    amb_a, own_a, mk_a = _masks(hid_a, None if other is None else other["acts"])
    W3, b3 = _np32(m["mu"].weight), _np32(m["mu"].bias)
    pre, epre = layer(hid_a[1][2], hid_a[1][3], W3, b3, None, H)
    a, ea = np.tanh(pre), tanh_err(pre, epre)

    # ---- the first critic: forward, q, dQ/da from dq = 1
    if mutant == "cat_action_obs":
        xin, exin, cols = np.concatenate([a, x], axis=1), np.concatenate([ea, np.zeros_like(x)], axis=1), slice(0, 3)
    else:
        xin, exin, cols = np.concatenate([x, a], axis=1), np.concatenate([np.zeros_like(x), ea], axis=1), slice(18, 21)
    Lc = T.layers_of(m["q2" if mutant == "second_critic" else "q1"])
    hid_c = _hidden(Lc[:-1], xin, exin)
    amb_c, own_c, mk_c = _masks(hid_c, None if other is None else other["acts1"])
    qv, eq = layer(hid_c[1][2], hid_c[1][3], *Lc[-1], None, H)
    qv, eq = qv[:, 0], eq[:, 0]
    if mutant == "critic_mask_dropped":
        mk_c = [np.ones_like(k) for k in mk_c]
    dz, edz = mk_c[1] * _f64(Lc[-1][0])[0][None], np.zeros_like(mk_c[1])
    da, eda = _back(dz, edz, Lc[1][0])
    dz, edz = mk_c[0] * da, mk_c[0] * eda
    dq = _back(dz, edz, _f64(Lc[0][0])[:, cols])

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
        da, eda = _back(dz, edz, LA[l][0])
        mk = mk_a[l] if mutant == "mask_from_above" else mk_a[l - 1]
        dz, edz = mk * da, mk * eda
    cut = slice(0, B)
    out.update(actions_pi=(a[cut], ea[cut]), q1_pi=(qv[cut], eq[cut]), dq_da=(dq[0][cut], dq[1][cut]),
               d_pre=(dh[cut], edh[cut]))

    n_a, n_c = sum(int(v.sum()) for v in amb_a), sum(int(v.sum()) for v in amb_c)
    info = dict(ambiguous_actor=amb_a, mask_actor=own_a, ambiguous_critic=amb_c, mask_critic=own_c,
                actor_share=n_a / sum(v.size for v in amb_a), critic_share=n_c / sum(v.size for v in amb_c),
                pre=(pre[cut], epre[cut]), B=B)
    return out, info


def assert_conditions(info, what, stress=False):
    """The conditions on the test case: stated from the reference alone, before any comparison."""
    assert info["actor_share"] <= MAX_ACTOR_SHARE, f"{what}: actor ReLU ambiguous share {info['actor_share']:.2e} > {MAX_ACTOR_SHARE}"
    assert info["critic_share"] <= MAX_CRITIC_SHARE, f"{what}: critic ReLU ambiguous share {info['critic_share']:.2e} > {MAX_CRITIC_SHARE}"
    if stress:
        pre, epre = info["pre"]
        firm = np.abs(pre[:, [0, 2]]) - epre[:, [0, 2]]
        assert (firm > STRESS_MIN_PRE).all(), f"{what}: tanh is not firmly saturated on components 0 and 2 (min {firm.min():.3f})"


def describe(info):
    return f"ambiguous: actor {info['actor_share']:.1e} critic {info['critic_share']:.1e}"


def assert_choices(info, parts, what):
    """Off the ambiguous pairs the compared evaluation's ReLU masks equal the reference's."""
    for name, ambs, mks, acts in (("actor", info["ambiguous_actor"], info["mask_actor"], parts["acts"]),
                                  ("critic", info["ambiguous_critic"], info["mask_critic"], parts["acts1"])):
        for l, (amb, mk, act) in enumerate(zip(ambs, mks, acts)):
            bad = ((_host(act) > 0) != mk) & ~amb
            assert not bad.any(), f"{what}: {name} layer {l}: {int(bad.sum())} masks differ off the ambiguous pairs, first {tuple(np.argwhere(bad)[0])}"


def assert_all_within(got, ref, what, worst=None):
    """Every output of ref within its bound (got: name -> array or tensor); worst: dict of the largest ratio per output."""
    for k, rb in ref.items():
        r = R.assert_within(_host(got[k]).reshape(rb[0].shape), rb, f"{what} {k}")
        if worst is not None:
            worst[k] = max(worst.get(k, 0.0), r)


def outside(got, ref):
    """Names of the outputs of got (name -> array) with an element outside ref's bound."""
    return [k for k, rb in ref.items() if k in got and R.ratio(np.asarray(got[k]).reshape(rb[0].shape), rb)[1].any()]


# ----------------------------------------------------------------------------------------------------------- fp32 restatement
def td3_actor_grad_f32(m, obs):
    """The whole statement in numpy float32, every operation rounded to fp32, sums pairwise: a second fp32 evaluation that
    must sit inside the bound.  Returns name -> float32 array, the parts' names included (acts, acts1 as lists)."""
    f = np.float32
    x = np.asarray(obs, f)
    fB = f(x.shape[0])
    LA = T.layers_of(m["lin"])
    acts, h = [x], x
    for W, b in LA:
        h = np.maximum(T._dense32(h, W, b), f(0))
        acts.append(h)
    W3 = _np32(m["mu"].weight)
    a = np.tanh(T._dense32(h, W3, _np32(m["mu"].bias)))
    Lc = T.layers_of(m["q1"])
    ca, hc = [], np.concatenate([x, a], axis=1)
    for W, b in Lc[:-1]:
        hc = np.maximum(T._dense32(hc, W, b), f(0))
        ca.append(hc)
    q = T._dense32(hc, *Lc[-1])[:, 0]
    dz = np.where(ca[1] > 0, Lc[-1][0][0][None], f(0)).astype(f)
    da = T._dense32(dz, np.ascontiguousarray(Lc[1][0].T), np.zeros(H, f))
    dz = np.where(ca[0] > 0, da, f(0)).astype(f)
    dq = T._dense32(dz, np.ascontiguousarray(Lc[0][0][:, 18:21].T), np.zeros(3, f))
    dh = ((-(dq / fB)) * (f(1) - a * a)).astype(f)
    out = {"actor_loss": np.array(-(q.sum(dtype=f) / fB), f), "mu.w": _bsum32(dh, acts[2]),
           "mu.b": np.ascontiguousarray(dh.T).sum(axis=1, dtype=f)}
    da = T._dense32(dh, np.ascontiguousarray(W3.T), np.zeros(H, f))
    dz = np.where(acts[2] > 0, da, f(0)).astype(f)
    for l in (1, 0):
        out[f"a.w{l}"] = _bsum32(dz, acts[l])
        out[f"a.b{l}"] = np.ascontiguousarray(dz.T).sum(axis=1, dtype=f)
        if l == 0:
            break
        da = T._dense32(dz, np.ascontiguousarray(LA[l][0].T), np.zeros(H, f))
        dz = np.where(acts[l] > 0, da, f(0)).astype(f)
    out.update(actions_pi=a, q1_pi=q, dq_da=dq, d_pre=dh, acts=acts[1:], acts1=ca)
    return out
