"""Host-only fp64 restatement of the SAC actor / entropy-coefficient kernel (csrc/meshenv_actor_grad.h: k_actor_grad,
k_actor_grad_reduce) with manual backpropagation and a per-element bound on the kernel's fp32 error, by the rules at the top
of tests/policy_ref.py.  Shared by tests/test_actor_grad_cpu.py and tests/test_gpu_actor_grad.py; nothing here touches a
device.

``actor_grad(m, obs, eps, ...)`` returns ``({name: (ref, bound)}, info)`` for ``actor_loss``, ``ent_coef_loss``, the
per-sample parts ``actions_pi``, ``log_prob``, ``q1_pi``, ``q2_pi``, ``dq_da``, ``d_mu``, ``d_log_std`` and the gradients
``a.w{l}`` / ``a.b{l}`` (l = 0..2, the actor's hidden layers), ``mu.w``, ``mu.b``, ``ls.w``, ``ls.b`` (torch's [out][in] /
[out] shapes) and ``ent.grad`` [1], of SB3's

    actions_pi, log_prob = actor.action_log_prob(obs);  ent_coef = exp(log_ent_coef.detach())
    ent_coef_loss = -(log_ent_coef * (log_prob + target_entropy).detach()).mean()
    actor_loss = (ent_coef * log_prob - min(q1(obs, actions_pi), q2(obs, actions_pi))).mean();  actor_loss.backward()

The chain, in the kernel's order, each bound built from the one before (u = 2^-24, gamma_m = m u / (1 - m u); "mul" and
"add" below are one fp32 operation: the propagated input errors plus u times the largest result the kernel can form):

  a_l, heads  td_target_ref.sac_target: the actor, log_std clamp, std, g, a = tanhf(g), log_prob, q1, q2 with their bounds
  dz_3^c      = mask_3 * w_out                            critic c, from dq = 1: exact
  da_{l-1}^c  = dz_l W_l                                  two fma chains of H / 2 terms and their sum: gamma_{H/2+1}
  dz_{l-1}^c  = mask_{l-1} * da_{l-1}                     a select: exact
  dQ_c/da     = dz_1 W_1[:, 18..20]                       gamma_{H/2+1} again
  sel         = q1 <= q2 ? 1 : 2                          SEE BELOW; dq = dQ_sel/da, qmin = q_sel with bound max(e_q1, e_q2)
  alpha       = expf(log_ent_coef) (4 ulp) or an exact fp32 constant;  ab = alpha / B   one rounding
  s           = 1 - a a                                   mul, add
  t           = ((2 a) s) / (s + 1e-6f)                   mul (2 a is exact), add, then the quotient: the kernel's
                                                          denominator w' lies in [max(w - e_w, fl(1e-6f)), w + e_w] because
                                                          |tanhf| <= 1 keeps fl(1 - a a) >= 0 (td_target_ref's argument), so
                                                          |n'/w' - n/w| <= e_n / w_lo + |n| e_w / (w w_lo), + one rounding
  dLa         = -(dq / B)                                 one rounding
  se          = std eps                                   one rounding on std's bound
  d_mu        = ab t + dLa s                              mul, mul, add
  d_log_std   = cm * (ab (-1 + t se) + (dLa s) se)        mul, add, mul, mul, mul, add; cm = -20 <= raw <= 2 (SEE BELOW)
  term_1      = alpha log_prob - qmin;  term_2 = log_prob + target_entropy      mul, add;  add
  actor_loss  = S_1 / B;  m = S_2 / B;  ent.grad = -m;  ent_coef_loss = -(log_ent_coef m)     BATCH SUMS S_k, one u per
                                                          division and for the product
  dW_head     = d_head^T a_3,  db_head = sum_rows d_head  BATCH SUMS; d_head = (d_mu, d_log_std)
  da_3        = sum_i d_head[i] W_head[i]                 one product and five fmaf: gamma_6
  dz_3        = mask_3 * da_3;  then dW_l, db_l (BATCH SUMS), da_{l-1} (gamma_{H/2+1}), dz_{l-1} for l = 3, 2, 1 exactly as
                                                          critic_grad_ref does it

The closed form.  autograd differentiates the Normal log-prob -(g - mu)^2 / (2 std^2) - log(std) through g = mu + std eps
AND through mu and std: the two eps^2 terms (-eps^2 / std through g, +eps^2 / std through the variance) cancel, as do
-(g - mu) / std^2 and its opposite for mu, and what is left is -1 per component of log_std.  The kernel evaluates the closed
form and never forms the pair; eager fp32 autograd forms both and they cancel only to rounding, which
``eager_pair_allowance`` bounds for the comparison with eager torch: each of the two terms is
|d| |eps| / std (d = g - mu, |d| <= |mu| + std |eps| is the size of the operands of the subtraction that forms d) and is
rounded a handful of times, so their difference is at most K u (|mu| + std |eps|) |eps| / std with K = 8 (the subtraction,
the division by the variance, two products and the accumulation, on each side), times the weight alpha / B of log_prob in
the loss, for d_log_std; for d_mu the same without the factor |eps|.

Batch sums: critic_grad_ref's (k_actor_grad has the same nwg policy): m = reduction_roundings(B) roundings on the longest
path, |fl(sum) - sum| <= gamma_m sum |terms| with |terms| taken at |x| + e_x; rows past B contribute exactly 0.

Ambiguities.  Three decisions of the kernel are discontinuous, and where the reference cannot tell which way fp32 falls,
either choice is a correct fp32 evaluation: the reference then takes the choice of the evaluation it is compared with
(``other``: the kernel's return_parts on the GPU, the second fp32 evaluation's on the CPU), and ``info`` reports each set.
  1. ReLU masks: (sample, neuron) pairs with |z_ref| <= e_z, in the actor and in both critics (the critics' input carries
     the error of the action).  Off them the mask is z_ref > 0.
  2. min: rows with |q1 - q2| <= e_q1 + e_q2.  Off them critic 1 is selected where q1 <= q2.
  3. clamp: components with raw within e_raw of -20 or 2.  Off them cm = (-20 <= raw <= 2).
``assert_conditions`` caps each set from the reference alone, BEFORE anything is compared.
"""
from __future__ import annotations

import numpy as np

import policy_ref as R
import td_target_ref as T
from critic_grad_ref import _bsum, _bsum32, reduction_roundings
from policy_ref import ULP, ULP_REL, U, _f64, _np32, gamma, layer, relu_err

PHILOX_TAG = 3                       # k_actor_grad's own stream
H = 128
MAX_ACTOR_SHARE = 2e-4               # ambiguous ReLU pairs of the actor / all its pairs
MAX_CRITIC_SHARE = 1.5e-3            # of both critics
MAX_MIN_SHARE = 0.10                 # ambiguous min rows / B (at most one row when B < 10)
MIN_SELECTED_SHARE = 0.20            # each critic selected on at least this share of the unambiguous rows when B >= 100
EAGER_PAIR_ROUNDINGS = 8
# The stress set (sac_modules(stress=True)) has conditions of its own, restated from the reference for it.  Its mu head is
# scaled by 6, which widens the bound of the action wherever tanh is not saturated (max e_a 6.6e-4 against 1.3e-4 on the
# default set at B = 256), and with it the intervals of the critics' pre-activations and of q1 - q2, by at most that factor;
# the caps on those two sets are set to TWICE the default ones, well inside what the factor would allow.  The actor's cap
# stays, no clamp component may be ambiguous, and the clamps must be firmly active (components 0 and 2 beyond 2 / -20 by
# more than their bound, component 1 inside) instead of firmly inactive.
STRESS_CRITIC_SHARE = 2 * MAX_CRITIC_SHARE
STRESS_MIN_SHARE = 2 * MAX_MIN_SHARE
MUTANTS = ("max_for_min", "q1_only", "drop_entropy_term", "drop_tanh_jacobian", "drop_1e-6", "no_clamp_mask", "sum_for_mean",
           "sign_of_q", "cat_action_obs", "mu_ls_swapped", "mask_from_above", "tail_rows", "ent_grad_sign")
STRESS_MUTANTS = ("drop_1e-6", "no_clamp_mask")     # show only where tanh saturates / where a clamp is active
GRADS = ("a.w0", "a.b0", "a.w1", "a.b1", "a.w2", "a.b2", "mu.w", "mu.b", "ls.w", "ls.b")
PARTS = ("actions_pi", "log_prob", "q1_pi", "q2_pi", "dq_da", "d_mu", "d_log_std")


# ----------------------------------------------------------------------------------------------------------- inputs
def batch(B, rows, seed=31, tight=True):
    """observations [B, 18]: a prefix of ``rows`` (policy_ref.input_rows()) restricted by td_target_ref.tight_rows when
    ``tight``, repeated beyond its length; eps [B, 3] standard normal; float32."""
    rows = np.asarray(rows, np.float32)
    if tight:
        rows = rows[T.tight_rows(rows)]
    obs = np.ascontiguousarray(np.resize(rows, (B, 18)).astype(np.float32))
    eps = np.random.default_rng(seed + B).standard_normal((B, 3)).astype(np.float32)
    return obs, eps


# ----------------------------------------------------------------------------------------------------------- fp32 operations
def _mul(x, y):
    (a, ea), (b, eb) = x, y
    return a * b, np.abs(a) * eb + np.abs(b) * ea + ea * eb + U * (np.abs(a) + ea) * (np.abs(b) + eb)


def _add(x, y):
    (a, ea), (b, eb) = x, y
    return a + b, ea + eb + U * (np.abs(a + b) + ea + eb)


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
    use = own if other_acts is None else [np.where(a, np.asarray(o)[:len(a)] > 0, k) for a, k, o in zip(amb, own, other_acts)]
    return amb, own, [k.astype(np.float64) for k in use]


def _back(dz, edz, W):
    """da = dz W as the kernel's two fma chains of H / 2 terms."""
    W = _f64(W)
    return dz @ W, edz @ np.abs(W) + gamma(H // 2 + 1) * ((np.abs(dz) + edz) @ np.abs(W))


def _sum(x, ex, m, axis=None):
    return x.sum(axis=axis), ex.sum(axis=axis) + gamma(m) * (np.abs(x) + ex).sum(axis=axis)


# ----------------------------------------------------------------------------------------------------------- the restatement
def actor_grad(m, obs, eps=None, log_ent_coef=None, ent_coef=None, target_entropy=-3.0, other=None, mutant=None):
    """m: td_target_ref.sac_modules().  Exactly one of log_ent_coef (fp32 scalar) and ent_coef.  other: dict with acts,
    acts1, acts2 (lists of [B, 128]), q1_pi, q2_pi and d_log_std of the evaluation this reference is compared with, or
    None (the reference's own choices everywhere)."""
    obs = np.asarray(obs, np.float32)
    B = obs.shape[0]
    ep = np.zeros((B, 3), np.float32) if eps is None else np.asarray(eps, np.float32)
    n_rows = B
    if mutant == "tail_rows":        # the rows of the last tile past B treated as samples (zero observation, zero eps)
        pad = (-B) % 16
        obs, ep = np.concatenate([obs, np.zeros((pad, 18), np.float32)]), np.concatenate([ep, np.zeros((pad, 3), np.float32)])
        n_rows = B + pad
        if other is not None:
            other = None
    fwd = T.sac_target(m, obs, np.zeros(n_rows), np.zeros(n_rows), ep, log_ent_coef=log_ent_coef, ent_coef=ent_coef,
                       mutant="drop_1e-6" if mutant == "drop_1e-6" else None)
    (a, ea), (lp, elp), (ls, els) = fwd["next_actions"], fwd["next_log_prob"], fwd["log_std"]
    mm = reduction_roundings(B)
    fB = float(B)
    div = 1.0 if mutant == "sum_for_mean" else fB
    x, e64 = _f64(obs), _f64(ep)
    info = {}

    # ---- the actor's hidden layers and the raw log_std (for the clamp mask)
    LA = T.layers_of(m["lin"])
    hid_a = _hidden(LA, x, np.zeros_like(x))
    amb_a, own_a, mk_a = _masks(hid_a, None if other is None else other["acts"])
    Wh = np.concatenate([_np32(m["mu"].weight), _np32(m["ls"].weight)])
    bh = np.concatenate([_np32(m["mu"].bias), _np32(m["ls"].bias)])
    y, ey = layer(hid_a[-1][2], hid_a[-1][3], Wh, bh, None, H)
    raw, er = y[:, 3:], ey[:, 3:]
    amb_c = (np.abs(raw + 20.0) <= er) | (np.abs(raw - 2.0) <= er)
    cm = (raw >= -20.0) & (raw <= 2.0)
    if other is not None and amb_c.any():
        cm = np.where(amb_c, np.asarray(other["d_log_std"]) != 0, cm)
    if mutant == "no_clamp_mask":
        cm = np.ones_like(cm)
    cm = cm.astype(np.float64)
    with np.errstate(over="ignore"):
        std = np.exp(ls)
        es = std * np.expm1(els) + ULP["expf"] * ULP_REL * np.exp(ls + els)
    se = (std * e64, np.abs(e64) * es + U * (std + es) * np.abs(e64))

    # ---- the critics: forward masks, dQ_c/da from dq = 1
    if mutant == "cat_action_obs":
        xin, exin, cols = np.concatenate([a, x], axis=1), np.concatenate([ea, np.zeros_like(x)], axis=1), slice(0, 3)
    else:
        xin, exin, cols = np.concatenate([x, a], axis=1), np.concatenate([np.zeros_like(x), ea], axis=1), slice(18, 21)
    dqa, amb_q, own_q = {}, {}, {}
    for c in (1, 2):
        Lc = T.layers_of(m[f"q{c}"])
        hid = _hidden(Lc[:-1], xin, exin)
        amb_q[c], own_q[c], mk = _masks(hid, None if other is None else other[f"acts{c}"])
        dz, edz = mk[2] * _f64(Lc[-1][0])[0][None], np.zeros_like(mk[2])
        for l in (2, 1):
            da, eda = _back(dz, edz, Lc[l][0])
            dz, edz = mk[l - 1] * da, mk[l - 1] * eda
        dqa[c] = _back(dz, edz, _f64(Lc[0][0])[:, cols])
    (q1, e1), (q2, e2) = fwd["q1"], fwd["q2"]
    amb_m = np.abs(q1 - q2) <= e1 + e2
    sel1 = q1 <= q2
    if other is not None:
        sel1 = np.where(amb_m, np.asarray(other["q1_pi"], np.float64) <= np.asarray(other["q2_pi"], np.float64), sel1)
    own_sel1 = q1 <= q2
    if mutant == "max_for_min":
        sel1 = ~sel1
    elif mutant == "q1_only":
        sel1 = np.ones_like(sel1)
    dq = (np.where(sel1[:, None], dqa[1][0], dqa[2][0]), np.where(sel1[:, None], dqa[1][1], dqa[2][1]))
    qmin = (np.where(sel1, q1, q2), np.maximum(e1, e2))

    # ---- head gradients
    if (log_ent_coef is None) == (ent_coef is None):
        raise ValueError("exactly one of log_ent_coef and ent_coef")
    if log_ent_coef is not None:
        al = float(np.exp(np.float64(np.float32(log_ent_coef))))
        alpha = (al, ULP["expf"] * ULP_REL * al)
    else:
        alpha = (float(np.float32(ent_coef)), 0.0)
    al_g = (0.0, 0.0) if mutant == "drop_entropy_term" else alpha
    ab = (al_g[0] / div, (al_g[1] + U * (al_g[0] + al_g[1])) / div)
    A_ = (a, ea)
    s = _add((np.ones_like(a), np.zeros_like(a)), tuple(v * k for v, k in zip(_mul(A_, A_), (-1.0, 1.0))))
    e6 = 0.0 if mutant == "drop_1e-6" else T.EPS6
    w = s[0] + e6
    ew = s[1] + abs(T.EPS6_F32 - T.EPS6) + U * (np.abs(w) + s[1])
    num = _mul((2.0 * a, 2.0 * ea), s)
    with np.errstate(divide="ignore", invalid="ignore"):
        w_lo = np.maximum(w - ew, T.EPS6_F32)
        t_v = num[0] / w
        t_e = num[1] / w_lo + np.abs(num[0]) * ew / (np.abs(w) * w_lo)
        t_e = t_e + U * (np.abs(t_v) + t_e)
    t = (t_v, t_e)
    dla = (-dq[0] / div, (dq[1] + U * (np.abs(dq[0]) + dq[1])) / div)
    if mutant == "sign_of_q":
        dla = (-dla[0], dla[1])
    dls_ = dla if mutant == "drop_tanh_jacobian" else _mul(dla, s)
    d_mu = _add(_mul(ab, t), dls_)
    inner = _add((-np.ones_like(a), np.zeros_like(a)), _mul(t, se))
    d_ls = _add(_mul(ab, inner), _mul(dls_, se))
    d_ls = (cm * d_ls[0], cm * d_ls[1])
    if mutant == "mu_ls_swapped":
        d_mu, d_ls = d_ls, d_mu
    dh, edh = np.concatenate([d_mu[0], d_ls[0]], axis=1), np.concatenate([d_mu[1], d_ls[1]], axis=1)

    # ---- the losses
    te = float(np.float32(target_entropy))
    t1 = _add(_mul(al_g, (lp, elp)), (qmin[0] if mutant == "sign_of_q" else -qmin[0], qmin[1]))
    t2 = (lp + te, elp + U * (np.abs(lp + te) + elp))
    S1, S2 = _sum(*t1, mm), _sum(*t2, mm)
    out = {"actor_loss": tuple(np.array(v) for v in (S1[0] / div, S1[1] / div + U * (abs(S1[0]) + S1[1]) / div))}
    mean2 = (S2[0] / div, S2[1] / div + U * (abs(S2[0]) + S2[1]) / div)
    if log_ent_coef is not None:
        lec = float(np.float32(log_ent_coef))
        out["ent.grad"] = (np.array([mean2[0] if mutant == "ent_grad_sign" else -mean2[0]]), np.array([mean2[1]]))
        out["ent_coef_loss"] = (np.array(-lec * mean2[0]), np.array(abs(lec) * mean2[1] + U * abs(lec) * (abs(mean2[0]) + mean2[1])))

    # ---- the actor's backward pass
    a3, ea3 = hid_a[2][2], hid_a[2][3]
    wh_g = _bsum(dh, edh, a3, ea3, mm)
    bh_g = _sum(dh, edh, mm, axis=0)
    out.update({"mu.w": (wh_g[0][:3], wh_g[1][:3]), "ls.w": (wh_g[0][3:], wh_g[1][3:]),
                "mu.b": (bh_g[0][:3], bh_g[1][:3]), "ls.b": (bh_g[0][3:], bh_g[1][3:])})
    W64 = _f64(Wh)
    da, eda = dh @ W64, edh @ np.abs(W64) + gamma(6) * ((np.abs(dh) + edh) @ np.abs(W64))
    dz, edz = mk_a[2] * da, mk_a[2] * eda
    acts = [(x, np.zeros_like(x))] + [(h, e) for _, _, h, e in hid_a]
    for l in (2, 1, 0):
        out[f"a.w{l}"] = _bsum(dz, edz, *acts[l], mm)
        out[f"a.b{l}"] = _sum(dz, edz, mm, axis=0)
        if l == 0:
            break
        da, eda = _back(dz, edz, LA[l][0])
        mk = mk_a[l] if mutant == "mask_from_above" else mk_a[l - 1]
        dz, edz = mk * da, mk * eda
    cut = slice(0, B)
    out.update(actions_pi=(a[cut], ea[cut]), log_prob=(lp[cut], elp[cut]), q1_pi=(q1[cut], e1[cut]), q2_pi=(q2[cut], e2[cut]),
               dq_da=(dq[0][cut], dq[1][cut]), d_mu=(d_mu[0][cut], d_mu[1][cut]), d_log_std=(d_ls[0][cut], d_ls[1][cut]))

    # ---- what the conditions and the mask / min checks need
    n_a, n_q = sum(int(v.sum()) for v in amb_a), sum(int(v.sum()) for c in (1, 2) for v in amb_q[c])
    clear = ~amb_m
    info.update(ambiguous_actor=amb_a, mask_actor=own_a, ambiguous_critic=amb_q, mask_critic=own_q,
                ambiguous_min=amb_m, select1=own_sel1, ambiguous_clamp=amb_c, clamp_mask=(raw >= -20.0) & (raw <= 2.0),
                actor_share=n_a / sum(v.size for v in amb_a), critic_share=n_q / sum(v.size for c in (1, 2) for v in amb_q[c]),
                min_rows=int(amb_m.sum()), clamp_components=int(amb_c.sum()),
                selected=(int((own_sel1 & clear).sum()), int((~own_sel1 & clear).sum())), clear_rows=int(clear.sum()),
                raw=(raw, er), std=(std, es), mean=(y[:, :3], ey[:, :3]), alpha=alpha, B=B)
    return out, info


def eager_pair_allowance(info, eps):
    """(allowance for d_mu, for d_log_std) [B, 3]: what eager autograd's uncancelled pair of the Normal log-prob adds (the
    docstring's derivation; not fitted)."""
    (mean, em), (std, es), (al, eal) = info["mean"], info["std"], info["alpha"]
    ae = np.abs(_f64(eps))
    size = (np.abs(mean) + em + (std + es) * ae) / np.maximum(std - es, 0.5 * std)
    k = EAGER_PAIR_ROUNDINGS * U * (al + eal) / info["B"]
    return k * size / np.maximum(std - es, 0.5 * std), k * size * ae


def assert_conditions(info, what, stress=False):
    """The conditions on the test case: stated from the reference alone, before any comparison."""
    B = info["B"]
    critic_cap, min_cap = (STRESS_CRITIC_SHARE, STRESS_MIN_SHARE) if stress else (MAX_CRITIC_SHARE, MAX_MIN_SHARE)
    assert info["actor_share"] <= MAX_ACTOR_SHARE, f"{what}: actor ReLU ambiguous share {info['actor_share']:.2e} > {MAX_ACTOR_SHARE}"
    assert info["critic_share"] <= critic_cap, f"{what}: critic ReLU ambiguous share {info['critic_share']:.2e} > {critic_cap}"
    cap = min_cap * B if B >= 10 else 1
    assert info["min_rows"] <= cap, f"{what}: {info['min_rows']} ambiguous min rows > {cap}"
    if B >= 100:
        for c, k in enumerate(info["selected"], start=1):
            assert k >= MIN_SELECTED_SHARE * info["clear_rows"], f"{what}: critic {c} selected on {k} of {info['clear_rows']} unambiguous rows"
    assert info["clamp_components"] == 0, f"{what}: {info['clamp_components']} ambiguous clamp components"
    if stress:
        (raw, er), cm = info["raw"], info["clamp_mask"]
        assert (raw[:, 0] - er[:, 0] > 2.0).all() and (raw[:, 2] + er[:, 2] < -20.0).all(), f"{what}: the clamps are not firmly active"
        assert not cm[:, [0, 2]].any() and cm[:, 1].all(), f"{what}: the clamp mask is not (0, 1, 0)"


def describe(info):
    return (f"ambiguous: actor {info['actor_share']:.1e} critic {info['critic_share']:.1e} min rows {info['min_rows']} "
            f"clamp {info['clamp_components']}; selected {info['selected']}")


def assert_choices(info, parts, what):
    """Off the ambiguous sets the compared evaluation's ReLU masks and min choice equal the reference's."""
    sets = [("actor", info["ambiguous_actor"], info["mask_actor"], parts["acts"])]
    sets += [(f"critic {c}", info["ambiguous_critic"][c], info["mask_critic"][c], parts[f"acts{c}"]) for c in (1, 2)]
    for name, ambs, mks, acts in sets:
        for l, (amb, mk, act) in enumerate(zip(ambs, mks, acts)):
            bad = ((_host(act) > 0) != mk) & ~amb
            assert not bad.any(), f"{what}: {name} layer {l}: {int(bad.sum())} masks differ off the ambiguous pairs, first {tuple(np.argwhere(bad)[0])}"
    got1 = _host(parts["q1_pi"]) <= _host(parts["q2_pi"])
    bad = (got1 != info["select1"]) & ~info["ambiguous_min"]
    assert not bad.any(), f"{what}: min picks another critic on {int(bad.sum())} unambiguous rows, first {int(np.argwhere(bad)[0][0])}"
    want = np.where(got1[:, None], 1, 2)
    return want


def _host(v):
    return v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)


def assert_all_within(got, ref, what, worst=None):
    """Every output of ref present in got within its bound; worst: dict of the largest ratio per output, updated."""
    for k, rb in ref.items():
        if k not in got or got[k] is None:
            continue
        r = R.assert_within(_host(got[k]).reshape(rb[0].shape), rb, f"{what} {k}")
        if worst is not None:
            worst[k] = max(worst.get(k, 0.0), r)


def outside(got, ref):
    """Names of the outputs of got (name -> array) with an element outside ref's bound."""
    return [k for k, rb in ref.items() if k in got and R.ratio(np.asarray(got[k]).reshape(rb[0].shape), rb)[1].any()]


# ----------------------------------------------------------------------------------------------------------- fp32 restatement
def actor_grad_f32(m, obs, eps=None, log_ent_coef=None, ent_coef=None, target_entropy=-3.0):
    """The whole statement in numpy float32, every operation rounded to fp32, sums pairwise: a second fp32 evaluation that
    must sit inside the bound.  Returns name -> float32 array, the parts' names included (acts, acts1, acts2 as lists)."""
    f = np.float32
    x = np.asarray(obs, f)
    B = x.shape[0]
    ep = np.zeros((B, 3), f) if eps is None else np.asarray(eps, f)
    fB = f(B)
    LA = T.layers_of(m["lin"])
    acts, h = [x], x
    for W, b in LA:
        h = np.maximum(T._dense32(h, W, b), f(0))
        acts.append(h)
    Wh = np.concatenate([_np32(m["mu"].weight), _np32(m["ls"].weight)])
    bh = np.concatenate([_np32(m["mu"].bias), _np32(m["ls"].bias)])
    y = T._dense32(h, Wh, bh)
    mean, raw = y[:, :3], y[:, 3:]
    ls = np.clip(raw, f(-20), f(2))
    std = np.exp(ls)
    se = std * ep
    g = mean + se
    a = np.tanh(g)
    dd = g - mean
    lpc = -(dd * dd) / (f(2) * (std * std)) - np.log(std) - f(R.LOG_SQRT_2PI)
    sq = np.log((f(1) - a * a) + f(1e-6))
    lp = ((lpc[:, 0] + lpc[:, 1]) + lpc[:, 2]) - ((sq[:, 0] + sq[:, 1]) + sq[:, 2])
    xin = np.concatenate([x, a], axis=1)
    out, qs, dqs = {}, [], []
    for c in (1, 2):
        Lc = T.layers_of(m[f"q{c}"])
        ca, hc = [], xin
        for W, b in Lc[:-1]:
            hc = np.maximum(T._dense32(hc, W, b), f(0))
            ca.append(hc)
        qs.append(T._dense32(hc, *Lc[-1])[:, 0])
        dz = np.where(ca[2] > 0, Lc[-1][0][0][None], f(0)).astype(f)
        for l in (2, 1):
            da = T._dense32(dz, np.ascontiguousarray(Lc[l][0].T), np.zeros(H, f))
            dz = np.where(ca[l - 1] > 0, da, f(0)).astype(f)
        dqs.append(T._dense32(dz, np.ascontiguousarray(Lc[0][0][:, 18:21].T), np.zeros(3, f)))
        out[f"acts{c}"] = ca
    sel1 = qs[0] <= qs[1]
    dq = np.where(sel1[:, None], dqs[0], dqs[1])
    qmin = np.where(sel1, qs[0], qs[1])
    alpha = np.exp(f(log_ent_coef)) if log_ent_coef is not None else f(ent_coef)
    ab = alpha / fB
    s = f(1) - a * a
    t = ((f(2) * a) * s) / (s + f(1e-6))
    dla = -(dq / fB)
    d_mu = ab * t + dla * s
    cm = (raw >= f(-20)) & (raw <= f(2))
    d_ls = np.where(cm, ab * (f(-1) + t * se) + (dla * s) * se, f(0)).astype(f)
    dh = np.concatenate([d_mu, d_ls], axis=1).astype(f)
    out["actor_loss"] = np.array((alpha * lp - qmin).sum(dtype=f) / fB, f)
    if log_ent_coef is not None:
        mean2 = (lp + f(target_entropy)).sum(dtype=f) / fB
        out["ent.grad"] = np.array([-mean2], f)
        out["ent_coef_loss"] = np.array(-(f(log_ent_coef) * mean2), f)
    wh_g = _bsum32(dh, acts[3])
    bh_g = np.ascontiguousarray(dh.T).sum(axis=1, dtype=f)
    out.update({"mu.w": wh_g[:3], "ls.w": wh_g[3:], "mu.b": bh_g[:3], "ls.b": bh_g[3:]})
    da = T._dense32(dh, np.ascontiguousarray(Wh.T), np.zeros(H, f))
    dz = np.where(acts[3] > 0, da, f(0)).astype(f)
    for l in (2, 1, 0):
        out[f"a.w{l}"] = _bsum32(dz, acts[l])
        out[f"a.b{l}"] = np.ascontiguousarray(dz.T).sum(axis=1, dtype=f)
        if l == 0:
            break
        da = T._dense32(dz, np.ascontiguousarray(LA[l][0].T), np.zeros(H, f))
        dz = np.where(acts[l] > 0, da, f(0)).astype(f)
    out.update(actions_pi=a, log_prob=lp, q1_pi=qs[0], q2_pi=qs[1], dq_da=dq, d_mu=d_mu, d_log_std=d_ls, acts=acts[1:])
    return out
