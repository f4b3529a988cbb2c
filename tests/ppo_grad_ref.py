"""Host-only fp64 restatement of the PPO / A2C loss kernels (csrc/meshenv_ppo_grad.h: k_ppo_adv_stats, k_ppo_grad,
k_ppo_grad_reduce, k_ppo_grad_clip) with manual backpropagation and a per-element bound on the kernels' fp32 error, by the
rules at the top of tests/policy_ref.py.  Shared by tests/test_ppo_grad_cpu.py, tests/test_gpu_ppo_grad.py and
tests/test_gpu_policy_refresh.py; nothing here touches a device.

``ppo_grad(m, data, hp)`` returns ``({name: (ref, bound)}, info)`` for the scalars ``loss policy_loss value_loss entropy_loss
approx_kl clip_fraction grad_norm``, the per-row parts ``log_prob ratio values advantages``, the kept activations ``acts_pi.0
acts_pi.1 acts_vf.0 acts_vf.1`` ([B, H]: a_l with the bound of act(z_l)) and the 13 gradients ``pi.w0 pi.b0
pi.w1 pi.b1 pi.wh pi.bh vf.w0 ... vf.bh log_std`` (torch's shapes) of SB3's PPO.train / A2C.train statement (``eager`` below
is its transcription).  m: ``modules()``; data: ``batch()``; hp: ``hyper()``.

The chain, in the kernel's order, each bound built from the one before (u = 2^-24, gamma_m = m u / (1 - m u); "mul", "add"
are one fp32 operation: the propagated input errors plus u times the largest result the kernel can form):

  a_l          = act(W_l a_{l-1} + b_l), l = 1, 2    policy_ref.layer: gamma_{K/2+2}, K = 32 then H; relu_err / tanh_err (4 ulp)
  mean, v      = W_h a_2 + b_h                       the same, K = H
  log_prob     policy_ref._log_prob: k_policy_forward's sequence (expf, logf at 4 ulp, the fp32 literal of log sqrt(2 pi))
  mean_adv     = S / B, S one sum of B terms         gamma_B (any order of at most B roundings), one u for the division
  inv_std      = 1 / (sqrt(S2 / (B - 1)) + 1e-8)     c = adv - mean_adv (add), c c (mul), S2 gamma_B, division u, sqrtf 1 ulp,
                                                     add u and the fp32 literal of 1e-8, division u
  adv'         = (adv - mean_adv) inv_std            add, mul
  log_ratio    = log_prob - old_log_prob (add);  ratio = expf(log_ratio): exp's slope over the interval, + 4 ulp
  p1, p2       = adv' ratio, adv' clamp(ratio)       mul each; the clamp passes at most the error of ratio
  c            = passes ? -(p1 / B) : 0              one u (A2C: -(adv' / B))
  d_mean       = (c d) / var, var = std std          mul, then a division by a var that carries expf's error twice and one u
  dls term     = c ((d d) / var - 1)                 mul, division, add, mul
  d_v          = (vf_coef (2 diff)) / B              diff = v - returns (add); the doubling is exact; mul, division
  row sums     policy, value, kl, the gradients      BATCH SUMS with m = critic_grad_ref.reduction_roundings(B) (the same nwg policy)
  da_2         = sum_i d_head[i] W_h[i]              one product and two fmaf (pi: gamma_3; vf: gamma_1)
  dz_l         = act'(a_l) da_l                      ReLU: a select, exact; Tanh: 1 - a a (mul, add), then mul
  da_1         = dz_2 W_2                            two fma chains of H / 2 terms and their sum: gamma_{H/2+1}
  d_log_std    = (sum of the dls terms) - ent_coef   one more u
  entropy_loss = -sum_i (c + log_std_i), c = 0.5 + 0.5 log(2 pi): the kernel's five additions and the fp32 literal; the bound also
                 admits evaluations that form log(exp(log_std)) (torch's Normal.entropy: expf and logf allowances) and that
                 take the mean of the B equal rows in any order of at most m roundings (gamma_m): the kernel does neither
  total_norm   the 2-norm of the 13 per-tensor 2-norms: |norm(g + e) - norm(g)| <= norm(e) for the gradients' own bounds e, and
                 the relative error gamma_{n_grad} of a sum of n_grad squares in any order (halved by the root, not claimed), the
                 roots' ulp; coef = min(max_grad_norm / (total_norm + 1e-6), 1) carries it on (division, add: 3 u); exactly 1
                 where the norm lies firmly below max_grad_norm; the clipped gradient is one more mul

AMBIGUOUS SETS, from the reference alone (``assert_conditions`` caps them BEFORE anything is compared):
  * ReLU pairs with |z_ref| <= e_z: either mask is a correct fp32 evaluation; the reference takes the mask of the evaluation it
    is compared with (``other``).  Cap: share <= 2e-4 per tower (actor_grad_ref.MAX_ACTOR_SHARE).
  * clip rows: ratio within its bound of lo / hi while the branch matters (at hi with adv' > 0, at lo with adv' < 0, or adv'
    within its own bound of 0 outside the range); the reference takes ``other``'s pass there.  Cap: 1 % of B, one row when B < 100.
  * the norm: |total_norm + 1e-6 - max_grad_norm| <= its bound.  Cap: none may occur.
Coverage at B >= 100 (PPO): at least 10 % of rows on each side of the predicate; each clipped-and-zeroed edge (ratio > hi with
adv' > 0, ratio < lo with adv' < 0) on at least 2 % of rows.
"""
from __future__ import annotations

import numpy as np

import policy_ref as R
import td_target_ref as T
from actor_grad_ref import MAX_ACTOR_SHARE, _add, _host, _mul, _sum
from critic_grad_ref import _bsum, _bsum32, reduction_roundings
from policy_ref import U, ULP, ULP_REL, _f64, _np32, gamma, layer, relu_err, tanh_err

CASES = {"ppo-relu128": ("relu", 128, False), "a2c-tanh64": ("tanh", 64, True), "ppo-tanh128": ("tanh", 128, False),
         "ppo-relu64": ("relu", 64, False)}                 # activation, width, A2C's loss
BOTH_SETS = ("ppo-relu128", "a2c-tanh64")                   # the cases that also run on the stress weight set
GPU_BS = (1, 17, 100, 256, 4101)
MAX_GRAD_NORM = 0.1            # the tests' max_grad_norm: firmly below the total norm of every case here (they lie in 0.2 .. 30)
MAX_CLIP_SHARE = 0.01
MIN_SIDE_SHARE, MIN_EDGE_SHARE = 0.10, 0.02
SCALARS = ("loss", "policy_loss", "value_loss", "entropy_loss", "approx_kl", "clip_fraction", "grad_norm")
PARTS = ("log_prob", "ratio", "values", "advantages")
ACTS = tuple(f"acts_{t}.{l}" for t in ("pi", "vf") for l in (0, 1))     # the kept activations a_1, a_2 of each tower, [B, H]
GRADS = tuple(f"{t}.{n}" for t in ("pi", "vf") for n in ("w0", "b0", "w1", "b1", "wh", "bh")) + ("log_std",)
ENT_C = 0.5 + 0.5 * np.log(2.0 * np.pi)
MUTANTS = ("clamp_ignored", "clip_regardless_of_sign", "tie_half", "biased_std", "eps_inside_root", "normalised_at_b1",
           "old_new_swapped", "dls_minus_one_dropped", "entropy_sign", "vf_coef_dropped", "mse_factor_2_dropped",
           "per_tensor_clip", "coef_not_clamped")


def _r32(v):
    return float(np.float32(v))


def hyper(clip_range=0.2, ent_coef=0.01, vf_coef=0.5, normalize_advantage=True, max_grad_norm=0.5):
    """The hyper-parameters as the kernel receives them: rounded to float32 (clip_range=None: A2C's loss)."""
    return dict(clip_range=None if clip_range is None else _r32(clip_range), ent_coef=_r32(ent_coef), vf_coef=_r32(vf_coef),
                normalize_advantage=bool(normalize_advantage), max_grad_norm=None if max_grad_norm is None else _r32(max_grad_norm))


# ----------------------------------------------------------------------------------------------------------- inputs
def modules(case, stress=False, seed=11):
    """torch (CPU) modules of an SB3 ActorCriticPolicy of the case's width: dict(act, H, a2c, pi, vf, action_net, value_net,
    log_std); torch's default init and SB3's log_std_init = 0.  stress: log_std = (-3, 0, 1), the first layers x 3 (Tanh
    saturates on part of the rows, ReLU pre-activations grow) and both heads x 4."""
    import torch
    act, H, a2c = CASES[case]
    m = R.policy_modules(("actor_critic", H, act), seed=seed)
    m["log_std"] = torch.nn.Parameter(torch.tensor([-3.0, 0.0, 1.0]) if stress else torch.zeros(3))
    if stress:
        with torch.no_grad():
            m["pi"][0].weight.mul_(3.0)
            m["vf"][0].weight.mul_(3.0)
            m["action_net"].weight.mul_(4.0)
            m["value_net"].weight.mul_(4.0)
    m.update(act=act, H=H, a2c=a2c)
    return m


def params(m):
    """The 13 parameters in bind order."""
    out = []
    for t, head in (("pi", "action_net"), ("vf", "value_net")):
        for l in (*m[t], m[head]):
            out += [l.weight, l.bias]
    return out + [m["log_std"]]


def _towers(m):
    return {"pi": T.layers_of([*m["pi"], m["action_net"]]), "vf": T.layers_of([*m["vf"], m["value_net"]])}


def batch(m, B, rows, seed=41, adv_scale=1.0):
    """A minibatch as SB3's RolloutBufferSamples lays it out, float32: observations (td_target_ref.tight_rows of
    policy_ref.input_rows(), repeated beyond their length), actions = mean + std eps, old_log_prob = log_prob + N(0, 0.3),
    advantages N(0.2, 1) adv_scale (both signs), returns N(0, 1) (the order of a discounted return of boundary()'s rewards)."""
    rng = np.random.default_rng(seed + B)
    rows = np.asarray(rows, np.float32)
    rows = rows[T.tight_rows(rows)]
    obs = np.ascontiguousarray(np.resize(rows, (B, 18)).astype(np.float32))
    L = _towers(m)["pi"]
    h = _f64(obs)
    for W, b in L[:-1]:
        z = h @ _f64(W).T + _f64(b)
        h = np.tanh(z) if m["act"] == "tanh" else np.maximum(z, 0.0)
    mean = h @ _f64(L[-1][0]).T + _f64(L[-1][1])
    std = np.exp(_f64(_np32(m["log_std"])))
    actions = (mean + std * rng.standard_normal((B, 3))).astype(np.float32)
    d = _f64(actions) - mean
    lp = (-(d * d) / (2.0 * std * std) - np.log(std) - R.LOG_SQRT_2PI).sum(axis=1)
    old = (lp + 0.3 * rng.standard_normal(B)).astype(np.float32)
    adv = ((0.2 + rng.standard_normal(B)) * adv_scale).astype(np.float32)
    ret = rng.standard_normal(B).astype(np.float32)
    return dict(observations=obs, actions=actions, old_log_prob=old, advantages=adv, returns=ret)


# ----------------------------------------------------------------------------------------------------------- pieces
def _act(act, z, ez):
    if act == "tanh":
        return np.tanh(z), tanh_err(z, ez)
    return np.maximum(z, 0.0), relu_err(z, ez)


def _dact(act, a, ea, da, eda, mask):
    """dz = act'(a) da: ReLU a select by `mask`; Tanh da (1 - a a)."""
    if act == "relu":
        return mask * da, mask * eda
    s = _add((np.ones_like(a), np.zeros_like(a)), tuple(v * k for v, k in zip(_mul((a, ea), (a, ea)), (-1.0, 1.0))))
    return _mul((da, eda), s)


def _div(x, ex, y, ey):
    """x / y for y > ey > 0, correctly rounded."""
    q = x / y
    eq = (ex + np.abs(q) * ey) / (y - ey)
    return q, eq + U * (np.abs(q) + eq)


def _tower_back(act, H, layers, x, hid, dh, edh, mm, masks, name, out):
    """The backward pass of one tower from its head gradient dh [B, n_out] into out[name.*]."""
    (z1, ez1, a1, ea1), (z2, ez2, a2, ea2) = hid
    Wh = _f64(layers[2][0])
    out[f"{name}.wh"] = _bsum(dh, edh, a2, ea2, mm)
    out[f"{name}.bh"] = _sum(dh, edh, mm, axis=0)
    da = dh @ Wh
    eda = edh @ np.abs(Wh) + gamma(Wh.shape[0]) * ((np.abs(dh) + edh) @ np.abs(Wh))
    dz, edz = _dact(act, a2, ea2, da, eda, masks[1])
    out[f"{name}.w1"] = _bsum(dz, edz, a1, ea1, mm)
    out[f"{name}.b1"] = _sum(dz, edz, mm, axis=0)
    W2 = _f64(layers[1][0])
    da = dz @ W2
    eda = edz @ np.abs(W2) + gamma(H // 2 + 1) * ((np.abs(dz) + edz) @ np.abs(W2))
    dz, edz = _dact(act, a1, ea1, da, eda, masks[0])
    out[f"{name}.w0"] = _bsum(dz, edz, x, np.zeros_like(x), mm)
    out[f"{name}.b0"] = _sum(dz, edz, mm, axis=0)


def _forward(act, H, layers, x):
    hid, h, e = [], x, np.zeros_like(x)
    for i, (W, b) in enumerate(layers[:2]):
        z, ez = layer(h, e, W, b, None, 32 if i == 0 else H)
        h, e = _act(act, z, ez)
        hid.append((z, ez, h, e))
    return hid, layer(h, e, *layers[2], None, H)


def _masks(act, hid, other_acts):
    if act != "relu":
        return [np.zeros(z.shape, bool) for z, _, _, _ in hid], [None, None], [None, None]
    amb = [np.abs(z) <= ez for z, ez, _, _ in hid]
    own = [z > 0 for z, _, _, _ in hid]
    use = own if other_acts is None else [np.where(a, _host(o)[:len(a)] > 0, k) for a, k, o in zip(amb, own, other_acts)]
    return amb, own, [k.astype(np.float64) for k in use]


# ----------------------------------------------------------------------------------------------------------- the restatement
def ppo_grad(m, data, hp, other=None, mutant=None):
    """other: dict with acts_pi, acts_vf (two [B, H] each) and pass [B] of the evaluation this reference is compared with, or
    None (the reference's own choices everywhere)."""
    act, H, a2c = m["act"], m["H"], hp["clip_range"] is None
    x = _f64(data["observations"])
    B = x.shape[0]
    mm = reduction_roundings(B)
    fB = float(B)
    Lw = _towers(m)
    ls = _f64(_np32(m["log_std"]))
    std = np.exp(ls)
    r_e = ULP["expf"] * ULP_REL
    out = {}

    # ---- forward: both towers, log_prob
    hid_p, (mean, em) = _forward(act, H, Lw["pi"], x)
    hid_v, (v, ev) = _forward(act, H, Lw["vf"], x)
    v, ev = v[:, 0], ev[:, 0]
    amb_p, own_p, mk_p = _masks(act, hid_p, None if other is None else other["acts_pi"])
    amb_v, own_v, mk_v = _masks(act, hid_v, None if other is None else other["acts_vf"])
    a = _f64(data["actions"])
    lp, elp = R._log_prob(a, mean, em, std, r_e)
    d = a - mean
    ed = em + U * (np.abs(d) + em)

    # ---- the advantages
    adv, eadv = _f64(data["advantages"]).reshape(-1), np.zeros(B)
    norm_it = hp["normalize_advantage"] and (B > 1 or mutant == "normalised_at_b1")
    if norm_it and B == 1:
        adv = np.zeros(1)           # the mutant: (adv - adv) / (0 + 1e-8)
    elif norm_it:
        mu = adv.mean()
        emu = gamma(B) * np.abs(adv).mean() + U * abs(mu)
        c0 = adv - mu
        ec0 = emu + U * (np.abs(c0) + emu)
        sq, esq = _mul((c0, ec0), (c0, ec0))
        S2, eS2 = _sum(sq, esq, B)
        nvar = fB if mutant == "biased_std" else fB - 1.0
        var_a, evar_a = S2 / nvar, eS2 / nvar + U * (S2 + eS2) / nvar
        lit = abs(_r32(1e-8) - 1e-8)
        if mutant == "eps_inside_root":
            den, eden = np.sqrt(var_a + 1e-8), evar_a / (2.0 * np.sqrt(max(var_a - evar_a, 1e-300))) + 2.0 * U * np.sqrt(var_a + 1e-8)
        else:
            sd = np.sqrt(var_a)
            esd = evar_a / (2.0 * np.sqrt(max(var_a - evar_a, 1e-300))) + ULP["sqrtf"] * ULP_REL * sd
            den, eden = sd + 1e-8, esd + lit + U * (sd + 1e-8 + esd)
        inv, einv = _div(1.0, 0.0, den, eden)
        adv, eadv = _mul((c0, ec0), (np.full(B, inv), np.full(B, einv)))

    # ---- the surrogate, the row coefficient c = dL/dlog_prob
    info = dict(B=B, a2c=a2c)
    if a2c:
        sur, esur = _mul((adv, eadv), (lp, elp))
        c, ec = -adv / fB, (eadv + U * (np.abs(adv) + eadv)) / fB
        ratio, eratio = np.ones(B), np.zeros(B)
        kl = cfv = (np.zeros(B), np.zeros(B))
        passes, amb_clip = np.ones(B, bool), np.zeros(B, bool)
        cf_amb = 0
    else:
        clip = hp["clip_range"]
        lo, hi = _r32(1.0 - clip), _r32(1.0 + clip)
        old = _f64(data["old_log_prob"]).reshape(-1)
        lr = (old - lp) if mutant == "old_new_swapped" else (lp - old)
        elr = elp + U * (np.abs(lr) + elp)
        ratio = np.exp(lr)
        eratio = ratio * np.expm1(elr) + ULP["expf"] * ULP_REL * ratio * np.exp(elr)
        p1 = _mul((adv, eadv), (ratio, eratio))
        p2 = _mul((adv, eadv), (np.clip(ratio, lo, hi), eratio))
        inside = (ratio >= lo) & (ratio <= hi)
        passes = inside | (p1[0] < p2[0])
        near_hi, near_lo = np.abs(ratio - hi) <= eratio, np.abs(ratio - lo) <= eratio
        amb_clip = (near_hi & (adv > -eadv)) | (near_lo & (adv < eadv)) | (~inside & ~near_hi & ~near_lo & (np.abs(adv) <= eadv))
        if other is not None:
            passes = np.where(amb_clip, _host(other["pass"]).reshape(-1)[:B] > 0.5, passes)
        sur, esur = np.minimum(p1[0], p2[0]), np.maximum(p1[1], p2[1])
        share = np.ones(B)
        if mutant == "clamp_ignored":
            sur, esur, passes = p1[0], p1[1], np.ones(B, bool)
        elif mutant == "clip_regardless_of_sign":
            sur, esur, passes = p2[0], p2[1], inside
        elif mutant == "tie_half":
            share = np.where(inside, 0.5, 1.0)
        c = np.where(passes, -p1[0] / fB, 0.0) * share
        ec = np.where(passes, (p1[1] + U * (np.abs(p1[0]) + p1[1])) / fB, 0.0)
        kl = _add(_add((ratio, eratio), (-np.ones(B), np.zeros(B))), (-lr, elr))
        clipf = _r32(clip)
        dist = np.abs(ratio - 1.0)
        cfv = (dist > clipf).astype(np.float64)
        cf_amb = int((np.abs(dist - clipf) <= eratio + U * (dist + eratio)).sum())
        zeroed = ~passes & ~amb_clip
        info.update(pass_share=float(passes.mean()), edge_hi=float((zeroed & (ratio > hi)).mean()),
                    edge_lo=float((zeroed & (ratio < lo)).mean()))
    info.update(ambiguous_clip=amb_clip, passes=passes, clip_share=float(amb_clip.mean()))

    # ---- the heads' gradients
    rho_v = (1 + r_e) ** 2 * (1 + U) - 1.0                 # relative error of the kernel's var = std std
    var = std * std
    evar = np.broadcast_to(rho_v * var, d.shape)
    varb = np.broadcast_to(var, d.shape)
    cd = _mul((c[:, None], ec[:, None]), (d, ed))
    dmean = _div(cd[0], cd[1], varb, evar)
    dd = _mul((d, ed), (d, ed))
    qv = _div(dd[0], dd[1], varb, evar)
    one = 0.0 if mutant == "dls_minus_one_dropped" else -1.0
    s = _add(qv, (np.full(d.shape, one), np.zeros(d.shape)))
    term = _mul((np.broadcast_to(c[:, None], d.shape), np.broadcast_to(ec[:, None], d.shape)), s)
    vf_c, ent_c = hp["vf_coef"], hp["ent_coef"]
    ret = _f64(data["returns"]).reshape(-1)
    diff = v - ret
    ediff = ev + U * (np.abs(diff) + ev)
    k2 = (1.0 if mutant == "mse_factor_2_dropped" else 2.0) * (1.0 if mutant == "vf_coef_dropped" else vf_c)
    dv, edv = k2 * diff / fB, (k2 * ediff + gamma(2) * k2 * (np.abs(diff) + ediff)) / fB
    sqv = _mul((diff, ediff), (diff, ediff))

    # ---- the losses
    def mean_of(x_, ex_):
        S, eS = _sum(x_, ex_, mm)
        return S / fB, eS / fB + U * (abs(S) + eS) / fB
    pl = mean_of(sur, esur)
    pl = (-pl[0], pl[1])
    vl = mean_of(*sqv)
    ent_terms = ENT_C + ls
    el_i = 1.01 * r_e + ULP["logf"] * ULP_REL * (np.abs(ls) + 1.01 * r_e)       # evaluations that form log(exp(log_std))
    ent = ent_terms.sum()
    eent = 3 * abs(_r32(ENT_C) - ENT_C) + el_i.sum() + (gamma(3) + gamma(mm)) * np.abs(ent_terms).sum()
    sign = 1.0 if mutant == "entropy_sign" else -1.0
    el = (sign * ent, eent)
    lossv = _add(_add(pl, _mul((np.float64(ent_c), 0.0), el)), _mul((np.float64(1.0 if mutant == "vf_coef_dropped" else vf_c), 0.0), vl))
    klm, cfm = mean_of(*kl), mean_of(cfv, np.zeros(B)) if not a2c else (0.0, 0.0)
    if a2c:
        klm = (0.0, 0.0)
    out.update(loss=lossv, policy_loss=pl, value_loss=vl, entropy_loss=el, approx_kl=klm,
               clip_fraction=(cfm[0], cfm[1] + cf_amb / fB))

    # ---- backward
    _tower_back(act, H, Lw["pi"], x, hid_p, dmean[0], dmean[1], mm, mk_p, "pi", out)
    _tower_back(act, H, Lw["vf"], x, hid_v, dv[:, None], edv[:, None], mm, mk_v, "vf", out)
    g, eg = _sum(term[0], term[1], mm, axis=0)
    g = g - sign * (-ent_c)
    out["log_std"] = (g, eg + U * (np.abs(g) + eg))

    # ---- clip_grad_norm_
    n_grad = sum(out[k][0].size for k in GRADS)
    total = np.sqrt(sum(float((out[k][0] ** 2).sum()) for k in GRADS))
    etotal = np.sqrt(sum(float((out[k][1] ** 2).sum()) for k in GRADS)) + (gamma(n_grad) + 16 * U) * total
    info.update(total_norm=total, total_norm_bound=etotal, n_grad=n_grad, ambiguous_norm=False)
    mgn = hp["max_grad_norm"]
    if mgn is None:
        out["grad_norm"] = (np.array(np.nan), np.array(np.inf))
    else:
        out["grad_norm"] = (np.array(total), np.array(etotal))
        info["ambiguous_norm"] = bool(abs(total + 1e-6 - mgn) <= etotal + 4 * U * mgn)
        if mutant == "per_tensor_clip":
            for k in GRADS:
                nk = np.sqrt(float((out[k][0] ** 2).sum()))
                out[k] = (out[k][0] * min(mgn / (nk + 1e-6), 1.0), out[k][1])
        elif total + 1e-6 > mgn or mutant == "coef_not_clamped":
            coef = mgn / (total + 1e-6)
            ecoef = coef * (etotal / (total - etotal) + 3 * U)
            for k in GRADS:
                gk, ek = out[k]
                out[k] = (gk * coef, np.abs(gk) * ecoef + coef * ek + ek * ecoef + U * (np.abs(gk) + ek) * (coef + ecoef))
    out.update(log_prob=(lp, elp), ratio=(ratio, eratio), values=(v, ev), advantages=(adv, eadv))
    for t, hid in (("pi", hid_p), ("vf", hid_v)):             # the kept activations: a_l with the bound of act(z_l)
        out.update({f"acts_{t}.{l}": (a_, ea_) for l, (_, _, a_, ea_) in enumerate(hid)})
    n_p, n_v = sum(int(a_.sum()) for a_ in amb_p), sum(int(a_.sum()) for a_ in amb_v)
    info.update(ambiguous_pi=amb_p, mask_pi=own_p, ambiguous_vf=amb_v, mask_vf=own_v, pi_share=n_p / (2.0 * B * H), vf_share=n_v / (2.0 * B * H))
    return out, info


def assert_conditions(info, what):
    """The conditions on the test case: stated from the reference alone, before any comparison."""
    B = info["B"]
    assert info["pi_share"] <= MAX_ACTOR_SHARE, f"{what}: pi ReLU ambiguous share {info['pi_share']:.2e} > {MAX_ACTOR_SHARE}"
    assert info["vf_share"] <= MAX_ACTOR_SHARE, f"{what}: vf ReLU ambiguous share {info['vf_share']:.2e} > {MAX_ACTOR_SHARE}"
    n_amb = int(info["ambiguous_clip"].sum())
    assert n_amb <= (MAX_CLIP_SHARE * B if B >= 100 else 1), f"{what}: {n_amb} ambiguous clip rows of {B}"
    assert not info["ambiguous_norm"], f"{what}: total_norm {info['total_norm']!r} within its bound of max_grad_norm"
    if B >= 100 and not info["a2c"]:
        ps = info["pass_share"]
        assert MIN_SIDE_SHARE <= ps <= 1.0 - MIN_SIDE_SHARE, f"{what}: {ps:.3f} of the rows pass the predicate"
        assert info["edge_hi"] >= MIN_EDGE_SHARE and info["edge_lo"] >= MIN_EDGE_SHARE, \
            f"{what}: clipped-and-zeroed edges on {info['edge_hi']:.3f} / {info['edge_lo']:.3f} of the rows"


def describe(info):
    s = f"ambiguous: relu pi {info['pi_share']:.1e} vf {info['vf_share']:.1e} clip rows {int(info['ambiguous_clip'].sum())}"
    if "pass_share" in info:
        s += f"; pass {info['pass_share']:.2f} edges {info['edge_hi']:.3f} / {info['edge_lo']:.3f}"
    return s + f"; norm {info['total_norm']:.4f}"


def assert_choices(info, parts, what):
    """Off the ambiguous sets the compared evaluation's ReLU masks and pass mask equal the reference's."""
    for name in ("pi", "vf"):
        for l, (amb, mk, got) in enumerate(zip(info[f"ambiguous_{name}"], info[f"mask_{name}"], parts[f"acts_{name}"])):
            if mk is None:
                continue
            bad = ((_host(got) > 0) != mk) & ~amb
            assert not bad.any(), f"{what}: {name} layer {l}: {int(bad.sum())} masks differ off the ambiguous pairs, first {tuple(np.argwhere(bad)[0])}"
    if not info["a2c"]:
        bad = ((_host(parts["pass"]).reshape(-1) > 0.5) != info["passes"]) & ~info["ambiguous_clip"]
        assert not bad.any(), f"{what}: {int(bad.sum())} rows' pass differs off the ambiguous rows, first {int(np.argwhere(bad)[0][0])}"


def with_acts(got):
    """got with its lists acts_pi, acts_vf (two [B, H] each) also under the reference's names acts_pi.0 ... acts_vf.1."""
    got = dict(got)
    for t in ("pi", "vf"):
        got.update({f"acts_{t}.{l}": a for l, a in enumerate(got[f"acts_{t}"])})
    return got


def assert_all_within(got, ref, what, worst=None, names=None):
    """Every output of ref (or of names) within its bound (got: name -> array or tensor); worst: the largest ratio per output."""
    for k in (names or ref):
        rb = ref[k]
        if not np.isfinite(rb[1]).all():          # grad_norm without a clip launch: NaN by contract
            assert np.isnan(_host(got[k])).all(), f"{what} {k}"
            continue
        r = R.assert_within(_host(got[k]).reshape(np.shape(rb[0])), (np.asarray(rb[0]), np.asarray(rb[1])), f"{what} {k}")
        if worst is not None:
            worst[k] = max(worst.get(k, 0.0), r)


def outside(got, ref, names=None):
    """Names of the outputs with an element outside ref's bound."""
    bad = []
    for k in (names or ref):
        rb = (np.asarray(ref[k][0]), np.asarray(ref[k][1]))
        if k in got and np.isfinite(rb[1]).all() and R.ratio(np.asarray(got[k]).reshape(rb[0].shape), rb)[1].any():
            bad.append(k)
    return bad


# ----------------------------------------------------------------------------------------------------------- eager torch
def eager(torch, mods, data, hp, dtype=None, device=None, backward=True):
    """SB3's statement transcribed on the modules of ``mods`` (moved by the caller; dtype: the dtype of the inputs), with autograd
    and clip_grad_norm_.  Returns name -> tensor for the scalars, the parts and, in ref's naming, p.grad of the 13 parameters."""
    act = torch.tanh if mods["act"] == "tanh" else torch.relu
    ps = params(mods)
    dtype = dtype or ps[0].dtype
    tt = lambda k: torch.as_tensor(data[k]).to(device=ps[0].device, dtype=dtype)   # noqa: E731
    obs, actions, adv, ret = tt("observations"), tt("actions"), tt("advantages").reshape(-1), tt("returns").reshape(-1)
    hp_, hv = obs, obs
    for l in mods["pi"]:
        hp_ = act(l(hp_))
    for l in mods["vf"]:
        hv = act(l(hv))
    dist = torch.distributions.Normal(mods["action_net"](hp_), torch.ones_like(actions) * mods["log_std"].exp())
    log_prob, entropy, values = dist.log_prob(actions).sum(dim=1), dist.entropy().sum(dim=1), mods["value_net"](hv).flatten()
    if hp["normalize_advantage"] and len(adv) > 1:
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    out = {}
    if hp["clip_range"] is None:
        policy_loss = -(adv * log_prob).mean()
        out.update(ratio=torch.ones_like(adv), approx_kl=torch.zeros(()), clip_fraction=torch.zeros(()))
    else:
        clip = hp["clip_range"]
        ratio = torch.exp(log_prob - tt("old_log_prob").reshape(-1))
        lo, hi = _r32(1.0 - clip), _r32(1.0 + clip)     # what a float32 clamp makes of the Python floats 1 -+ clip_range
        policy_loss = -torch.min(adv * ratio, adv * torch.clamp(ratio, lo, hi)).mean()
        log_ratio = log_prob - tt("old_log_prob").reshape(-1)
        out.update(ratio=ratio, approx_kl=((ratio - 1) - log_ratio).mean(), clip_fraction=((ratio - 1).abs() > clip).to(dtype).mean())
    value_loss = torch.nn.functional.mse_loss(ret, values)
    entropy_loss = -torch.mean(entropy)
    loss = policy_loss + hp["ent_coef"] * entropy_loss + hp["vf_coef"] * value_loss
    out.update(loss=loss, policy_loss=policy_loss, value_loss=value_loss, entropy_loss=entropy_loss, log_prob=log_prob, values=values,
               advantages=adv)
    if backward:
        for p in ps:
            p.grad = None
        loss.backward()
        out["grad_norm"] = (torch.nn.utils.clip_grad_norm_(ps, hp["max_grad_norm"]) if hp["max_grad_norm"] is not None
                            else torch.full((), float("nan")))
        out.update({k: p.grad for k, p in zip(GRADS, ps)})
    return {k: v.detach() for k, v in out.items()}


# ----------------------------------------------------------------------------------------------------------- fp32 restatement
def ppo_grad_f32(m, data, hp):
    """The whole statement in numpy float32, every operation rounded to fp32, sums pairwise: a second fp32 evaluation that must
    sit inside the bound.  Returns name -> float32 array, with acts_pi, acts_vf (lists) and pass."""
    f = np.float32
    act, a2c = m["act"], hp["clip_range"] is None
    x = np.asarray(data["observations"], f)
    B = x.shape[0]
    fB = f(B)
    Lw = _towers(m)
    fa = (lambda z: np.tanh(z)) if act == "tanh" else (lambda z: np.maximum(z, f(0)))
    fwd = {}
    for t in ("pi", "vf"):
        a1 = fa(T._dense32(x, *Lw[t][0])).astype(f)
        a2 = fa(T._dense32(a1, *Lw[t][1])).astype(f)
        fwd[t] = (a1, a2, T._dense32(a2, *Lw[t][2]))
    ls = _np32(m["log_std"])
    std = np.exp(ls)
    var = std * std
    mean, v = fwd["pi"][2], fwd["vf"][2][:, 0]
    d = np.asarray(data["actions"], f) - mean
    dd = d * d
    lpc = -dd / (f(2) * var) - np.log(std) - f(R.LOG_SQRT_2PI)
    lp = (lpc[:, 0] + lpc[:, 1]) + lpc[:, 2]
    adv = np.asarray(data["advantages"], f).reshape(-1)
    if hp["normalize_advantage"] and B > 1:
        mu = adv.sum(dtype=f) / fB
        c0 = adv - mu
        sd = np.sqrt((c0 * c0).sum(dtype=f) / f(B - 1))
        adv = c0 * (f(1) / (sd + f(1e-8)))
    out = {}
    if a2c:
        sur, c = adv * lp, -(adv / fB)
        ratio, passes = np.ones(B, f), np.ones(B, bool)
        out.update(approx_kl=f(0), clip_fraction=f(0))
    else:
        clip = f(hp["clip_range"])
        lo, hi = f(1.0 - hp["clip_range"]), f(1.0 + hp["clip_range"])
        lr = lp - np.asarray(data["old_log_prob"], f).reshape(-1)
        ratio = np.exp(lr)
        p1, p2 = adv * ratio, adv * np.clip(ratio, lo, hi)
        sur = np.minimum(p1, p2)
        passes = ((ratio >= lo) & (ratio <= hi)) | (p1 < p2)
        c = np.where(passes, -(p1 / fB), f(0)).astype(f)
        out.update(approx_kl=((ratio - f(1)) - lr).sum(dtype=f) / fB, clip_fraction=(np.abs(ratio - f(1)) > clip).astype(f).sum(dtype=f) / fB)
    dmean = (c[:, None] * d) / var
    term = c[:, None] * (dd / var - f(1))
    diff = v - np.asarray(data["returns"], f).reshape(-1)
    vf_c, ent_c = f(hp["vf_coef"]), f(hp["ent_coef"])
    dv = (vf_c * (f(2) * diff)) / fB
    pl, vl = -(sur.sum(dtype=f) / fB), (diff * diff).sum(dtype=f) / fB
    el = -(((f(ENT_C) + ls[0]) + (f(ENT_C) + ls[1])) + (f(ENT_C) + ls[2]))
    out.update(loss=(pl + ent_c * el) + vf_c * vl, policy_loss=pl, value_loss=vl, entropy_loss=el)

    def dact(a, g):
        return (g * (f(1) - a * a)).astype(f) if act == "tanh" else np.where(a > 0, g, f(0)).astype(f)
    for t, dh in (("pi", dmean.astype(f)), ("vf", dv[:, None].astype(f))):
        a1, a2, _ = fwd[t]
        Wh = Lw[t][2][0]
        out[f"{t}.wh"], out[f"{t}.bh"] = _bsum32(dh, a2), np.ascontiguousarray(dh.T).sum(axis=1, dtype=f)
        dz = dact(a2, T._dense32(dh, np.ascontiguousarray(Wh.T), np.zeros(Wh.shape[1], f)))
        out[f"{t}.w1"], out[f"{t}.b1"] = _bsum32(dz, a1), np.ascontiguousarray(dz.T).sum(axis=1, dtype=f)
        W2 = Lw[t][1][0]
        dz = dact(a1, T._dense32(dz, np.ascontiguousarray(W2.T), np.zeros(W2.shape[1], f)))
        out[f"{t}.w0"], out[f"{t}.b0"] = _bsum32(dz, x), np.ascontiguousarray(dz.T).sum(axis=1, dtype=f)
    out["log_std"] = np.ascontiguousarray(term.T).sum(axis=1, dtype=f) - ent_c
    if hp["max_grad_norm"] is None:
        out["grad_norm"] = f(np.nan)
    else:
        total = np.sqrt(sum((np.sqrt((out[k].astype(f) ** 2).sum(dtype=f)) ** 2 for k in GRADS), f(0)))
        coef = min(f(hp["max_grad_norm"]) / (total + f(1e-6)), f(1))
        for k in GRADS:
            out[k] = (out[k] * coef).astype(f)
        out["grad_norm"] = total
    out.update(log_prob=lp, ratio=ratio, values=v, advantages=adv, acts_pi=list(fwd["pi"][:2]), acts_vf=list(fwd["vf"][:2]))
    out["pass"] = passes.astype(f)
    return out


# ----------------------------------------------------------------------------------------------------------- one Adam step
def adam_step_bound(p, g, eg, lr, betas, eps, stats=None):
    """The one-step bound of tests/optim_step_ref.py (its operation sequence and primitives, first step from zero moments) on
    the stepped parameter, for a float32 gradient that is only known to lie within eg of g: the gradient's bound enters as the
    input error of G.  Where the interval of the denominator reaches 0 (a gradient within its bound of 0) the analysis gives
    nothing; there the bound is the cap 2.002 lr + 4 u |p|: at step 1 the update is lr g / (|g| + eps'), at most lr on
    either side whatever g is.  stats (a dict): gains ``capped``, the share of the elements whose bound is the cap, i.e.
    on which the comparison of the stepped parameters says no more than that both moved by at most lr."""
    import optim_step_ref as O
    sc = O.scalars(1, lr=lr, beta1=betas[0], beta2=betas[1], eps=eps)
    Pp, G = (_f64(p), 0.0), (_f64(g).reshape(np.shape(p)), _f64(eg).reshape(np.shape(p)))
    Z = (np.zeros_like(G[0]), 0.0)
    with np.errstate(all="ignore"):
        m1 = O._add(Z, O._mul(O._add(G, Z), O._c(sc.w1)))
        v1 = O._add(O._mul(Z, O._c(sc.b2)), O._mul(O._mul(O._c(sc.w2), G), G))
        den = O._add(O._div(O._sqrt(v1), O._c(sc.c2), False), O._c(sc.eps))
        r = O._div(m1, den, False)
        p1 = O._add(Pp, O._mul(O._c(-sc.ss), r))
        cap = 2.002 * lr + 4 * U * np.abs(Pp[0])
        ok = ((np.abs(den[0]) - den[1]) > 0) & np.isfinite(p1[1]) & (p1[1] >= 0)
        capped = ~ok | (p1[1] >= cap)
        if stats is not None:
            stats["capped"] = float(capped.mean())
        return np.where(capped, cap, p1[1])
