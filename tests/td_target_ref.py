"""Host-only fp64 restatement of the SAC / TD3 TD-target kernel (csrc/meshenv_target.h, k_td_target) with a per-element
bound on the kernel's fp32 error, by the rules at the top of tests/policy_ref.py (dense layers as two k-ordered fmaf
chains of K / 2 terms each, ReLU / tanh by the mean value theorem, 4 ulp for expf / logf / tanhf, one u per elementwise
fp32 operation).  Shared by tests/test_td_target_cpu.py and tests/test_gpu_td_target.py; nothing here touches a device.

``sac_target`` / ``td3_target`` return ``{name: (ref, bound)}`` for ``target`` [n], ``next_actions`` [n, 3],
``next_log_prob`` [n] (SAC), ``q1``, ``q2`` [n], all from the same fp32 weights and inputs the kernel reads.

The chain (SAC; the kernel's operations in order, each bound built from the one before):

  mean, log_std_raw   = the actor's head (policy_ref.layer: gamma_{K/2+2} per layer, errors passed through ReLU)
  log_std             = clamp(log_std_raw, -20, 2)        no error where the clamp holds beyond doubt
  std                 = expf(log_std)                     std (e^{e_ls} - 1) + 4 ulp
  g                   = mean + std * eps                  two roundings
  a                   = tanhf(g)                          slope (1 - tanh^2) on [g - e, g + e], + 4 ulp
  d                   = g - mean                          the kernel subtracts ITS mean from ITS g: the error of the mean
                                                          cancels; what is left is the error of std * eps and 3 roundings
  lpc_k               = -(d d) / (2 (std std)) - logf(std) - 0.9189385f       interval bound on the quotient, 4 ulp for logf
  sq_k                = logf((1 - a a) + 1e-6f)           SEE BELOW
  log_prob            = ((lpc_0 + lpc_1) + lpc_2) - ((sq_0 + sq_1) + sq_2)
  q_i                 = Q_i(cat(obs, a))                  layers again, input error (0, e_a)
  q                   = min(q_1, q_2)                     SEE BELOW
  q'                  = q - ent_coef * log_prob           ent_coef = expf(log_ent_coef) (4 ulp) or an exact fp32 constant
  target              = reward + ((1 - done) * gamma) * q'

``log(1 - a^2 + 1e-6)`` near |a| -> 1.  The argument is w = 1 - a^2 + 1e-6 >= 1e-6.  The kernel's argument differs from it
by e_w = 2 |a| e_a + e_a^2 (the error of a: at least tanhf's 4 ulp = 4.8e-7 at |a| = 1) + u (|a| + e_a)^2 (the product) +
u |1 - a a| (the subtraction) + |fl(1e-6) - 1e-6| + u w (the sum).  That ABSOLUTE error is divided by w: at |a| = 1,
e_w ~ 1e-6 ~ w and the relative error of the argument is of order 1.  The kernel's argument cannot fall below fl(1e-6f),
because |tanhf| <= 1 makes fl(1 - a a) >= 0; so the bound is the width of the interval
[log(max(w - e_w, fl(1e-6f))), log(w + e_w)] about log(w) -- at most log(3) ~ 1.1 at saturation, ~2 e_a / (1 - a^2)
elsewhere -- plus logf's 4 ulp.  This is fp32's doing, not the kernel's: eager torch computes the same expression and
shares it.  test_td_target_cpu.py checks that on the default-init case the loose region is small (the tightness condition).

``min(q1, q2)``.  |min(a', b') - min(a, b)| <= max(|a' - a|, |b' - b|) (min is 1-Lipschitz in the max norm; the kernel may
pick the other critic when the two are within their bounds of each other, and then its value still lies within the larger
bound of the reference's), so the bound of q is max(e_q1, e_q2), not their sum and not the bound of the smaller one.

TD3: a = clamp(tanhf(mu) + clamp(policy_noise * eps, -noise_clip, noise_clip), -1, 1): one rounding for the product, one
for the sum; both clamps are 1-Lipschitz.  The rest as above without the entropy term.
"""
from __future__ import annotations

import numpy as np

import policy_ref as R
from policy_ref import ULP, ULP_REL, U, _f64, _np32, gamma, layer, tanh_err

EPS6 = 1e-6
EPS6_F32 = float(np.float32(1e-6))
PHILOX_TAG = 2                     # k_td_target's own stream (rollout noise 0, replay draw 1)
MUTANTS = ("max_for_min", "drop_not_done", "drop_entropy", "drop_1e-6", "cat_action_obs", "box_action", "no_log_std_clamp",
           "td3_no_noise_clip", "td3_no_action_clamp", "gamma_on_reward")


# ----------------------------------------------------------------------------------------------------------- inputs
def batch_rows(n, seed=23, reward_scale=1.0, done_p=0.2):
    """rewards, dones float32 [n]: rewards uniform in [-reward_scale, reward_scale] (a few exact zeros), dones 0 / 1."""
    rng = np.random.default_rng(seed)
    rew = (rng.uniform(-1.0, 1.0, n) * reward_scale).astype(np.float32)
    rew[::41] = 0.0
    done = (rng.random(n) < done_p).astype(np.float32)
    return rew, done


def tight_rows(obs, l1_max=12.0):
    """Mask of the rows of the tightness condition (test_td_target_cpu.py): observations with sum_k |obs_k| <= 12, the
    smaller half of input_rows().  The a-priori bound of a dense layer is gamma_m |W| |x|, linear in the size of the input
    row; through the eight layers of actor and critic it reaches 7.6e-4 at the median of ALL rows (correlation with
    sum |obs_k|: 0.96) before the log term adds anything, so on all rows only 76 % of the targets meet
    bound <= 1e-3 max(1, |ref|) and the condition would measure the layer bound, not the log term it is there to watch."""
    return np.abs(_f64(obs)).sum(axis=1) <= l1_max


def _critic_modules(H, nl):
    import torch
    dims = [21] + [H] * nl
    return [torch.nn.Linear(dims[i], dims[i + 1]) for i in range(nl)] + [torch.nn.Linear(H, 1)]


def sac_modules(seed=41, stress=False):
    """dict(kind, lin, mu, ls, q1, q2) of torch (CPU) Linear layers with torch's default init.  stress: the actor of
    policy_ref.actor_modules with the action head x 6 (tanh saturates) and the log_std head's bias +40 / -40 (both clamps)."""
    import torch
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        if stress:
            lin, mu, ls = R.actor_modules(seed=seed, mu_scale=6.0)
        else:
            lin = [torch.nn.Linear(18, 128), torch.nn.Linear(128, 128), torch.nn.Linear(128, 128)]
            mu, ls = torch.nn.Linear(128, 3), torch.nn.Linear(128, 3)
        torch.manual_seed(seed + 1)
        q1, q2 = _critic_modules(128, 3), _critic_modules(128, 3)
    return dict(kind="sac", lin=lin, mu=mu, ls=ls, q1=q1, q2=q2)


def td3_modules(seed=43, head_scale=1.0):
    import torch
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        lin, mu = [torch.nn.Linear(18, 256), torch.nn.Linear(256, 256)], torch.nn.Linear(256, 3)
        q1, q2 = _critic_modules(256, 2), _critic_modules(256, 2)
        with torch.no_grad():
            mu.weight.mul_(head_scale)
    return dict(kind="td3", lin=lin, mu=mu, q1=q1, q2=q2)


def layers_of(mods):
    return [(_np32(m.weight), _np32(m.bias)) for m in mods]


# ----------------------------------------------------------------------------------------------------------- pieces
def mlp(x, ex, layers, H):
    """ReLU layers then a linear head; layers [(W, b), ...]; returns (head [n, n_out], bound)."""
    h, e = x, ex
    for i, (W, b) in enumerate(layers[:-1]):
        h, e = layer(h, e, W, b, "relu", 32 if i == 0 else H)
    return layer(h, e, *layers[-1], None, H)


def _critics(m, obs, a, ea, H, mutant):
    x = _f64(obs)
    if mutant == "box_action":
        lo, hi = _f64(R.ACTION_LOW), _f64(R.ACTION_HIGH)
        a = lo + 0.5 * (a + 1.0) * (hi - lo)
    xin = np.concatenate([a, x], axis=1) if mutant == "cat_action_obs" else np.concatenate([x, a], axis=1)
    exin = np.concatenate([np.zeros_like(x), ea], axis=1)
    if mutant == "cat_action_obs":
        exin = np.concatenate([ea, np.zeros_like(x)], axis=1)
    q1, e1 = mlp(xin, exin, layers_of(m["q1"]), H)
    q2, e2 = mlp(xin, exin, layers_of(m["q2"]), H)
    return (q1[:, 0], e1[:, 0]), (q2[:, 0], e2[:, 0])


def _finish(out, q1, q2, lp, ent, rewards, dones, gamma_, mutant):
    """min, entropy term and the Bellman step; lp / ent: (value, bound) or None."""
    (v1, e1), (v2, e2) = q1, q2
    q = np.maximum(v1, v2) if mutant == "max_for_min" else np.minimum(v1, v2)
    eq = np.maximum(e1, e2)
    if lp is not None and mutant != "drop_entropy":
        (l, el), (c, ec) = lp, ent
        q, eq = q - c * l, eq + np.abs(l) * ec + (c + ec) * el + gamma(2) * (np.abs(q) + eq + (abs(c) + ec) * (np.abs(l) + el))
    r, d = _f64(rewards).reshape(-1), _f64(dones).reshape(-1)
    g = float(np.float32(gamma_))
    nd = np.ones_like(d) if mutant == "drop_not_done" else 1.0 - d
    z = nd * g * q
    ez = np.abs(nd * g) * eq + gamma(3) * np.abs(nd * g) * (np.abs(q) + eq)
    t = (r + nd * q) * g if mutant == "gamma_on_reward" else r + z
    out.update(q1=q1, q2=q2, target=(t, ez + U * (np.abs(r) + np.abs(z) + ez)))
    return out


# ----------------------------------------------------------------------------------------------------------- SAC
def sac_target(m, obs, rewards, dones, eps=None, gamma_=0.99, log_ent_coef=None, ent_coef=None, mutant=None):
    """eps None: the launch without noise (eps = 0).  Exactly one of log_ent_coef (fp32 scalar, the kernel takes expf) and
    ent_coef (a host float, rounded to fp32) is given."""
    x = _f64(obs)
    n = x.shape[0]
    wh = np.concatenate([_np32(m["mu"].weight), _np32(m["ls"].weight)])
    bh = np.concatenate([_np32(m["mu"].bias), _np32(m["ls"].bias)])
    y, ey = mlp(x, np.zeros_like(x), layers_of(m["lin"]) + [(wh, bh)], 128)
    mean, em, raw, er = y[:, :3], ey[:, :3], y[:, 3:], ey[:, 3:]
    if mutant == "no_log_std_clamp":
        ls, els = raw, er
    else:
        ls = np.clip(raw, -20.0, 2.0)
        els = np.where((raw - er >= 2.0) | (raw + er <= -20.0), 0.0, er)
    ep = _f64(eps) if eps is not None else np.zeros((n, 3))
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        std = np.exp(ls)
        es = std * np.expm1(els) + ULP["expf"] * ULP_REL * np.exp(ls + els)
        g = mean + std * ep
        eg = em + np.abs(ep) * es + gamma(2) * (np.abs(mean) + em + (std + es) * np.abs(ep))
        a, ea = np.tanh(g), tanh_err(g, eg)
        # Normal(mean, std).log_prob(g) as the kernel evaluates it
        d = std * ep
        ed = np.abs(ep) * es + gamma(3) * (np.abs(mean) + em + (std + es) * np.abs(ep))
        t = d * d / (2.0 * std * std)
        s_lo, s_hi = np.maximum(std - es, 0.5 * std), std + es
        t_hi = (np.abs(d) + ed) ** 2 / (2.0 * s_lo * s_lo) * (1.0 + gamma(3))
        t_lo = np.maximum(np.abs(d) - ed, 0.0) ** 2 / (2.0 * s_hi * s_hi) * (1.0 - gamma(3))
        et = np.maximum(t_hi - t, t - t_lo)
        l = np.log(std)
        dl = -np.log1p(-np.minimum(es / std, 0.5))
        el = dl + ULP["logf"] * ULP_REL * (np.abs(l) + dl)
        lpc = -t - l - R.LOG_SQRT_2PI
        elc = et + el + R.LOG_SQRT_2PI_F32_ERR + gamma(2) * (np.abs(t) + et + np.abs(l) + el + R.LOG_SQRT_2PI)
        # log((1 - a a) + 1e-6f): the docstring's interval bound
        e6 = 0.0 if mutant == "drop_1e-6" else EPS6
        w = 1.0 - a * a + e6
        ew = 2.0 * np.abs(a) * ea + ea * ea + U * (np.abs(a) + ea) ** 2 + U * np.abs(1.0 - a * a) + abs(EPS6_F32 - EPS6) + U * w
        sq = np.log(w)
        esq = np.maximum(np.log(w + ew) - sq, sq - np.log(np.maximum(w - ew, EPS6_F32)))
        esq = esq + ULP["logf"] * ULP_REL * (np.abs(sq) + esq)
        lp = lpc.sum(axis=1) - sq.sum(axis=1)
        elp = elc.sum(axis=1) + esq.sum(axis=1) + gamma(3) * ((np.abs(lpc) + elc).sum(axis=1) + (np.abs(sq) + esq).sum(axis=1))
    if (log_ent_coef is None) == (ent_coef is None):
        raise ValueError("exactly one of log_ent_coef and ent_coef")
    if log_ent_coef is not None:
        c = float(np.exp(np.float64(np.float32(log_ent_coef))))
        ent = (c, ULP["expf"] * ULP_REL * c)
    else:
        ent = (float(np.float32(ent_coef)), 0.0)
    out = {"next_actions": (a, ea), "next_log_prob": (lp, elp), "log_std": (ls, els), "gaussian": (g, eg)}
    q1, q2 = _critics(m, obs, a, ea, 128, mutant)
    return _finish(out, q1, q2, (lp, elp), ent, rewards, dones, gamma_, mutant)


# ----------------------------------------------------------------------------------------------------------- TD3
def td3_target(m, obs, rewards, dones, eps=None, gamma_=0.99, policy_noise=0.2, noise_clip=0.5, mutant=None):
    x = _f64(obs)
    n = x.shape[0]
    mean, em = mlp(x, np.zeros_like(x), layers_of(m["lin"]) + [(_np32(m["mu"].weight), _np32(m["mu"].bias))], 256)
    s, es = np.tanh(mean), tanh_err(mean, em)
    ep = _f64(eps) if eps is not None else np.zeros((n, 3))
    pn, nc = float(np.float32(policy_noise)), float(np.float32(noise_clip))
    nz = pn * ep
    enz = U * np.abs(nz)
    if mutant != "td3_no_noise_clip":
        nz = np.clip(nz, -nc, nc)
    un = s + nz
    ea = es + enz + U * (np.abs(s) + es + np.abs(nz) + enz)
    a = un if mutant == "td3_no_action_clamp" else np.clip(un, -1.0, 1.0)
    out = {"next_actions": (a, ea), "unclipped": (un, ea)}
    q1, q2 = _critics(m, obs, a, ea, 256, mutant)
    return _finish(out, q1, q2, None, None, rewards, dones, gamma_, mutant)


def target_ref(m, obs, rewards, dones, eps=None, mutant=None, **kw):
    return (sac_target if m["kind"] == "sac" else td3_target)(m, obs, rewards, dones, eps, mutant=mutant, **kw)


# ----------------------------------------------------------------------------------------------------------- Philox
def philox_normal(seed, counter, idx):
    """fp64 Box-Muller on the kernel's fp32 uniforms for samples idx at (seed, counter), counter words (idx, counter lo,
    counter hi, 2): eps [len(idx), 3] and its bound (policy_ref.philox_normal's derivation, with the tag of this kernel)."""
    return _normal(R.philox4x32(np.asarray(idx, np.uint64), counter & R.MASK, (counter >> 32) & R.MASK, PHILOX_TAG,
                                seed & R.MASK, (seed >> 32) & R.MASK))


def philox_words(seed, counter, idx, tag):
    return R.philox4x32(np.asarray(idx, np.uint64), counter & R.MASK, (counter >> 32) & R.MASK, tag, seed & R.MASK,
                        (seed >> 32) & R.MASK)


def _normal(r):
    eps, bnd = [], []
    for c in range(3):
        a, b = (r[0], r[1]) if c < 2 else (r[2], r[3])
        u1, u2 = R._u01(a).astype(np.float64), R._u01(b).astype(np.float64)
        rad = np.sqrt(-2.0 * np.log(u1))
        th = 2.0 * np.pi * u2
        sc = np.sin(th) if c == 1 else np.cos(th)
        r_rad = 0.5 * 1.01 * ULP["logf"] * ULP_REL + ULP["sqrtf"] * ULP_REL
        dth = abs(R.TWO_PI_F32 - 2.0 * np.pi) * u2 + U * R.TWO_PI_F32 * u2
        esc = dth + ULP["sincosf"] * ULP_REL * np.minimum(1.0, np.abs(sc) + dth)
        eps.append(rad * sc)
        bnd.append(rad * (1 + r_rad) * esc + r_rad * rad * np.abs(sc) + U * rad * (1 + r_rad) * (np.abs(sc) + esc))
    return np.stack(eps, axis=1), np.stack(bnd, axis=1)


# ----------------------------------------------------------------------------------------------------------- fp32 restatement
def _dense32(x, W, b, chunk=64):
    """float32 y = W x + b with numpy's pairwise summation over k (another order than the kernel's two chains)."""
    W, b = np.asarray(W, np.float32), np.asarray(b, np.float32)
    out = np.empty((x.shape[0], W.shape[0]), np.float32)
    for i in range(0, x.shape[0], chunk):
        out[i:i + chunk] = (x[i:i + chunk, None, :] * W[None]).sum(axis=2, dtype=np.float32) + b
    return out


def _mlp32(x, layers):
    h = x
    for W, b in layers[:-1]:
        h = np.maximum(_dense32(h, W, b), np.float32(0))
    return _dense32(h, *layers[-1])


def target_f32(m, obs, rewards, dones, eps=None, gamma_=0.99, log_ent_coef=None, ent_coef=None, policy_noise=0.2,
               noise_clip=0.5):
    """The whole block in numpy float32, every operation rounded to fp32, dense layers summed pairwise: a second fp32
    evaluation that must sit inside the bound.  Returns dict of float32 arrays."""
    f = np.float32
    x = np.asarray(obs, f)
    n = x.shape[0]
    ep = np.asarray(eps, f) if eps is not None else np.zeros((n, 3), f)
    r, d = np.asarray(rewards, f).reshape(-1), np.asarray(dones, f).reshape(-1)
    out = {}
    if m["kind"] == "sac":
        wh = np.concatenate([_np32(m["mu"].weight), _np32(m["ls"].weight)])
        bh = np.concatenate([_np32(m["mu"].bias), _np32(m["ls"].bias)])
        y = _mlp32(x, layers_of(m["lin"]) + [(wh, bh)])
        mean, ls = y[:, :3], np.clip(y[:, 3:], f(-20), f(2))
        std = np.exp(ls)
        g = mean + std * ep
        a = np.tanh(g)
        dd = g - mean
        lpc = -(dd * dd) / (f(2) * (std * std)) - np.log(std) - f(R.LOG_SQRT_2PI)
        sq = np.log((f(1) - a * a) + f(1e-6))
        lp = ((lpc[:, 0] + lpc[:, 1]) + lpc[:, 2]) - ((sq[:, 0] + sq[:, 1]) + sq[:, 2])
        out["next_log_prob"] = lp
    else:
        mean = _mlp32(x, layers_of(m["lin"]) + [(_np32(m["mu"].weight), _np32(m["mu"].bias))])
        nz = np.clip(f(policy_noise) * ep, -f(noise_clip), f(noise_clip))
        a = np.clip(np.tanh(mean) + nz, f(-1), f(1))
    xin = np.concatenate([x, a], axis=1)
    q1, q2 = _mlp32(xin, layers_of(m["q1"]))[:, 0], _mlp32(xin, layers_of(m["q2"]))[:, 0]
    q = np.minimum(q1, q2)
    if m["kind"] == "sac":
        c = np.exp(f(log_ent_coef)) if log_ent_coef is not None else f(ent_coef)
        q = q - c * out["next_log_prob"]
    out.update(next_actions=a, q1=q1, q2=q2, target=r + ((f(1) - d) * f(gamma_)) * q)
    return out


OUTPUTS = ("target", "next_actions", "next_log_prob", "q1", "q2")


def assert_all_within(got, ref, what, worst=None):
    """Every output present in both within its bound; worst: dict of the largest ratio per output, updated."""
    for k in OUTPUTS:
        if k in got and k in ref:
            v = got[k]
            v = v.cpu().numpy() if hasattr(v, "cpu") else v
            r = R.assert_within(np.asarray(v).reshape(ref[k][0].shape), ref[k], f"{what} {k}")
            if worst is not None:
                worst[k] = max(worst.get(k, 0.0), r)
