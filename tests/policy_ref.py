"""Host-only fp64 references of the fused policy kernels, with a per-element bound on the kernels' fp32 error.

Shared by tests/test_policy_ref_cpu.py (which shows that the bound admits other fp32 summation orders and rejects
plausible kernel mistakes) and the GPU tests of csrc/meshenv_policy.h (k_policy_forward, 12 instantiations) and
csrc/meshenv_actor.h (k_actor_forward, philox_normal).  Nothing here touches a device.

Every forward returns ``{name: (ref, bound)}``: ``ref`` the fp64 result computed from the same fp32 weights and inputs,
``bound`` an fp64 upper bound on ``|kernel - ref|`` for that element, derived from the kernel's arithmetic:

* A dense layer ``y = W x + b`` runs as ``v_mfma_f32_16x16x4_f32``, bit for bit a k-ordered ``fmaf`` chain (one rounding
  per step), over two accumulators (even / odd k-groups, K / 2 terms each), then ``acc0 + acc1``, then ``+ b``: the
  longest chain is m = K / 2 + 2 roundings, so ``|fl(W x + b) - (W x + b)| <= gamma_m (|W| |x| + |b|)`` with
  ``gamma_m = m u / (1 - m u)``, u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1).  K is the
  padded width (32 for the 18 observations).  An input error e_x propagates as ``|W| e_x`` and ``|x|`` is replaced by
  ``|x| + e_x``, which bounds the kernel's own activation.
* Activations pass the error on by the mean value theorem: ReLU as is where z >= 0 and only up to max(0, z + e) below
  (an output clipped either way carries none); tanh scaled by the largest slope 1 - tanh^2 on [z - e, z + e], plus
  ``tanhf``'s ulp allowance.
* Transcendentals: ULP below, in units of ulp(result) <= 2^-23 |result|.  The CUDA / HIP single-precision math tables
  document at most 2 ulp for expf, tanhf and sincosf and 1 ulp for logf; the allowance is 4 ulp for each (twice the
  largest).  sqrtf is correctly rounded under -fhip-fp32-correctly-rounded-divide-sqrt (the build's flag): 1 ulp allowed.
* Elementwise fp32 operations (the library is built with -ffp-contract=off, so no fusion) cost one u each, collected in
  gamma_k over the k operations on the path.
"""
from __future__ import annotations

import glob
import os

import numpy as np

U = 2.0 ** -24                  # unit roundoff of fp32
ULP_REL = 2.0 ** -23            # one ulp, relative to the result
ULP = dict(expf=4, logf=4, tanhf=4, sincosf=4, sqrtf=1)
LOG_SQRT_2PI = 0.91893853320467274178
LOG_SQRT_2PI_F32_ERR = abs(float(np.float32(LOG_SQRT_2PI)) - LOG_SQRT_2PI)   # the kernel's literal, rounded to fp32
TWO_PI_F32 = float(np.float32(6.2831853071795864))

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ACTION_LOW = np.array([-1.0, -1.5, 0.0], dtype=np.float32)     # vec_env.ACTION_LOW / HIGH (rl/boundary_env.py:27)
ACTION_HIGH = np.array([1.0, 1.5, 1.5], dtype=np.float32)

# the 12 instantiations of k_policy_forward: (kind, hidden, activation)
POLICY_CASES = [(kind, H, act) for kind in ("actor_critic", "deterministic") for H in (64, 128, 256) for act in ("relu", "tanh")]
LOG_STD = np.array([-5.0, -0.4, 1.5], dtype=np.float32)        # std 0.0067 .. 4.5
SIGMA = np.array([0.3, 0.0, 0.7], dtype=np.float32)            # one component without noise


def case_id(case):
    kind, H, act = case
    return f"{'ac' if kind == 'actor_critic' else 'det'}{H}-{act}"


def gamma(m):
    return m * U / (1.0 - m * U)


def _f64(a):
    return np.asarray(a, dtype=np.float64)


# ----------------------------------------------------------------------------------------------------------- inputs
def input_rows(n_real=5000):
    """The observation rows the tests feed the kernels, float32 [28 + n_real, 18]:
    18 basis rows (column k alone non-zero, k = 0..17: pins every input column), 2 zero rows, 8 saturating rows
    (magnitude 100: tanh layers reach exactly +-1, ReLU layers grow large), then n_real rows of real observations (the
    obs arrays of the recorded traces, angles in [-pi/2, 2 pi]).  Prefixes of it are the small-n inputs."""
    basis = np.zeros((18, 18), np.float32)
    for k in range(18):
        basis[k, k] = (1.0 + 0.25 * k) * (-1.0 if k % 2 else 1.0)
    zero = np.zeros((2, 18), np.float32)
    signs = np.random.default_rng(5).choice([-1.0, 1.0], size=(4, 18))
    sat = np.concatenate([np.full((1, 18), 100.0), np.full((1, 18), -100.0),
                          np.tile([100.0, -100.0], 9)[None], np.tile([-100.0, 100.0], 9)[None], 100.0 * signs]).astype(np.float32)
    real = []
    for f in sorted(glob.glob(os.path.join(GOLDEN_DIR, "*.npz"))):
        name = os.path.basename(f)
        if name.startswith(("quality_", "samples_", "front_", "plot_")):
            continue
        if name.startswith(("smooth_xf_", "smoothfront_xf_", "smoothfinal_xf_")):
            continue      # the smoothing records on transformed domains came later: the rows (and every recorded bit) stay
        z = np.load(f)
        if "obs" in z.files and z["obs"].ndim == 2 and z["obs"].shape[1] == 18:
            real.append(z["obs"].astype(np.float32))
    real = np.concatenate(real)
    real = real[np.random.default_rng(17).permutation(len(real))[:n_real]]
    # interleave a few real rows early so that small prefixes hold real observations too
    special = np.concatenate([basis, zero, sat])
    head = np.insert(special, [4, 9, 14, 20, 26], real[:5], axis=0)
    return np.ascontiguousarray(np.concatenate([head, real[5:]]))


def noise_rows(n, seed=3):
    """Explicit N(0, 1) noise [n, 3] float32, with a few large draws (|eps| up to 6)."""
    e = np.random.default_rng(seed).standard_normal((n, 3)).astype(np.float32)
    e.reshape(-1)[::37] *= 3.0
    return np.clip(e, -6.0, 6.0)


def policy_modules(case, seed=11, head_scale=1.0):
    """torch (CPU) modules of one instantiation with torch's default init: dict(pi=[Linear, Linear], vf=..., action_net,
    value_net, log_std) or dict(pi=..., mu, sigma).  head_scale multiplies the action head's weight (x6: actions reach the
    clamps)."""
    import torch
    kind, H, _ = case
    g = torch.random.fork_rng(devices=[])
    with g:
        torch.manual_seed(seed)
        tower = lambda: [torch.nn.Linear(18, H), torch.nn.Linear(H, H)]   # noqa: E731
        if kind == "actor_critic":
            m = dict(pi=tower(), vf=tower(), action_net=torch.nn.Linear(H, 3), value_net=torch.nn.Linear(H, 1),
                     log_std=torch.from_numpy(LOG_STD.copy()))
            head = m["action_net"]
        else:
            m = dict(pi=tower(), mu=torch.nn.Linear(H, 3), sigma=torch.from_numpy(SIGMA.copy()))
            head = m["mu"]
        with torch.no_grad():
            head.weight.mul_(head_scale)
    return m


def policy_spec(case, m):
    from reinforcementlearning4meshgeneration_amd.policy import PolicySpec
    kind, H, act = case
    if kind == "actor_critic":
        return PolicySpec.actor_critic(m["pi"], m["vf"], m["action_net"], m["value_net"], m["log_std"], activation=act)
    return PolicySpec.deterministic(m["pi"], m["mu"], activation=act, sigma=m["sigma"])


def actor_modules(seed=999, mu_scale=12.0):
    """SAC actor (3 x ReLU [128], mu and log_std heads), torch's default init; the log_std head's bias is +40 on component 0
    and -40 on component 2 (clamp(-20, 2) is hit both ways), the mu head is scaled so that tanh saturates."""
    import torch
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        lin = [torch.nn.Linear(18, 128), torch.nn.Linear(128, 128), torch.nn.Linear(128, 128)]
        mu, ls = torch.nn.Linear(128, 3), torch.nn.Linear(128, 3)
        with torch.no_grad():
            mu.weight.mul_(mu_scale)
            ls.bias[0] = 40.0
            ls.bias[2] = -40.0
    return lin, mu, ls


# ----------------------------------------------------------------------------------------------------------- layers
def _np32(t):
    return t.detach().cpu().numpy().astype(np.float32) if hasattr(t, "detach") else np.asarray(t, np.float32)


def spec_weights(spec):
    """{tower: [(W, b), (W, b), (Wh, bh)]} float32 from a PolicySpec."""
    w = spec.weights
    out = {"pi": [(w["pi_w1"], w["pi_b1"]), (w["pi_w2"], w["pi_b2"]), (w["pi_wh"], w["pi_bh"])]}
    if w.get("vf_w1") is not None:
        out["vf"] = [(w["vf_w1"], w["vf_b1"]), (w["vf_w2"], w["vf_b2"]), (w["vf_wh"], w["vf_bh"])]
    return out


def layer(x, ex, W, b, act, k_pad, rnd=None):
    """fp64 y = act(W x + b) and the bound on the kernel's y given a bound ex on its x.  k_pad: the K of the kernel's
    layer (inputs padded to a multiple of 16).  rnd: optional rounding applied to x and W (mutation tests)."""
    W64, b64 = _f64(W), _f64(b)
    if rnd is not None:
        x, W64 = rnd(x), rnd(W64)
    aW = np.abs(W64)
    z = x @ W64.T + b64
    ez = ex @ aW.T + gamma(k_pad // 2 + 2) * ((np.abs(x) + ex) @ aW.T + np.abs(b64))
    if act == "relu":
        return np.maximum(z, 0.0), relu_err(z, ez)
    if act == "tanh":
        return np.tanh(z), tanh_err(z, ez)
    return z, ez


def relu_err(z, ez):
    """|relu(z') - relu(z)| for |z' - z| <= ez: ez where z >= 0, max(0, z + ez) below (0 when both are clipped)."""
    return np.where(z >= 0, ez, np.maximum(0.0, z + ez))


def tanh_err(z, ez):
    """|tanhf(z') - tanh(z)| for |z' - z| <= ez: the mean value theorem (tanh' = 1 - tanh^2 is largest at the point of
    [z - ez, z + ez] nearest 0) plus tanhf's ulp allowance."""
    y = np.tanh(z)
    slope = 1.0 - np.tanh(np.maximum(0.0, np.abs(z) - ez)) ** 2
    return slope * ez + ULP["tanhf"] * ULP_REL * np.minimum(1.0, np.abs(y) + ez)


def tower(x, layers, act, H, rnd=None, swap_k2=None, bias_shift=None):
    """Two hidden layers and the head of one tower; returns (head output [n, n_out], its bound)."""
    (w1, b1), (w2, b2), (wh, bh) = layers
    if swap_k2 is not None:      # mutant: two k indices of layer 2 exchanged
        w2 = w2.copy(); w2[:, list(swap_k2)] = w2[:, list(swap_k2[::-1])]
    if bias_shift is not None:   # mutant: neuron n of one 16-neuron tile of layer 2 gets the bias of neuron n + 1
        b2 = b2.copy(); t0 = 16 * bias_shift; b2[t0:t0 + 16] = _f64(b2)[t0 + 1:t0 + 17]
    h, e = layer(x, np.zeros_like(x), w1, b1, act, 32, rnd)
    h, e = layer(h, e, w2, b2, act, H, rnd)
    return layer(h, e, wh, bh, None, H, rnd)


def _rescale(s, es, low, high):
    """action = low + 0.5 * (s + 1) * (high - low), four fp32 operations."""
    lo, hl = _f64(low), _f64(high) - _f64(low)
    a = lo + 0.5 * (s + 1.0) * hl
    return a, 0.5 * np.abs(hl) * es + gamma(4) * (np.abs(lo) + 0.5 * (np.abs(s) + es + 1.0) * np.abs(hl))


# ----------------------------------------------------------------------------------------------------------- policies
def policy_forward(spec, obs, eps=None, ba_kernel=None, mutant=None):
    """fp64 forward of a PolicySpec (k_policy_forward) on obs [n, 18] with noise eps [n, 3] (None: the deterministic launch,
    no noise drawn).  ba_kernel: the kernel's buffer_actions; log_prob is evaluated there (an error in ba is not counted
    twice).  mutant: name of a deliberate mistake (test_policy_ref_cpu.py)."""
    x = _f64(obs)
    n = x.shape[0]
    if mutant == "swap_in_16_17":
        x = x[:, [*range(16), 17, 16]]
    elif mutant == "drop_in_17":
        x = x.copy(); x[:, 17] = 0.0
    elif mutant == "shift_last_row":
        flat = np.concatenate([x.reshape(-1), [0.0]])
        x = x.copy(); x[-1] = flat[(n - 1) * 18 + 1:n * 18 + 1]
    rnd = tf32 if mutant == "tf32" else None
    swap = (1, 4) if mutant == "swap_k_layer2" else None
    shift = 1 if mutant == "bias_next_neuron" else None
    L = spec_weights(spec)
    H, act = spec.hidden, spec.activation
    low, high = _f64(spec.low), _f64(spec.high)
    mean, em = tower(x, L["pi"], act, H, rnd, swap, shift)
    noisy = eps is not None
    e = _f64(eps) if noisy else np.zeros((n, 3))
    out = {}
    if spec.kind == 0:
        ls = _f64(spec.weights["log_std_or_sigma"])
        std = np.exp(ls)
        r_e = ULP["expf"] * ULP_REL                       # expf(log_std) = std (1 + d), |d| <= r_e
        ba = mean + std * e
        eba = em + np.abs(e) * std * r_e + gamma(2) * (np.abs(mean) + em + std * (1 + r_e) * np.abs(e))
        act_ = np.clip(ba, low, high)
        out.update(mean=(mean, em), buffer_actions=(ba, eba), actions=(act_, eba))
        bak = ba if ba_kernel is None else _f64(ba_kernel)
        out["log_prob"] = _log_prob(bak, mean, em, std, r_e, mutant)
        v, ev = tower(x, L["vf"], act, H, rnd, swap, shift)
        v, ev = v[:, 0], ev[:, 0]
        if mutant == "value_col1":          # column 1 of the value tile: zero weights, zero bias
            v = np.zeros(n)
        out["value"] = (v, ev)
    else:
        sig = _f64(spec.weights["log_std_or_sigma"]) if spec.weights["log_std_or_sigma"] is not None else np.zeros(3)
        s, es = np.tanh(mean), tanh_err(mean, em)
        if noisy:
            es = es + gamma(2) * (np.abs(s) + es + sig * np.abs(e))
            s = s + sig * e
        out["unclipped"] = (s, es)
        s = np.clip(s, -1.0, 1.0)
        out.update(mean=(mean, em), buffer_actions=(s, es), actions=_rescale(s, es, low, high))
    return out


def _log_prob(ba, mean, em, std, r_e, mutant=None):
    """sum_c Normal(mean_c, std_c).log_prob(ba_c) and its bound; the kernel: d = ba - mean,
    lp_c = -(d * d) / (2 * (std * std)) - logf(std) - 0.9189385f, lp = (lp_0 + lp_1) + lp_2."""
    d = ba - mean
    ed = em + U * (np.abs(d) + em)
    var = std * std if mutant != "std_for_var" else std
    t = d * d / (2.0 * var)
    rho = (1 + U) ** 2 / ((1 - r_e) ** 2 * (1 - U)) - 1.0
    et = (2 * np.abs(d) * ed + ed * ed) / (2.0 * std * std) + rho * (np.abs(d) + ed) ** 2 / (2.0 * std * std)
    l = np.log(std)
    el = 1.01 * r_e + ULP["logf"] * ULP_REL * (np.abs(l) + 1.01 * r_e)
    lpc = -t - l - LOG_SQRT_2PI
    elc = et + el + LOG_SQRT_2PI_F32_ERR + gamma(2) * (np.abs(t) + et + np.abs(l) + el + LOG_SQRT_2PI)
    k = 2 if mutant == "lp_two_components" else 3
    lp = lpc[:, :k].sum(axis=1)
    elp = elc.sum(axis=1) + gamma(2) * (np.abs(lpc) + elc).sum(axis=1)
    return lp, elp


def actor_forward(lin, mu, ls, obs, eps=None, low=ACTION_LOW, high=ACTION_HIGH, mutant=None):
    """fp64 forward of the SAC actor (k_actor_forward): three ReLU layers, mu / log_std heads (one 16-wide tile),
    log_std clamped to [-20, 2]; with noise z = mu + exp(log_std) eps; action = rescale(tanh(z)).  Returns
    {"actions": (ref, bound), "mu": ..., "log_std": ...}."""
    x = _f64(obs)
    n = x.shape[0]
    if mutant == "swap_in_16_17":
        x = x[:, [*range(16), 17, 16]]
    elif mutant == "drop_in_17":
        x = x.copy(); x[:, 17] = 0.0
    elif mutant == "shift_last_row":
        flat = np.concatenate([x.reshape(-1), [0.0]])
        x = x.copy(); x[-1] = flat[(n - 1) * 18 + 1:n * 18 + 1]
    rnd = tf32 if mutant == "tf32" else None
    Ws = [(_np32(m.weight), _np32(m.bias)) for m in lin]
    if mutant == "swap_k_layer2":
        w = Ws[1][0].copy(); w[:, [1, 4]] = w[:, [4, 1]]; Ws[1] = (w, Ws[1][1])
    if mutant == "bias_next_neuron":
        b = _f64(Ws[1][1]).copy(); b[16:32] = _f64(Ws[1][1])[17:33]; Ws[1] = (Ws[1][0], b)
    h, e = layer(x, np.zeros_like(x), *Ws[0], "relu", 32, rnd)
    h, e = layer(h, e, *Ws[1], "relu", 128, rnd)
    h, e = layer(h, e, *Ws[2], "relu", 128, rnd)
    wh = np.concatenate([_np32(mu.weight), _np32(ls.weight)])
    bh = np.concatenate([_np32(mu.bias), _np32(ls.bias)])
    y, ey = layer(h, e, wh, bh, None, 128, rnd)
    m_, em = y[:, :3], ey[:, :3]
    raw, er = y[:, 3:], ey[:, 3:]
    lsc = np.clip(raw, -20.0, 2.0)
    elsc = np.where((raw - er >= 2.0) | (raw + er <= -20.0), 0.0, er)
    z, ez = m_, em
    if eps is not None:
        ep = _f64(eps)
        std = np.exp(lsc)
        es = std * np.expm1(elsc) + ULP["expf"] * ULP_REL * np.exp(lsc + elsc)
        z = m_ + std * ep
        ez = em + np.abs(ep) * es + gamma(2) * (np.abs(m_) + em + (std + es) * np.abs(ep))
    sq, esq = np.tanh(z), tanh_err(z, ez)
    return {"actions": _rescale(sq, esq, low, high), "mu": (m_, em), "log_std": (lsc, elsc)}


def tf32(a):
    """Round to TF32 (10 explicit mantissa bits, round to nearest even) -- what a reduced-precision matrix path would do."""
    f = np.asarray(a, np.float32).copy()
    i = f.view(np.uint32)
    i += np.uint32(0xFFF) + ((i >> np.uint32(13)) & np.uint32(1))
    i &= np.uint32(0xFFFFE000)
    return f.astype(np.float64)


# ----------------------------------------------------------------------------------------------------------- Philox
M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32(c0, c1, c2, c3, k0, k1, rounds=10):
    """Philox4x32-10 (Salmon et al., SC'11; Random123), vectorised over numpy arrays of uint32 words."""
    c = [np.asarray(v, np.uint64) & np.uint64(MASK) for v in (c0, c1, c2, c3)]
    c = np.broadcast_arrays(*c)
    c0, c1, c2, c3 = (v.copy() for v in c)
    k0, k1 = np.uint64(k0 & MASK), np.uint64(k1 & MASK)
    m = np.uint64(MASK)
    for _ in range(rounds):
        p0 = np.uint64(M0) * c0
        p1 = np.uint64(M1) * c2
        hi0, lo0 = p0 >> np.uint64(32), p0 & m
        hi1, lo1 = p1 >> np.uint64(32), p1 & m
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + np.uint64(W0)) & m, (k1 + np.uint64(W1)) & m
    return [v.astype(np.uint32) for v in (c0, c1, c2, c3)]


def philox_words(seed, counter, env, mutant=None):
    """The four words philox_normal draws for environment(s) env at (seed, counter):
    counter words (env, counter lo, counter hi, 0), key (seed lo, seed hi)."""
    env = np.asarray(env, np.uint64)
    clo, chi = counter & MASK, (counter >> 32) & MASK
    if mutant == "drop_counter_hi":
        chi = 0
    if mutant == "swap_env_counter":
        return philox4x32(np.full(env.shape, clo, np.uint64), env, chi, 0, seed & MASK, (seed >> 32) & MASK)
    return philox4x32(env, clo, chi, 0, seed & MASK, (seed >> 32) & MASK)


def _u01(w):
    """((float)(w >> 8) + 0.5f) * 2^-24 in fp32 arithmetic, exactly as the kernel rounds it."""
    return ((w >> np.uint32(8)).astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 16777216.0)


def philox_normal(seed, counter, env, mutant=None):
    """fp64 Box-Muller on the kernel's exact fp32 u1 / u2: eps [len(env), 3] and its bound.
    Component c uses words (r0, r1) for c < 2 (cos, sin) and (r2, r3) for c = 2 (cos).  The bound: logf and sqrtf relative
    errors on the radius; the angle fl(2pi_f * u2) differs from 2 pi u2 by |2pi_f - 2pi| u2 + u 2pi_f u2 (the fp32
    constant and the product's rounding; ~3e-6 of eps at |eps| = 6); sincosf's ulp allowance; the final product's u."""
    r = philox_words(seed, counter, env, mutant)
    eps, bnd = [], []
    for c in range(3):
        a, b = (r[0], r[1]) if (c < 2 or mutant == "comp2_words01") else (r[2], r[3])
        u1, u2 = _u01(a).astype(np.float64), _u01(b).astype(np.float64)
        rad = np.sqrt(-2.0 * np.log(u1))
        th = 2.0 * np.pi * u2
        sc = np.sin(th) if c == 1 else np.cos(th)
        r_rad = 0.5 * 1.01 * ULP["logf"] * ULP_REL + ULP["sqrtf"] * ULP_REL
        dth = abs(TWO_PI_F32 - 2.0 * np.pi) * u2 + U * TWO_PI_F32 * u2
        esc = dth + ULP["sincosf"] * ULP_REL * np.minimum(1.0, np.abs(sc) + dth)
        e = rad * sc
        eb = rad * (1 + r_rad) * esc + r_rad * rad * np.abs(sc) + U * rad * (1 + r_rad) * (np.abs(sc) + esc)
        eps.append(e); bnd.append(eb)
    return np.stack(eps, axis=1), np.stack(bnd, axis=1)


def philox_normal_f32(seed, counter, env):
    """An fp32 restatement of the kernel's Box-Muller (numpy float32 log / sqrt / cos / sin): must sit inside the bound."""
    r = philox_words(seed, counter, env)
    out = []
    for c in range(3):
        a, b = (r[0], r[1]) if c < 2 else (r[2], r[3])
        u1, u2 = _u01(a), _u01(b)
        rad = np.sqrt(np.float32(-2.0) * np.log(u1))
        th = np.float32(TWO_PI_F32) * u2
        out.append(rad * (np.sin(th) if c == 1 else np.cos(th)))
    return np.stack(out, axis=1).astype(np.float32)


# ----------------------------------------------------------------------------------------------------------- checks
def assert_clamped(actions, ba_ref_bound, low=ACTION_LOW, high=ACTION_HIGH):
    """Where the fp64 buffer action lies beyond a bound of the Box by more than its error bound, the kernel's clamped action
    is that bound exactly; everywhere the action lies inside the Box.  Returns the number of clamped elements."""
    ref, bound = ba_ref_bound
    a = _f64(actions)
    lo, hi = _f64(low), _f64(high)
    assert ((a >= lo) & (a <= hi)).all(), "action outside the Box"
    above, below = ref - bound > hi, ref + bound < lo
    assert (a[above] == np.broadcast_to(hi, a.shape)[above]).all(), "action not clamped to high exactly"
    assert (a[below] == np.broadcast_to(lo, a.shape)[below]).all(), "action not clamped to low exactly"
    return int(above.sum() + below.sum())


def check_clamps(out, ref, low=ACTION_LOW, high=ACTION_HIGH):
    """The clamps of a policy forward (dict of outputs, numpy or CUDA) against its fp64 reference: actor-critic actions
    are buffer_actions clamped to the Box; deterministic buffer_actions are clamped to [-1, 1] and map to low / high
    exactly at +-1.  Returns the number of elements the fp64 reference clamps beyond doubt."""
    out = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in out.items()}
    if "unclipped" not in ref:
        return assert_clamped(out["actions"], ref["buffer_actions"], low, high)
    ba = out["buffer_actions"]
    n = assert_clamped(ba, ref["unclipped"], -np.ones(3), np.ones(3))
    a = _f64(out["actions"])
    lo, hi = np.broadcast_to(_f64(low), a.shape), np.broadcast_to(_f64(high), a.shape)
    assert (a[ba == 1] == hi[ba == 1]).all() and (a[ba == -1] == lo[ba == -1]).all(), "tanh action at +-1 not at the Box bound"
    return n


def ratio(got, ref_bound):
    """max |got - ref| / bound (0 where both are 0, inf where got is not finite), and the mask of violations (NaN and
    inf included: a NaN difference compares false, so the mask is taken as "not within")."""
    ref, bound = ref_bound
    d = np.abs(_f64(got) - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(d == 0, 0.0, d / bound)
    r = np.where(np.isfinite(d), r, np.inf)
    return float(r.max()) if r.size else 0.0, ~(d <= bound)


def assert_within(got, ref_bound, what):
    r, bad = ratio(got, ref_bound)
    if bad.any():
        idx = np.argwhere(bad)[0]
        ref, bound = ref_bound
        raise AssertionError(f"{what}: {int(bad.sum())} elements outside the fp64 bound, first at {tuple(idx)}: "
                             f"got {_f64(got)[tuple(idx)]!r} ref {ref[tuple(idx)]!r} bound {bound[tuple(idx)]!r}")
    return r
