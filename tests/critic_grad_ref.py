"""Host-only fp64 restatement of the critic-loss kernel (csrc/meshenv_critic_grad.h: k_critic_grad, k_critic_grad_reduce)
with manual backpropagation and a per-element bound on the kernel's fp32 error, by the rules at the top of
tests/policy_ref.py.  Shared by tests/test_critic_grad_cpu.py and tests/test_gpu_critic_grad.py; nothing here touches a
device.

``critic_grad(m, obs, actions, y)`` returns ``({name: (ref, bound)}, info)`` for ``loss``, ``q1``, ``q2`` and every gradient
tensor ``q{c}.w{i}`` / ``q{c}.b{i}`` (c = 1, 2; i = 0 .. NL - 1 the hidden layers, i = NL the output layer; torch's
[out][in] / [out] shapes), of SB3's

    critic_loss = 0.5 * sum(F.mse_loss(q, y) for q in critic(obs, actions));  zero_grad(); critic_loss.backward()

The chain, in the kernel's order, each bound built from the one before (u = 2^-24, gamma_m = m u / (1 - m u)):

  a_l, q     policy_ref.layer (two fma chains of K / 2 terms, + combine, + bias: gamma_{K/2+2}; ReLU by relu_err)
  d          = q - y                     one rounding:   e_d = e_q + u (|d| + e_q)
  dq         = d / B                     correctly rounded division: e_dq = (e_d + u (|d| + e_d)) / B
  d2         = d * d                     e_d2 = 2 |d| e_d + e_d^2 + u (|d| + e_d)^2
  loss       = 0.5 (S_1 / B + S_2 / B), S_c the batch sum of d2 (below): one u per division and for the sum; 0.5 is exact
  dz_L       = mask_L * (dq * w_out)     one rounding
  dW_l       = dz_l^T a_{l-1},  db_l = sum_rows dz_l        BATCH SUMS (below); term errors e_dz (|a| + e_a) + |dz| e_a
  da_{l-1}   = dz_l W_l                  two fma chains of H / 2 terms and their sum: gamma_{H/2+1}; input error e_dz |W|
  dz_{l-1}   = mask_{l-1} * da_{l-1}     a select: exact

Batch sums -- the kernel's actual reduction order.  With tiles = ceil(B / 16), the launch has nwg = min(tiles, 64)
workgroups per critic up to 512 tiles and 128 beyond; workgroup g owns tiles g, g + nwg, ... (at most T = ceil(tiles / nwg))
and adds every row of them to ONE accumulator by fused multiply-add (v_mfma_f32_16x16x4_f32 for dW and db, fmaf for the
output layer's weight, a plain add for its bias and for S_c: one rounding per row either way), 16 T roundings; the partial
results of the workgroups are then added in index order, nwg - 1 roundings.  The longest path has m = 16 T + nwg - 1
roundings, so |fl(sum) - sum| <= gamma_m sum |terms|, with |terms| taken at |x| + e_x.  Rows past B contribute exactly 0.
(B = 100: m = 22; 256: 31; 4096: 127; 4101: 143; 65536: 639.)

ReLU masks.  A (sample, neuron) pair is AMBIGUOUS when |z_ref| <= e_z, the forward bound of its pre-activation: fp32 may
land on either side of 0 there and either mask is a correct fp32 evaluation.  The reference backpropagates with its own
mask (z_ref > 0; torch's ReLU gradient is 0 at z = 0) except on ambiguous pairs, where it takes the mask of the evaluation it
is compared with (``other_acts``: the kernel's returned activations on the GPU, the second fp32 evaluation's on the CPU).
``info`` carries the ambiguous pairs, the reference masks and the ambiguous share, which the tests cap at 2e-4 BEFORE
anything is compared.
"""
from __future__ import annotations

import numpy as np

import policy_ref as R
import td_target_ref as T
from policy_ref import U, _f64, gamma, layer, relu_err

MAX_AMBIGUOUS_SHARE = 2e-4
MUTANTS = ("sum_for_mean", "drop_half", "mask_from_above", "dw_transposed", "da_other_critic", "cat_action_obs",
           "target_sign", "tail_rows", "db_zero", "q2_copy_of_q1")


def reduction_roundings(B):
    """m of the docstring: roundings on the longest path of a batch sum of k_critic_grad + k_critic_grad_reduce."""
    tiles = (B + 15) // 16
    nwg = min(tiles, 64) if tiles <= 512 else 128
    return 16 * ((tiles + nwg - 1) // nwg) + nwg - 1


# ----------------------------------------------------------------------------------------------------------- inputs
def critic_modules(kind, seed=None, stress=False):
    """dict(kind, q1, q2): the twin critics of td_target_ref.sac_modules / td3_modules (torch default init).  stress: the
    first layer's weights x 6 (large pre-activations, many neurons clipped)."""
    import torch
    m = T.sac_modules(**({} if seed is None else {"seed": seed})) if kind == "sac" else T.td3_modules(**({} if seed is None else {"seed": seed}))
    m = dict(kind=kind, q1=m["q1"], q2=m["q2"])
    if stress:
        with torch.no_grad():
            m["q1"][0].weight.mul_(6.0)
            m["q2"][0].weight.mul_(6.0)
    return m


def batch(B, obs_rows, seed=29, target_scale=1.0):
    """observations [B, 18] (a prefix of policy_ref.input_rows(), repeated beyond its length), uniform actions in [-1, 1]
    [B, 3], targets [B] uniform in [-target_scale, target_scale]; float32."""
    rng = np.random.default_rng(seed + B)
    obs = np.ascontiguousarray(np.resize(obs_rows, (B, 18)).astype(np.float32))
    act = rng.uniform(-1.0, 1.0, (B, 3)).astype(np.float32)
    y = (rng.uniform(-1.0, 1.0, B) * target_scale).astype(np.float32)
    return obs, act, y


def names(nl):
    """Gradient names of one critic in the order of its parameters (CriticGradSpec.q1): w0 b0 ... w{nl} b{nl}."""
    return [f"{p}{i}" for i in range(nl + 1) for p in ("w", "b")]


# ----------------------------------------------------------------------------------------------------------- pieces
def _bsum(A, eA, Bm, eB, m):
    """sum_rows A[r][i] B[r][j] as the kernel's batch sum: (ref [i][j], bound)."""
    aA, aB = np.abs(A), np.abs(Bm)
    ref = A.T @ Bm
    err = eA.T @ (aB + eB) + aA.T @ eB
    return ref, err + gamma(m) * ((aA + eA).T @ (aB + eB))


def _forward(layers, x, H):
    """[(z, ez, a, ea)] per hidden layer and (q, eq) [B]."""
    hid, h, e = [], x, np.zeros_like(x)
    for i, (W, b) in enumerate(layers[:-1]):
        z, ez = layer(h, e, W, b, None, 32 if i == 0 else H)
        h, e = np.maximum(z, 0.0), relu_err(z, ez)
        hid.append((z, ez, h, e))
    q, eq = layer(h, e, *layers[-1], None, H)
    return hid, (q[:, 0], eq[:, 0])


def _one_critic(layers, other_layers, x, y, B, m, H, other_acts, mutant):
    nl = len(layers) - 1
    hid, (q, eq) = _forward(layers, x, H)
    info = dict(ambiguous=[], mask=[])
    masks = []
    for l, (z, ez, _, _) in enumerate(hid):
        amb, mk = np.abs(z) <= ez, z > 0
        info["ambiguous"].append(amb)
        info["mask"].append(mk)
        if other_acts is not None:
            mk = np.where(amb, np.asarray(other_acts[l])[:len(z)] > 0, mk)
        masks.append(mk.astype(np.float64))
    d = q + y if mutant == "target_sign" else q - y
    e_d = eq + U * (np.abs(d) + eq)
    div = 1.0 if mutant == "sum_for_mean" else float(B)
    dq, e_dq = d / div, (e_d + U * (np.abs(d) + e_d)) / div
    d2 = d * d
    e_d2 = 2.0 * np.abs(d) * e_d + e_d * e_d + U * (np.abs(d) + e_d) ** 2
    S, eS = d2.sum(), e_d2.sum() + gamma(m) * (d2 + e_d2).sum()
    lc, elc = S / div, eS / div + U * (S + eS) / div
    out = {}
    acts = [(x, np.zeros_like(x))] + [(a, ea) for (_, _, a, ea) in hid]
    wh = _f64(layers[-1][0])[0]
    a_last, ea_last = acts[-1]
    out[f"w{nl}"] = _bsum(dq[:, None], e_dq[:, None], a_last, ea_last, m)          # [1][H]
    out[f"b{nl}"] = (np.array([dq.sum()]), np.array([e_dq.sum() + gamma(m) * (np.abs(dq) + e_dq).sum()]))
    dz = masks[-1] * (dq[:, None] * wh[None])
    edz = masks[-1] * (e_dq[:, None] * np.abs(wh)[None] + U * (np.abs(dq) + e_dq)[:, None] * np.abs(wh)[None])
    for l in range(nl - 1, -1, -1):              # hidden layer l: dz is dz_l, its input a_l = acts[l]
        a_prev, ea_prev = acts[l]
        w, ew = _bsum(dz, edz, a_prev, ea_prev, m)
        if mutant == "dw_transposed" and w.shape[0] == w.shape[1]:
            w = w.T
        out[f"w{l}"] = (w, ew)
        out[f"b{l}"] = (dz.sum(axis=0), edz.sum(axis=0) + gamma(m) * (np.abs(dz) + edz).sum(axis=0))
        if l == 0:
            break
        W = _f64((other_layers if mutant == "da_other_critic" else layers)[l][0])
        da = dz @ W
        eda = edz @ np.abs(W) + gamma(H // 2 + 1) * ((np.abs(dz) + edz) @ np.abs(W))
        mk = masks[l] if mutant == "mask_from_above" else masks[l - 1]
        dz, edz = mk * da, mk * eda
    if mutant == "db_zero":
        for k in out:
            if k.startswith("b"):
                out[k] = (np.zeros_like(out[k][0]), out[k][1])
    return out, (q, eq), (lc, elc), info


def critic_grad(m, obs, actions, y, other_acts=None, mutant=None):
    """other_acts: {1: [a_0 .. a_{NL-1}], 2: [...]} post-ReLU activations [B, H] of the evaluation this reference is
    compared with (its mask is taken on the ambiguous pairs), or None (the reference's own mask everywhere)."""
    H = 128 if m["kind"] == "sac" else 256
    o, a, yy = _f64(obs), _f64(actions), _f64(y).reshape(-1)
    B = o.shape[0]
    x = np.concatenate([a, o], axis=1) if mutant == "cat_action_obs" else np.concatenate([o, a], axis=1)
    if mutant == "tail_rows":      # the rows of the last tile past B treated as samples (zero input, zero target)
        pad = (-B) % 16
        x, yy = np.concatenate([x, np.zeros((pad, 21))]), np.concatenate([yy, np.zeros(pad)])
        if other_acts is not None:
            other_acts = {c: [np.concatenate([np.asarray(v), np.zeros((pad, H))]) for v in vs] for c, vs in other_acts.items()}
    mm = reduction_roundings(B)
    L1, L2 = T.layers_of(m["q1"]), T.layers_of(m["q2"])
    out, info, losses = {}, {}, []
    for c, (own, other) in ((1, (L1, L2)), (2, (L2, L1))):
        g, q, lc, inf = _one_critic(own, other, x, yy, B, mm, H, None if other_acts is None else other_acts[c], mutant)
        out[f"q{c}"] = (q[0][:B], q[1][:B])
        for k, v in g.items():
            out[f"q{c}.{k}"] = v
        info[c] = inf
        losses.append(lc)
    if mutant == "q2_copy_of_q1":
        for k in list(out):
            if k.startswith("q2."):
                out[k] = (out["q1." + k[3:]][0], out[k][1])
    (l1, e1), (l2, e2) = losses
    half = 1.0 if mutant == "drop_half" else 0.5
    out["loss"] = (np.array(half * (l1 + l2)), np.array(half * (e1 + e2 + U * (abs(l1) + abs(l2) + e1 + e2))))
    if mutant == "drop_half":
        for k in out:
            if "." in k:
                out[k] = (2.0 * out[k][0], out[k][1])
    n_amb = sum(int(a_.sum()) for c in (1, 2) for a_ in info[c]["ambiguous"])
    n_all = sum(a_.size for c in (1, 2) for a_ in info[c]["ambiguous"])
    info["ambiguous_pairs"], info["ambiguous_share"] = n_amb, n_amb / n_all
    return out, info


def assert_share(info, what):
    """The condition on the test case: stated from the reference alone, before any comparison."""
    assert info["ambiguous_share"] <= MAX_AMBIGUOUS_SHARE, \
        f"{what}: {info['ambiguous_pairs']} ambiguous (sample, neuron) pairs, share {info['ambiguous_share']:.2e} > {MAX_AMBIGUOUS_SHARE}"


def assert_masks(info, acts, what):
    """Off the ambiguous pairs the compared evaluation's mask equals the reference's."""
    for c in (1, 2):
        for l, (amb, mk) in enumerate(zip(info[c]["ambiguous"], info[c]["mask"])):
            got = np.asarray(acts[c][l]) > 0
            bad = (got != mk) & ~amb
            assert not bad.any(), f"{what}: critic {c} layer {l}: {int(bad.sum())} masks differ off the ambiguous pairs, first {tuple(np.argwhere(bad)[0])}"


def assert_all_within(got, ref, what, worst=None):
    """Every output of ref within its bound (got: name -> array); worst: dict of the largest ratio per output, updated."""
    for k, rb in ref.items():
        v = got[k]
        v = v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)
        r = R.assert_within(v.reshape(rb[0].shape), rb, f"{what} {k}")
        if worst is not None:
            worst[k] = max(worst.get(k, 0.0), r)


def outside(got, ref):
    """Names of the outputs of got (name -> array) with an element outside ref's bound."""
    return [k for k, rb in ref.items() if R.ratio(np.asarray(got[k]).reshape(rb[0].shape), rb)[1].any()]


# ----------------------------------------------------------------------------------------------------------- fp32 restatement
def _bsum32(A, Bm):
    """float32 sum_rows A[r][i] B[r][j], numpy's pairwise summation over the rows (another order than the kernel's)."""
    At, Bt = np.ascontiguousarray(A.T), np.ascontiguousarray(Bm.T)
    out = np.empty((At.shape[0], Bt.shape[0]), np.float32)
    for i in range(0, At.shape[0], 32):
        out[i:i + 32] = (At[i:i + 32, None, :] * Bt[None]).sum(axis=2, dtype=np.float32)
    return out


def critic_grad_f32(m, obs, actions, y):
    """The whole statement in numpy float32, every operation rounded to fp32, sums pairwise: a second fp32 evaluation that
    must sit inside the bound.  Returns (name -> float32 array, {1: acts, 2: acts})."""
    f = np.float32
    x = np.concatenate([np.asarray(obs, f), np.asarray(actions, f)], axis=1)
    yy = np.asarray(y, f).reshape(-1)
    B = f(x.shape[0])
    out, acts_all, ls = {}, {}, []
    for c in (1, 2):
        layers = T.layers_of(m[f"q{c}"])
        nl = len(layers) - 1
        acts, h = [x], x
        for W, b in layers[:-1]:
            h = np.maximum(T._dense32(h, W, b), f(0))
            acts.append(h)
        q = T._dense32(h, *layers[-1])[:, 0]
        d = q - yy
        dq = d / B
        ls.append((d * d).sum(dtype=f) / B)
        out[f"q{c}"] = q
        out[f"q{c}.w{nl}"] = _bsum32(dq[:, None], h)
        out[f"q{c}.b{nl}"] = np.array([dq.sum(dtype=f)])
        dz = np.where(h > 0, dq[:, None] * layers[-1][0][0][None], f(0)).astype(f)
        for l in range(nl - 1, -1, -1):
            out[f"q{c}.w{l}"] = _bsum32(dz, acts[l])
            out[f"q{c}.b{l}"] = np.ascontiguousarray(dz.T).sum(axis=1, dtype=f)
            if l == 0:
                break
            da = T._dense32(dz, np.ascontiguousarray(layers[l][0].T), np.zeros(layers[l][0].shape[1], f))
            dz = np.where(acts[l] > 0, da, f(0)).astype(f)
        acts_all[c] = acts[1:]
    out["loss"] = np.array(f(0.5) * (ls[0] + ls[1]), f)
    return out, acts_all
