"""Host only: networks and batches on which DDPG's two gradient statements at [400, 300] (csrc/meshenv_wide_grad.h) are EXACT in
fp32, whatever the order of the sums: every product and every partial sum is a small integer times one power of two.  The
kernels must then return the float64 values themselves at every batch size, and a dropped, doubled or misplaced row, tile,
chunk or column is a wrong number with no tolerance to hide in.  tests/ddpg_grad_ref.py's bounds cannot see that at large B:
a batch sum of 65 536 rows carries gamma_1087 = 6.5e-5 of sum |terms| and one row is 1.5e-5 of it.  Shared by
tests/test_ddpg_range_cpu.py and tests/test_gpu_ddpg_range.py; nothing here touches a device.

The inputs (``build(B)``):

  critic statement   W_1 [400][21]: 2 nonzeros +-1 a neuron; W_2 [300][400]: 3 a neuron; b_1, b_2 in {-1, 0, 1}; out_w dense +-1,
                     out_b = 0; obs, actions in {-1, 0, 1}.  y = q - s B with q the integer forward value and s integers in
                     -2..2, nonzero on row 0, on the last row and on the first and last row of every chunk of the weight phase.
                     Then d = s B, d / B = s and dq = 2 loss_scale s exactly, for every B.
  actor statement    pre = 0 on the data and not identically: observation columns 9..17 repeat 0..8; layer-1 neurons 200..399
                     are neurons 0..199 with their weights moved from columns 0..8 to 9..17; layer-2 neurons 150..299 are
                     neurons 0..149 with their weights moved from inputs 0..199 to 200..399; W_3[i][150 + n] = -W_3[i][n] in
                     {-1, 0, 1}, b_3 = 0.  Hence actions_pi = tanh(0) = 0 and 1 - a a = 1, and the hidden layers' gradients are
                     nonzero because the paired rows of W_3 differ.
  its critic         the critic statement's hidden layers; out_w: 64 nonzeros +-c with c = B / 2^ceil(log2 B), so that
                     dq_da / B is exact (B's odd part has at most 13 bits at the sizes used: multiples of 8 up to 65 536).

``critic_eval`` / ``actor_eval`` are the two statements in float64 (any weights: they are tests/ddpg_grad_ref.py's chains without
the bounds) and return the per-row matrices of the weight phase as well.  ``assert_exact_precondition`` states, from those
float64 values alone, why fp32 is exact on them: for every batch sum and every per-row chain, sum |terms| / grid < 2^24, grid
the largest power of two that divides every term.  The two losses are exact only where B is a power of two (d d = s^2 B^2 and
S = c sum(m) need more than 24 bits otherwise): elsewhere they are compared within ddpg_grad_ref's bound, which
``critic_loss_bound`` / ``actor_loss_bound`` restate without the gradients' share of its cost.

``chunk_sums32`` is the weight phase's batch sum in float32 in the kernels' order, with named mistakes (``SUM_MUTANTS``).
"""
from __future__ import annotations

import types

import numpy as np

import ddpg_grad_ref as G
import ddpg_ref as D
from actor_grad_ref import _sum
from policy_ref import U, _f64, gamma, tanh_err

SIZES = (4096, 4168, 5128, 16392, 65528, 65536)
# B: (tiles, T, chunks, tiles of the last chunk, rows of the last tile)
SCHEDULE = {4096: (256, 4, 64, 4, 16), 4168: (261, 5, 53, 1, 8), 5128: (321, 6, 54, 3, 8), 16392: (1025, 17, 61, 5, 8),
            65528: (4096, 64, 64, 64, 8), 65536: (4096, 64, 64, 64, 16)}
SUM_MUTANTS = ("drop_last_row", "drop_last_tile", "drop_last_chunk", "last_chunk_twice")
LIMIT = 2.0 ** 24
HEAD_NONZEROS = 64
CRITIC_OUT = ("critic_loss", "q1") + G.CRITIC_GRADS
ACTOR_OUT = ("actor_loss",) + G.PARTS + G.ACTOR_GRADS


def schedule(B):
    """(tiles, T, chunks, tiles of the last chunk, rows of the last tile) of k_wgrad_weights at B rows."""
    tiles = (B + 15) // 16
    T = max(G.CHUNK_MIN_TILES, -(-tiles // G.MAX_CHUNKS))
    chunks = -(-tiles // T)
    return tiles, T, chunks, tiles - (chunks - 1) * T, B - 16 * (tiles - 1)


def where_row(B, row):
    """'tile t, chunk c' of a batch row."""
    _, T, _, _, _ = schedule(B)
    return f"row {row}: tile {row // 16}, chunk {row // (16 * T)}"


# ----------------------------------------------------------------------------------------------------------- the inputs
def _sparse(rng, n_out, n_in, lo, hi, k):
    """[n_out][n_in] with k entries +-1 per row, in columns lo..hi-1."""
    W = np.zeros((n_out, n_in), np.float32)
    for n in range(n_out):
        W[n, rng.choice(np.arange(lo, hi), size=k, replace=False)] = rng.choice([-1.0, 1.0], size=k)
    return W


def _bias(rng, n):
    return rng.integers(-1, 2, n).astype(np.float32)


def _set(seq, layers):
    import torch
    lin = [l for l in seq if type(l).__name__ == "Linear"]
    with torch.no_grad():
        for l, (W, b) in zip(lin, layers):
            assert tuple(l.weight.shape) == W.shape and tuple(l.bias.shape) == b.shape
            l.weight.copy_(torch.from_numpy(W))
            l.bias.copy_(torch.from_numpy(b))


def _model(actor, critic):
    """ddpg_grad_ref.model()-shaped, the live and the target networks alike."""
    m = D.ddpg_model()
    for a, c in ((m.actor, m.critic), (m.actor_target, m.critic_target)):
        _set(a.mu, actor)
        _set(c.q_networks[0], critic)
    return G.attach_optimizers(m)


def head_scale(B):
    """c = B / 2^ceil(log2 B), in (1/2, 1]."""
    return B / 2.0 ** int(np.ceil(np.log2(B)))


def build(B, seed=83):
    """The exact case at B rows: critic_model with obs, actions, y (and s) for the critic statement; actor_model with
    actor_obs for the actor statement.  The models are ddpg_grad_ref.model()-shaped; everything float32."""
    rng = np.random.default_rng(seed)
    f = np.float32
    # ---- the critic's hidden layers (both statements) and its two output layers
    c1, c2 = (_sparse(rng, 400, 21, 0, 21, 2), _bias(rng, 400)), (_sparse(rng, 300, 400, 0, 400, 3), _bias(rng, 300))
    out_dense = rng.choice([-1.0, 1.0], size=(1, 300)).astype(f)
    out_few = np.zeros((1, 300), f)
    out_few[0, rng.choice(300, size=HEAD_NONZEROS, replace=False)] = rng.choice([-1.0, 1.0], size=HEAD_NONZEROS)
    # ---- the paired actor
    w1 = np.zeros((400, 18), f)
    w1[:200] = _sparse(rng, 200, 18, 0, 9, 2)
    w1[200:, 9:] = w1[:200, :9]
    b1 = np.tile(_bias(rng, 200), 2)
    w2 = np.zeros((300, 400), f)
    w2[:150] = _sparse(rng, 150, 400, 0, 200, 3)
    w2[150:, 200:] = w2[:150, :200]
    b2 = np.tile(_bias(rng, 150), 2)
    w3 = rng.integers(-1, 2, (3, 150)).astype(f)
    w3 = np.concatenate([w3, -w3], axis=1)
    actor = [(w1, b1), (w2, b2), (w3, np.zeros(3, f))]
    # ---- the batches: a stream of their own, so that a prefix of a larger batch is the smaller one's rows
    rb = np.random.default_rng(seed + 1)
    obs = rb.integers(-1, 2, (SIZES[-1], 18))[:B].astype(f)
    act = rb.integers(-1, 2, (SIZES[-1], 3))[:B].astype(f)
    half = rb.integers(-1, 2, (SIZES[-1], 9))[:B].astype(f)
    s = rb.integers(-2, 3, SIZES[-1])[:B].astype(np.float64)
    _, T, chunks, _, _ = schedule(B)
    forced = sorted({0, B - 1} | {c * 16 * T for c in range(chunks)} | {min((c + 1) * 16 * T, B) - 1 for c in range(chunks)})
    s[forced] = np.where(s[forced] == 0, 1.0, s[forced])
    case = types.SimpleNamespace(B=B, s=s, forced=forced, obs=obs, actions=act, actor_obs=np.concatenate([half, half], axis=1),
                                 critic_model=_model(actor, [c1, c2, (out_dense, np.zeros(1, f))]),
                                 actor_model=_model(actor, [c1, c2, (out_few * f(head_scale(B)), np.zeros(1, f))]))
    q = _forward(G.live_layers(case.critic_model)[1], np.concatenate([obs, act], axis=1))[2][:, 0]
    y = q - s * B
    case.y = y.astype(f)
    assert np.array_equal(_f64(case.y), y) and float(f(head_scale(B))) == head_scale(B)
    return case


def distinct_batch(B, rows, period=5028):
    """ddpg_grad_ref.batch(B, rows) with its repeated observations made distinct: batch repeats policy_ref.input_rows() with
    period 5028, so beyond row 5027 column 0 gets 2^-10 (row // 5028) added (exact in fp32 at these magnitudes or not: the
    sum is rounded to float32 here, and the float32 rows are the inputs of reference and kernel alike)."""
    assert len(rows) == period
    obs, act, y = G.batch(B, rows)
    obs = obs.copy()
    obs[:, 0] += (2.0 ** -10 * (np.arange(B) // period)).astype(np.float32)
    return np.ascontiguousarray(obs), act, y


# ----------------------------------------------------------------------------------------------------------- float64
def _forward(layers, x):
    """a_1, a_2, the head's output and the chains [(name, x, W, b)] of one network in float64."""
    (w1, b1), (w2, b2), (wh, bh) = [(_f64(W), _f64(b)) for W, b in layers]
    x = _f64(x)
    a1 = np.maximum(x @ w1.T + b1, 0.0)
    a2 = np.maximum(a1 @ w2.T + b2, 0.0)
    return a1, a2, a2 @ wh.T + bh, [("z_1", x, w1, b1), ("z_2", a1, w2, b2), ("head", a2, wh, bh)]


def critic_eval(m, obs, actions, y, loss_scale=1.0):
    """The critic statement in float64: name -> array for CRITIC_OUT, 'acts1' [a_1, a_2], and what the precondition and
    the chunk-order sums read: 'sums' {name: (dz [B][n], act [B][k])} and 'chains' [(name, x, W, b)]."""
    x = np.concatenate([_f64(np.asarray(obs, np.float32)), _f64(np.asarray(actions, np.float32))], axis=1)
    yy = _f64(np.asarray(y, np.float32)).reshape(-1)
    B = x.shape[0]
    L = G.live_layers(m)[1]
    a1, a2, q, chains = _forward(L, x)
    q = q[:, 0]
    d = q - yy
    dq = 2.0 * loss_scale * (d / B)
    w2, wo = _f64(L[1][0]), _f64(L[2][0])[0]
    dz2 = (a2 > 0) * (dq[:, None] * wo[None])
    dz1 = (a1 > 0) * (dz2 @ w2)
    dh = np.stack([dq, d * d], axis=1)
    out = {"critic_loss": np.array(loss_scale * (d * d).sum() / B), "q1": q, "acts1": [a1, a2],
           "c.w2": dq[None] @ a2, "c.b2": np.array([dq.sum()]), "c.w1": dz2.T @ a1, "c.b1": dz2.sum(axis=0), "c.w0": dz1.T @ x,
           "c.b0": dz1.sum(axis=0)}
    out["sums"] = {"w1": (dz2, a1), "w0": (dz1, x), "head": (dh, a2)}
    out["chains"] = chains + [("da_1", dz2, w2.T, None)]
    return out


def actor_eval(m, obs):
    """The actor statement in float64: name -> array for ACTOR_OUT, 'acts', 'acts1', 'c.w2' / 'c.b2' (the zeros the call adds
    to the critic's set), 'sums' and 'chains' as critic_eval."""
    x = _f64(np.asarray(obs, np.float32))
    B = x.shape[0]
    LA, Lc = G.live_layers(m)
    a1, a2, pre, chains = _forward(LA, x)
    a = np.tanh(pre)
    c1, c2, q, cchains = _forward(Lc, np.concatenate([x, a], axis=1))
    q = q[:, 0]
    cw1, cw2, wo = _f64(Lc[0][0])[:, 18:21], _f64(Lc[1][0]), _f64(Lc[2][0])[0]
    cdz2 = (c2 > 0) * wo[None]
    cdz1 = (c1 > 0) * (cdz2 @ cw2)
    dq_da = cdz1 @ cw1
    d_pre = (-(dq_da / B)) * (1.0 - a * a)
    w2, w3 = _f64(LA[1][0]), _f64(LA[2][0])
    dz2 = (a2 > 0) * (d_pre @ w3)
    dz1 = (a1 > 0) * (dz2 @ w2)
    dh = np.concatenate([d_pre, q[:, None]], axis=1)
    out = {"actor_loss": np.array(-q.sum() / B), "actions_pi": a, "q1_pi": q, "dq_da": dq_da, "d_pre": d_pre, "acts": [a1, a2],
           "acts1": [c1, c2], "mu.w": d_pre.T @ a2, "mu.b": d_pre.sum(axis=0), "a.w1": dz2.T @ a1, "a.b1": dz2.sum(axis=0),
           "a.w0": dz1.T @ x, "a.b0": dz1.sum(axis=0), "c.w2": np.zeros((1, 300)), "c.b2": np.zeros(1)}
    out["sums"] = {"w1": (dz2, a1), "w0": (dz1, x), "head": (dh, a2)}
    out["chains"] = chains + [(f"critic {n}", *r) for n, *r in cchains] + \
        [("critic da_1", cdz2, cw2.T, None), ("dq_da", cdz1, cw1.T, None), ("dz_2", d_pre, w3.T, None), ("da_1", dz2, w2.T, None)]
    return out


def halved(ev):
    """critic_eval(..., loss_scale = 0.5) from critic_eval(..., 1.0): every output but q1 and the activations is linear in
    loss_scale, and a halving is exact."""
    return {k: v if k in ("q1", "acts1") else 0.5 * v for k, v in ev.items() if k not in ("sums", "chains")}


# ----------------------------------------------------------------------------------------------------------- the precondition
def grid_exponent(a):
    """g with 2^g the largest power of two dividing every element of a (float64); None where a is all zeros."""
    v = np.ascontiguousarray(_f64(a)).reshape(-1)
    assert np.isfinite(v).all()
    bits = v.view(np.int64)
    exp = (bits >> 52) & 0x7FF
    assert not ((exp == 0) & (v != 0)).any(), "a subnormal float64"
    mant = (bits & ((1 << 52) - 1)) | (1 << 52)
    low = np.ldexp((mant & -mant).astype(np.float64), (exp - 1075).astype(np.int32))   # the value of the lowest set bit
    low[v == 0] = np.inf
    g = float(low.min()) if low.size else np.inf
    return None if np.isinf(g) else int(np.log2(g))


def _units(total, *factors):
    """max of `total` (sums of |terms|) in units of the terms' grid: the product of the factors' grids."""
    g = [grid_exponent(f) for f in factors]
    if any(e is None for e in g) or not total.size:
        return 0.0
    return float(total.max()) / 2.0 ** sum(g)


def assert_exact_precondition(ev, what, losses):
    """From the float64 values alone: every batch sum of the weight phase (each product's columns of ones and, with
    `losses`, the loss column included) and every per-row chain has sum |terms| / grid < 2^24, so that every partial sum
    in every order is an integer below 2^24 times the grid, which fp32 holds.  Returns the largest such figure."""
    worst = {}
    for name, (dz, act) in ev["sums"].items():
        if name == "head":               # its last column is d^2 or q: summed against the column of ones alone, for the loss
            dz, last = dz[:, :-1], dz[:, -1]
            if losses:
                worst["sum loss"] = _units(np.abs(last).sum(keepdims=True), last)
        ones = np.abs(dz).sum(axis=0)                                          # the column of ones: the bias gradient
        worst[f"sum {name}"] = max(_units(np.abs(dz).T @ np.abs(act), dz, act), _units(ones, dz))
    for name, x, W, b in ev["chains"]:
        gx, gw, gb = grid_exponent(x), grid_exponent(W), None if b is None else grid_exponent(b)
        if gx is None or gw is None:
            continue
        # sum_k |x[r][k] W[n][k]| + |b[n]| <= max |x| max_n sum_k |W[n][k]| + max |b|: the rows of W are sparse and small, so
        # this bound is far below 2^24 and spares a [B, n] product per chain
        total = float(np.abs(x).max()) * float(np.abs(W).sum(axis=1).max()) + (0.0 if b is None else float(np.abs(b).max()))
        worst[f"chain {name}"] = total / 2.0 ** (gx + gw if gb is None else min(gx + gw, gb))
    bad = {k: v for k, v in worst.items() if not v < LIMIT}
    assert not bad, f"{what}: sum |terms| / grid reaches 2^24: {bad}"
    for k in ev:                                                               # and every value is an fp32 number
        if k not in ("sums", "chains", "acts", "acts1") and (losses or not k.endswith("_loss")):
            v = _f64(ev[k])
            assert np.array_equal(v, v.astype(np.float32).astype(np.float64)), f"{what}: {k} is not representable in fp32"
    return max(worst.values())


# ----------------------------------------------------------------------------------------------------------- the comparison
def first_difference(got, want):
    """The index of the first element of got that is not want's NUMBER (-0.0 equals 0.0; a NaN differs), or None."""
    g, w = _f64(got), _f64(want)
    assert g.size == w.size, (g.shape, w.shape)
    bad = ~(g.reshape(w.shape) == w)
    return tuple(int(i) for i in np.argwhere(bad)[0]) if bad.any() else None


def assert_same_numbers(got, want, names, what, B=None):
    """got[k] equals want[k] as numbers for k in names; the failure names (output, index), both values, the count and,
    for an output with a row per sample, the row's tile and chunk."""
    for k in names:
        g = got[k]
        g = g.detach().cpu().numpy() if hasattr(g, "detach") else np.asarray(g)
        at = first_difference(g, want[k])
        if at is not None:
            w = _f64(want[k])
            n = int((~(_f64(g).reshape(w.shape) == w)).sum())
            row = f" ({where_row(B, at[0])})" if B is not None and w.ndim and w.shape[0] == B else ""
            raise AssertionError(f"{what}: {k}{list(at)}{row}: got {_f64(g).reshape(w.shape)[at]!r}, float64 {w[at]!r}; "
                                 f"{n} of {w.size} elements differ")


# ----------------------------------------------------------------------------------------------------------- the losses' bounds
def critic_loss_bound(m, obs, actions, y, loss_scale=1.0):
    """(ref, bound) of critic_loss as ddpg_grad_ref.critic_grad states it, without the gradients."""
    x = np.concatenate([_f64(np.asarray(obs, np.float32)), _f64(np.asarray(actions, np.float32))], axis=1)
    yy, B = _f64(np.asarray(y, np.float32)).reshape(-1), x.shape[0]
    L = G.live_layers(m)[1]
    hid = G._hidden(L, x, np.zeros_like(x))
    q, eq = G._layer(hid[1][2], hid[1][3], *L[2], 2)
    d, eq = q[:, 0] - yy, eq[:, 0]
    e_d = eq + U * (np.abs(d) + eq)
    d2 = d * d
    e_d2 = 2.0 * np.abs(d) * e_d + e_d * e_d + U * (np.abs(d) + e_d) ** 2
    S, eS = d2.sum(), e_d2.sum() + gamma(G.reduction_roundings(B)) * (d2 + e_d2).sum()
    return np.array(loss_scale * S / B), np.array(loss_scale * (eS / B + U * (S + eS) / B))


def actor_loss_bound(m, obs):
    """(ref, bound) of actor_loss as ddpg_grad_ref.actor_grad states it, without the backward pass."""
    x = _f64(np.asarray(obs, np.float32))
    B = x.shape[0]
    LA, Lc = G.live_layers(m)
    hid = G._hidden(LA, x, np.zeros_like(x))
    pre, epre = G._layer(hid[1][2], hid[1][3], *LA[2], 2)
    a, ea = np.tanh(pre), tanh_err(pre, epre)
    hid = G._hidden(Lc, np.concatenate([x, a], axis=1), np.concatenate([np.zeros_like(x), ea], axis=1))
    q, eq = G._layer(hid[1][2], hid[1][3], *Lc[2], 2)
    S = _sum(q[:, 0], eq[:, 0], G.reduction_roundings(B))
    return np.array(-S[0] / B), np.array(S[1] / B + U * (abs(S[0]) + S[1]) / B)


# ----------------------------------------------------------------------------------------------------------- the kernels' order
def chunk_sums32(dz, act, B, mutants=()):
    """sum_rows dz[r][i] [act | 1][r][j] in float32 as k_wgrad_weights and k_wgrad_reduce order it: one accumulator per
    chunk of T row tiles, the rows ascending, four to a step (an MFMA step adds four rows' products to the accumulator); then
    the chunks' partial sums added in index order.  Returns {None: the sum, mutant: the sum with that mistake}, each
    [n][k + 1] float64 (column k: the bias gradient).  The mutants: the last row of the batch, its last row tile or its last
    chunk left out; the last chunk added twice."""
    import torch
    _, T, chunks, _, _ = schedule(B)
    rows = 16 * T
    d = torch.from_numpy(np.ascontiguousarray(dz, np.float32))
    a = torch.from_numpy(np.concatenate([np.asarray(act, np.float32), np.ones((B, 1), np.float32)], axis=1))
    assert d.shape[0] == a.shape[0] == B

    def partial(r0, r1):
        acc = torch.zeros((d.shape[1], a.shape[1]), dtype=torch.float32)
        for r in range(r0, r1, 4):
            acc.addmm_(d[r:min(r + 4, r1)].T, a[r:min(r + 4, r1)])
        return acc

    def total(parts):
        s = parts[0].clone()
        for p in parts[1:]:
            s = s + p
        return s.numpy().astype(np.float64)

    parts = [partial(c * rows, min((c + 1) * rows, B)) for c in range(chunks)]
    out = {None: total(parts)}
    r0 = (chunks - 1) * rows
    for mutant in mutants:
        if mutant == "drop_last_row":
            out[mutant] = total(parts[:-1] + [partial(r0, B - 1)])
        elif mutant == "drop_last_tile":
            out[mutant] = total(parts[:-1] + [partial(r0, 16 * ((B - 1) // 16))])
        elif mutant == "drop_last_chunk":
            out[mutant] = total(parts[:-1])
        elif mutant == "last_chunk_twice":
            out[mutant] = total(parts + [parts[-1]])
        else:
            raise ValueError(mutant)
    return out


def gradients_from_sums(ev, prefix, B, mutants=(), losses=True):
    """The statement's gradients (and, with `losses`, its loss) from chunk_sums32 of ev['sums']: {None or mutant: {name:
    float64 array}}, names and shapes as ev's.  prefix: 'c.' (the critic statement) or 'a.' (the actor statement)."""
    critic = prefix == "c."
    sums = {k: chunk_sums32(dz, act, B, mutants) for k, (dz, act) in ev["sums"].items()}
    out = {}
    for mu in (None, *mutants):
        w1, w0, head = sums["w1"][mu], sums["w0"][mu], sums["head"][mu]
        g = {f"{prefix}w1": w1[:, :-1], f"{prefix}b1": w1[:, -1], f"{prefix}w0": w0[:, :-1], f"{prefix}b0": w0[:, -1]}
        if critic:
            g.update({"c.w2": head[:1, :-1], "c.b2": head[:1, -1]})
            if losses:
                g["critic_loss"] = np.array(np.float32(head[1, -1]) / np.float32(B), np.float64)     # (loss_scale 1)
        else:
            g.update({"mu.w": head[:3, :-1], "mu.b": head[:3, -1]})
            if losses:
                g["actor_loss"] = np.array(-(np.float32(head[3, -1]) / np.float32(B)), np.float64)
        out[mu] = g
    return out
