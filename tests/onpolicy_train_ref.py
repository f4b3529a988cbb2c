"""The loop of SB3 2.x's ``PPO.train`` / ``A2C.train`` transcribed (stable_baselines3 is not in the image), for the tests of
``FusedOnPolicyTrain``:

    train_loop        the epochs x minibatches loop with its lists, its early stop and its log arithmetic, over callables: the CPU
                      tests feed it hand-made records, ``compose`` feeds it the kernels the project already ships
    explained_variance_ref / explained_variance_f64
                      stable_baselines3.common.utils.explained_variance as numpy states it, and its fp64 restatement
    finish_order_f64  k_train_finish's own order of the same sums in numpy float64: 1024 strided partial sums and a halving tree
    compose           rb.get -> pg.backward -> host KL test -> fo.policy_step -> refresh on a model: the oracle of the GPU tests
    histories, perms  the synthetic [T][n] rollout and the fixed permutations both sides of a GPU test take
    eager_kls         the same loop on CPU torch (ppo_grad_ref.eager + torch's Adam): how the seed of the second-epoch stop was checked

PPO.train (ppo.py), restated:
    for epoch in range(n_epochs):
        approx_kl_divs = []
        for rollout_data in rollout_buffer.get(batch_size):
            ... losses ...
            pg_losses.append(policy_loss.item()); clip_fractions.append(clip_fraction); value_losses.append(value_loss.item())
            entropy_losses.append(entropy_loss.item()); approx_kl_divs.append(approx_kl_div)          # a float32 numpy value
            if self.target_kl is not None and approx_kl_div > 1.5 * self.target_kl: continue_training = False; break
            zero_grad; loss.backward(); clip_grad_norm_; optimizer.step()
        self._n_updates += 1
        if not continue_training: break
"""
import math

import numpy as np

SCALARS = ("loss", "policy_loss", "value_loss", "entropy_loss", "approx_kl", "clip_fraction", "grad_norm")
MEANS = ("policy_loss", "value_loss", "entropy_loss", "clip_fraction")


def train_loop(n_epochs, get, evaluate, step, target_kl=None):
    """SB3's loop.  get(epoch) yields the minibatches, evaluate(minibatch) returns a record (SCALARS -> float32 value),
    step(record) is zero_grad / backward / clip / optimizer.step().  Returns the lists, the counters and the logged values."""
    entropy_losses, pg_losses, value_losses, clip_fractions = [], [], [], []
    records, approx_kl_divs, loss, n_updates, steps = [], [], None, 0, 0
    continue_training = True
    for epoch in range(n_epochs):
        approx_kl_divs = []
        for rollout_data in get(epoch):
            rec = evaluate(rollout_data)
            records.append(rec)
            pg_losses.append(float(rec["policy_loss"]))                 # .item(): Python floats
            clip_fractions.append(float(rec["clip_fraction"]))
            value_losses.append(float(rec["value_loss"]))
            entropy_losses.append(float(rec["entropy_loss"]))
            approx_kl_divs.append(np.float32(rec["approx_kl"]))
            loss = rec["loss"]
            if target_kl is not None and approx_kl_divs[-1] > 1.5 * target_kl:     # float32 against a Python double
                continue_training = False
                break                                                    # BEFORE zero_grad / backward / clip / step
            step(rec)
            steps += 1
        n_updates += 1                                                   # also for the epoch that stopped
        if not continue_training:
            break
    logs = {"entropy_loss": np.mean(entropy_losses), "policy_gradient_loss": np.mean(pg_losses), "value_loss": np.mean(value_losses),
            "approx_kl": np.mean(approx_kl_divs), "clip_fraction": np.mean(clip_fractions), "loss": float(loss)}
    return dict(logs=logs, n_updates=n_updates, steps=steps, records=records, last_epoch_kl=[float(x) for x in approx_kl_divs],
                lists=dict(entropy_loss=entropy_losses, policy_loss=pg_losses, value_loss=value_losses, clip_fraction=clip_fractions))


def explained_variance_ref(y_pred, y_true):
    """stable_baselines3.common.utils.explained_variance, on the arrays as they are (float32 in SB3's buffers)."""
    assert y_true.ndim == 1 and y_pred.ndim == 1
    var_y = np.var(y_true)
    return np.nan if var_y == 0 else 1 - np.var(y_true - y_pred) / var_y


def explained_variance_f64(y_pred, y_true):
    """(the value, var(y_true - y_pred), var(y_true)) with d = y_true - y_pred formed in float32 and everything after it in
    fp64 with exactly rounded sums: what k_train_finish is held to."""
    y_pred, y_true = np.asarray(y_pred, np.float32), np.asarray(y_true, np.float32)
    d = (y_true - y_pred).astype(np.float64)
    r = y_true.astype(np.float64)
    n = len(r)

    def var(x):
        mean = math.fsum(x) / n
        return math.fsum((x - mean) ** 2) / n
    var_d, var_r = var(d), var(r)
    return (float("nan") if var_r == 0 else 1.0 - var_d / var_r), var_d, var_r


FINISH_THREADS = 1024      # kTrFinishThreads: k_train_finish's one workgroup


def finish_order_f64(values, returns, threads=FINISH_THREADS, trips=None):
    """(the value, var(returns - values), var(returns)) in k_train_finish's order (csrc/meshenv_onpolicy_train.h), restated in
    numpy float64 with no device code: d = r - v formed in float32; thread t adds its rows t, t + 1024, ... one after another
    to a partial sum that starts at 0.0; train_block_sum's tree halves the 1024 partial sums (red[t] += red[t + w], w = 512,
    256, ..., 1); two passes, the means first, then the centred squares (cr * cr rounded, then added: the library is built
    with -ffp-contract=off); every sum is divided by ``rows``.

    ``trips``: how many trips of the strided loop are taken; None is all of them.  ``trips=1`` is the kernel that reads only
    rows 0 .. 1023 and still divides by ``rows``: the counter-example the sizes above 1024 are there to catch."""
    r32, v32 = np.asarray(returns, np.float32), np.asarray(values, np.float32)
    rows = len(r32)
    r, d = r32.astype(np.float64), (r32 - v32).astype(np.float64)
    n_trips = -(-rows // threads) if trips is None else min(trips, -(-rows // threads))

    def block_sum(x):
        s = np.zeros(threads, np.float64)
        for k in range(n_trips):
            seg = x[k * threads:(k + 1) * threads]
            s[:len(seg)] = s[:len(seg)] + seg
        w = threads // 2
        while w > 0:
            s[:w] = s[:w] + s[w:2 * w]
            w >>= 1
        return float(s[0])
    mean_r, mean_d = block_sum(r) / float(rows), block_sum(d) / float(rows)
    cr, cd = r - mean_r, d - mean_d
    var_r, var_d = block_sum(cr * cr) / float(rows), block_sum(cd * cd) / float(rows)
    return (float("nan") if var_r == 0.0 else 1.0 - var_d / var_r), var_d, var_r


def std_ref(log_std):
    """exp(log_std).mean() in float32 over the three elements: each exp correctly rounded, ((e0 + e1) + e2) / 3."""
    e = [np.float32(math.exp(float(x))) for x in np.asarray(log_std, np.float32)]
    return float(np.float32(np.float32(e[0] + e[1]) + e[2]) / np.float32(3.0))


# ----------------------------------------------------------------------------------------------------------- inputs
def host_histories(kind, T, n, constant_returns=False, offset=0.0, scale=1.0):
    """A [T][n] rollout (numpy float32) of tests/ppo_grad_ref.py's batch rows for the recipe's policy: returns N(0, 1), values =
    returns / 2 (so var(returns - values) / var(returns) = 1 / 4).

    ``offset``, ``scale``: returns = offset + scale z with z the same N(0, 1) draw, in float32.  With ``offset == 0`` the values
    stay returns / 2; then d = returns - values is returns / 2 EXACTLY, so var_d / var_r is 1 / 4 over ANY subset of the rows
    and explained_variance cannot tell a kernel that drops rows.  With an offset, values = returns - scale / 2 z: d is still
    about scale / 2 z, but the mean of the returns is far from 0 and every row counts.  The defaults give the arrays of the
    two-argument call bit for bit."""
    import on_policy_stubs as S
    import policy_ref as R
    import ppo_grad_ref as P
    data = P.batch(P.modules(S.RECIPES[kind]), T * n, R.input_rows())
    z = data["returns"].reshape(T, n)
    plain = offset == 0.0 and scale == 1.0
    shifted = z if plain else np.float32(offset) + np.float32(scale) * z
    value = shifted * np.float32(0.5) if offset == 0.0 else shifted - np.float32(0.5 * scale) * z
    ret = np.full((T, n), 0.75, np.float32) if constant_returns else shifted
    host = {"obs": data["observations"].reshape(T, n, 18), "buffer_actions": data["actions"].reshape(T, n, 3),
            "value": value, "log_prob": data["old_log_prob"].reshape(T, n),
            "advantages": data["advantages"].reshape(T, n), "returns": ret}
    return {k: np.ascontiguousarray(v) for k, v in host.items()}


def perms(n_epochs, rows, seed=7):
    """[n_epochs, rows] int64: one numpy permutation per epoch, as SB3 draws them."""
    rng = np.random.default_rng(seed)
    return np.stack([rng.permutation(rows) for _ in range(n_epochs)]).astype(np.int64)


def hyper_of(model):
    clip = None if model.clip_range is None else float(model.clip_range(model._current_progress_remaining))
    return dict(clip_range=clip, ent_coef=model.ent_coef, vf_coef=model.vf_coef, normalize_advantage=model.normalize_advantage,
                max_grad_norm=model.max_grad_norm)


# ----------------------------------------------------------------------------------------------------------- the oracle on the GPU
def compose(model, pg, fo, rb, fp, out, perm_rows):
    """examples/ppo_train_step.py's ``train_iteration`` with SB3's bookkeeping: one gather per epoch, per minibatch the
    gradient launches, the KL test ON THE HOST (a read-back per minibatch) and ``policy_step()``; then the refresh.  perm_rows:
    [n_epochs, rows] device tensor.  Returns train_loop's dict; ``model._n_updates`` is advanced."""
    hp = hyper_of(model)
    rb.load(out)

    def evaluate(mb):
        res = pg.backward(mb, **hp)
        host = np.asarray([float(res[k]) for k in SCALARS], np.float64).astype(np.float32)
        return dict(zip(SCALARS, host))

    res = train_loop(model.n_epochs, lambda e: rb.get(model.batch_size, perm=perm_rows[e]), evaluate, lambda rec: fo.policy_step(),
                     getattr(model, "target_kl", None) if model.clip_range is not None else None)
    if fp is not None:
        fp.refresh()
    model._n_updates = getattr(model, "_n_updates", 0) + res["n_updates"]
    return res


# ----------------------------------------------------------------------------------------------------------- the same loop on CPU torch
def eager_kls(kind, T, n, perm_seed=7, n_epochs=2, batch_size=16):
    """approx_kl per minibatch of the loop run with CPU torch in float32 (ppo_grad_ref.eager, torch.optim.Adam(lr=3e-4,
    eps=1e-5)), old_log_prob being the policy's own log_prob of the rollout: an independent look at how KL grows over a
    train(), used to choose the seed of the second-epoch stop."""
    import torch

    import on_policy_stubs as S
    import ppo_grad_ref as P
    import rollout_buffer_ref as RB
    mods = P.modules(S.RECIPES[kind])
    host = host_histories(kind, T, n)
    rows = T * n
    hp = dict(clip_range=0.2, ent_coef=0.0, vf_coef=0.5, normalize_advantage=True, max_grad_norm=0.5)
    flat = {"observations": host["obs"].reshape(rows, 18), "actions": host["buffer_actions"].reshape(rows, 3),
            "old_log_prob": host["log_prob"].reshape(rows), "advantages": host["advantages"].reshape(rows), "returns": host["returns"].reshape(rows)}
    host["log_prob"] = P.eager(torch, mods, flat, hp, backward=False)["log_prob"].numpy().reshape(T, n)
    opt = torch.optim.Adam(P.params(mods), lr=3e-4, eps=1e-5)
    kls = []
    for e, perm in enumerate(perms(n_epochs, rows, perm_seed)):
        for mb in RB.get(host, perm, batch_size):
            kls.append(float(P.eager(torch, mods, mb, hp)["approx_kl"]))
            opt.step()
    return kls


def first_exceeding(kls, first, margin=0.01):
    """The first index j >= first with kls[j] >= (1 + margin) * max(kls[:j]), or None."""
    for j in range(first, len(kls)):
        if kls[j] >= (1.0 + margin) * max(kls[:j]) and kls[j] > 0:
            return j
    return None
