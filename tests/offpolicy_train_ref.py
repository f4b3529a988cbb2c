"""The oracle of ``FusedOffPolicyTrain`` (reinforcementlearning4meshgeneration_amd/offpolicy_train.py): the composition the
project ships (examples/sac_train_step.py, examples/td3_train_step.py), driven by a transcription of SB3 2.x's two loops, on a
twin model made by ``copy.deepcopy`` before anything runs, with the same seeds and counters:

    SAC   buf.sample(B, seed, c) -> td.target(s, seed, c) -> cg.backward -> fo.critic_step() -> ag.backward(s, seed, c)
          -> fo.actor_step(polyak=k % target_update_interval == 0) -> td.refresh()
    TD3   _n_updates += 1; sample -> target -> cg.backward -> critic_step; if _n_updates % policy_delay == 0:
          ag.backward(s) -> fo.actor_step(polyak=True) -> td.refresh()

and the models and the buffer the tests share.  ``sac_steps`` / ``td3_steps`` are the two schedules as SB3 states them, with
no device; ``finish_order_means`` is k_offpolicy_finish's own order of the logged sums in numpy float64, with no device
either."""
import copy
import math

import numpy as np

import replay_ref
import rl_stubs

N_ENVS = 7
TAU = 0.005
LR = 3e-4


# ---------------------------------------------------------------------------------------- SB3's two schedules, transcribed
def sac_steps(gradient_steps, target_update_interval):
    """[(gradient_step, update_targets)] of one SAC.train: the index is the one inside the call."""
    return [(k, k % target_update_interval == 0) for k in range(gradient_steps)]


def td3_steps(gradient_steps, policy_delay, n_updates):
    """([(the incremented _n_updates, update the actor and the targets)], _n_updates afterwards) of one TD3.train."""
    out = []
    for _ in range(gradient_steps):
        n_updates += 1
        out.append((n_updates, n_updates % policy_delay == 0))
    return out, n_updates


# ---------------------------------------------------------------------------------------- k_offpolicy_finish, restated
FINISH_THREADS = 1024                                    # kTrFinishThreads
SAC_LEARNED, SAC_FIXED, TD3 = 0, 1, 2                    # kOffSacLearned, kOffSacFixed, kOffTd3


def phase_period(actor):
    """(phase, period) as meshenv_offpolicy_train_run derives them from the per-step flags "this step updates the actor": the
    first such step and the distance to the second; one actor step: period K; none: phase K, period 1."""
    at = [k for k, u in enumerate(actor) if u]
    K = len(actor)
    if not at:
        return K, 1
    return at[0], (K if len(at) == 1 else at[1] - at[0])


def finish_order_means(slots, K, phase, period, mode, ent_coef=None, threads=FINISH_THREADS, trips=None):
    """What k_offpolicy_finish (csrc/meshenv_offpolicy_train.h) writes, restated in numpy float64: thread t adds the float32
    slots of its steps k = t, t + 1024, ... one after another to four partial sums that start at 0.0 (critic_loss of every
    step; ent_coef of every step with a learned coefficient; actor_loss, and ent_coef_loss when learned, of the steps with
    k >= phase and (k - phase) % period == 0), train_block_sum's tree halves the 1024 partial sums of each, and the sums are
    divided by K or by the number of actor steps (NaN without one).  slots: [>= K][4] float32.

    Returns dict(critic_loss, actor_loss, ent_coef_loss, ent_coef, last_critic_loss, steps: the selected k).  ``trips``: how
    many trips of the strided loop are taken, None for all; ``trips=1`` is the kernel that reads steps 0 .. 1023 only."""
    slots = np.asarray(slots, np.float32)[:K].astype(np.float64)
    k = np.arange(K)
    selected = (k >= phase) & ((k - phase) % period == 0)
    learned = mode == SAC_LEARNED
    n_trips = -(-K // threads) if trips is None else min(trips, -(-K // threads))

    def block_sum(x, take):
        s = np.zeros(threads, np.float64)
        for trip in range(n_trips):
            seg, use = x[trip * threads:(trip + 1) * threads], take[trip * threads:(trip + 1) * threads]
            s[:len(seg)] = np.where(use, s[:len(seg)] + seg, s[:len(seg)])
        w = threads // 2
        while w > 0:
            s[:w] = s[:w] + s[w:2 * w]
            w >>= 1
        return float(s[0])
    every, none = np.ones(K, bool), np.zeros(K, bool)
    critic = block_sum(slots[:, 0], every)
    actor = block_sum(slots[:, 1], selected)
    ent_loss = block_sum(slots[:, 2], selected if learned else none)
    ent = block_sum(slots[:, 3], every if learned else none)
    n_actor = int(selected.sum())
    nan = float("nan")
    return dict(critic_loss=critic / float(K), actor_loss=actor / float(n_actor) if n_actor else nan,
                ent_coef_loss=ent_loss / float(n_actor) if learned and n_actor else nan,
                ent_coef=ent / float(K) if learned else float(np.float32(ent_coef)) if mode == SAC_FIXED else nan,
                last_critic_loss=float(slots[K - 1, 0]), steps=[int(i) for i in k[selected]])


# ---------------------------------------------------------------------------------------- models
def _modules(model):
    a = model.actor
    mods = [a.latent_pi, a.mu, a.log_std] if hasattr(a, "latent_pi") else [a.mu]
    if hasattr(model, "actor_target"):
        mods.append(model.actor_target.mu)
    return mods + list(model.critic.q_networks) + list(model.critic_target.q_networks)


def actor_params(model):
    a = model.actor
    mods = [a.latent_pi, a.mu, a.log_std] if hasattr(a, "latent_pi") else [a.mu]
    return [p for m in mods for p in m.parameters()]


def critic_params(model, attr="critic"):
    return [p for q in getattr(model, attr).q_networks for p in q.parameters()]


def model(kind, device="cuda", learned=True, seed=7, **attrs):
    """rl_stubs' SAC / TD3 model on ``device`` with SB3's optimisers attached (Adam, lr 3e-4), ``tau``, ``batch_size`` and
    ``_n_updates``; targets that differ from their sources; ``attrs`` set on the model last."""
    import torch
    torch.manual_seed(seed)
    m = rl_stubs.sac_model(learned=learned) if kind == "sac" else rl_stubs.td3_model()
    for mod in _modules(m):
        mod.to(device)
    with torch.no_grad():
        for p in critic_params(m, "critic_target"):
            p.mul_(0.75)
        if kind == "td3":
            for p in m.actor_target.mu.parameters():
                p.mul_(0.75)
    m.actor.optimizer = torch.optim.Adam(actor_params(m), lr=LR)
    m.critic.optimizer = torch.optim.Adam(critic_params(m), lr=LR)
    m.tau, m.batch_size, m._n_updates = TAU, 100, 0
    if kind == "sac":
        m.target_update_interval = 1
        if learned:
            m.log_ent_coef = torch.zeros(1, device=device).requires_grad_(True)
            m.ent_coef_optimizer = torch.optim.Adam([m.log_ent_coef], lr=LR)
        else:
            m.ent_coef_tensor = m.ent_coef_tensor.to(device)
            m.ent_coef_optimizer = None
    else:
        m.policy_delay = 2
    for k, v in attrs.items():
        setattr(m, k, v)
    return m


def twin(m):
    return copy.deepcopy(m)


def optimizers(m):
    out = [("critic", m.critic.optimizer), ("actor", m.actor.optimizer)]
    if getattr(m, "ent_coef_optimizer", None) is not None:
        out.append(("ent_coef", m.ent_coef_optimizer))
    return out


def state(m):
    """name -> tensor: every parameter of actor, critics, target critics, actor_target and log_ent_coef, every exp_avg /
    exp_avg_sq and every optimiser step."""
    out = {}
    for i, p in enumerate(actor_params(m)):
        out[f"actor.{i}"] = p
    for attr in ("critic", "critic_target"):
        for i, p in enumerate(critic_params(m, attr)):
            out[f"{attr}.{i}"] = p
    if hasattr(m, "actor_target"):
        for i, p in enumerate(m.actor_target.mu.parameters()):
            out[f"actor_target.{i}"] = p
    if getattr(m, "log_ent_coef", None) is not None:
        out["log_ent_coef"] = m.log_ent_coef
    for name, opt in optimizers(m):
        for i, p in enumerate(opt.param_groups[0]["params"]):
            st = opt.state.get(p, {})
            for k in ("exp_avg", "exp_avg_sq", "step"):
                if k in st:
                    out[f"{name}.optimizer.{i}.{k}"] = st[k]
    return out


def differing(a, b):
    """The names of ``state`` whose bits differ between two models (or that only one has)."""
    import torch
    sa, sb = state(a), state(b)
    bad = sorted(set(sa) ^ set(sb))
    for k in sa:
        if k in sb:
            x, y = sa[k].detach().cpu().contiguous(), sb[k].detach().cpu().contiguous()
            if x.shape != y.shape or not torch.equal(x.view(torch.int32), y.view(torch.int32)):
                bad.append(k)
    if getattr(a, "_n_updates", None) != getattr(b, "_n_updates", None):
        bad.append("_n_updates")
    return bad


# ---------------------------------------------------------------------------------------- the buffer
def fill(buf, steps=6, seed=11):
    """``steps`` vector steps of ``replay_ref.synthetic`` (finite values) stored into a DeviceReplayBuffer."""
    import torch
    n = buf.n_envs
    h = replay_ref.synthetic(steps, n, seed=seed, special=False)
    h["reward"] = h["reward"] * 0.05                     # |reward| of order one: losses that stay finite over the steps
    acts = np.concatenate([h["actions"], np.zeros((1, n, 3), np.float32)])
    d = dict(actions=acts, obs=h["obs_after"], reward=h["reward"], done=h["done"], complete=h["complete"], terminal_obs=h["terminal_obs"])
    out = {k: torch.from_numpy(np.ascontiguousarray(v)).to(buf.device) for k, v in d.items()}
    buf.add_rollout(out, obs0=torch.from_numpy(h["obs0"]).to(buf.device))
    return buf


# ---------------------------------------------------------------------------------------- the composition
class Composition:
    """The handles of examples/*_train_step.py on one model, and SB3's loop over them."""

    def __init__(self, m, buf):
        from reinforcementlearning4meshgeneration_amd import (FusedActorGrad, FusedCriticGrad, FusedOptimStep, FusedTD3ActorGrad,
                                                              FusedTDTarget)
        self.m, self.buf = m, buf
        self.sac = hasattr(m.actor, "latent_pi")
        self.td = FusedTDTarget.from_sb3(m)
        self.cg = FusedCriticGrad.from_sb3(m)
        self.ag = (FusedActorGrad if self.sac else FusedTD3ActorGrad).from_sb3(m)
        self.fo = FusedOptimStep.from_sb3(m)
        self.records = []                                # per gradient step: the float32 values SB3 would append

    def close(self):
        for h in (self.fo, self.ag, self.cg, self.td):
            h.close()

    def set_lr(self, lr):
        for _, opt in optimizers(self.m):
            opt.param_groups[0]["lr"] = lr

    def train(self, gradient_steps, batch_size=None, seed=0, counter=0):
        """One train(); returns the records of its steps (device tensors: read them afterwards)."""
        m, B = self.m, batch_size or self.m.batch_size
        recs = []
        if self.sac:
            for k, update in sac_steps(gradient_steps, m.target_update_interval):
                c = counter + k
                s = self.buf.sample(B, seed=seed, counter=c)
                rec = {}
                if getattr(m, "log_ent_coef", None) is not None:
                    rec["log_ent_coef"] = m.log_ent_coef.detach().clone()
                y = self.td.target(s, seed=seed, counter=c)
                rec["critic_loss"] = self.cg.backward(s, y)
                self.fo.critic_step()
                rec["actor_loss"], ent_loss = self.ag.backward(s, seed=seed, counter=c)
                if ent_loss is not None:
                    rec["ent_coef_loss"] = ent_loss
                self.fo.actor_step(polyak=update)
                self.td.refresh()
                recs.append(rec)
            m._n_updates += gradient_steps
        else:
            steps, after = td3_steps(gradient_steps, m.policy_delay, m._n_updates)
            for k, (_, update) in enumerate(steps):
                c = counter + k
                s = self.buf.sample(B, seed=seed, counter=c)
                y = self.td.target(s, seed=seed, counter=c)
                rec = {"critic_loss": self.cg.backward(s, y)}
                self.fo.critic_step()
                if update:
                    rec["actor_loss"] = self.ag.backward(s)
                    self.fo.actor_step(polyak=True)
                    self.td.refresh()
                recs.append(rec)
            m._n_updates = after
        self.records += recs
        return recs


def host(recs):
    """The records as Python floats (float32 values widened)."""
    return [{k: float(v.reshape(-1)[0]) for k, v in r.items()} for r in recs]


def mean_and_bound(values):
    """(math.fsum(values) / n, the bound of a float64 sum of n float32 values in any fixed order, divided by n): section 22's
    (n + 1) * 2**-53 * sum|x| / n."""
    n = len(values)
    return math.fsum(values) / n, (n + 1) * 2.0 ** -53 * math.fsum(abs(v) for v in values) / n
