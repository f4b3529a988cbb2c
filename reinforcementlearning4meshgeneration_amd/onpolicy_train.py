"""The body of SB3 2.x's ``PPO.train()`` / ``A2C.train()`` as ONE call into the library (include/meshenv_onpolicy_train.h,
csrc/meshenv_onpolicy_train.h: k_optim_step_gated, k_train_finish):

    for epoch in range(n_epochs):
        for rollout_data in rollout_buffer.get(batch_size):
            ... evaluate_actions, the losses ...                                   FusedPPOGrad's statement
            if target_kl is not None and approx_kl > 1.5 * target_kl: continue_training = False; break
            zero_grad; backward; clip_grad_norm_; optimizer.step()
        _n_updates += 1
        if not continue_training: break
    explained_variance(values, returns); the logged means

``FusedOnPolicyTrain.train(out)`` enqueues every launch of every epoch (per epoch one gather, per minibatch the launches of
``FusedPPOGrad.backward`` and one gated optimiser step, then the log kernel and the refresh of the rollout policy) and returns.
The early stop on ``target_kl`` is a flag on the device, so nothing is read back between minibatches: without a ``target_kl``
there is no synchronisation at all, with one there is exactly one small read-back at the end (how many steps were applied and
how many epochs ran, for the optimiser's ``step`` and ``_n_updates``).  After a stop the remaining gradient launches of the
queue still run, on unchanged parameters, and are ignored; ``p.grad`` then holds the stopping minibatch's clipped gradients
where SB3 would still hold the previous minibatch's (nothing reads them).

    tr = FusedOnPolicyTrain.from_sb3(model, policy)        # policy: the FusedPolicy with bind_live(model) done
    out = env.collect_rollout(policy, T, gamma=model.gamma, gae_lambda=model.gae_lambda)
    logs = tr.train(out)                                   # queued; logs.device is the [12] float64 tensor on the GPU
    print(logs.read())                                     # one copy: SB3's train/... keys as Python floats

The functions of this module that take no device (``hyper``, ``check_perms``, ``step_values``, ``scalar_sets``,
``OnPolicyTrainSpec``) are the host half: every refusal is made by them or by the classes this one drives."""
from __future__ import annotations

import ctypes as C
import math
from typing import List, Optional

from . import _capi
from . import sb3_nets as N
from ._handle import Handle
from .optim_step import PROGRAMS, FusedOptimStep, OptimStepSpec, Plan, adam_scalars
from .ppo_grad import FusedPPOGrad, PPOGradSpec
from .rollout_buffer import DeviceRolloutBuffer, minibatch_bounds

OUTPUTS = ("loss", "policy_gradient_loss", "value_loss", "entropy_loss", "approx_kl", "clip_fraction", "explained_variance", "std",
           "steps_applied", "epochs_run", "minibatches_evaluated", "grad_norm")       # meshenv_onpolicy_train.h's enum
MAX_MINIBATCHES = _capi.TRAIN_MAX_MINIBATCHES
# what SB3 records, in its order: PPO.train, A2C.train
PPO_KEYS = ("entropy_loss", "policy_gradient_loss", "value_loss", "approx_kl", "clip_fraction", "loss", "explained_variance", "std")
A2C_KEYS = ("explained_variance", "entropy_loss", "policy_loss", "value_loss", "std")
COUNTS = ("steps_applied", "epochs_run", "minibatches_evaluated")


def hyper(model) -> dict:
    """What ``PPO.train`` / ``A2C.train`` read from the model at the call.  A model whose ``clip_range`` is None (or absent) is
    A2C: one pass over one minibatch of all rows unless it says otherwise, no KL test.  ``clip_range`` is called with
    ``_current_progress_remaining`` when it is a schedule."""
    cr = getattr(model, "clip_range", None)
    a2c = cr is None
    progress = getattr(model, "_current_progress_remaining", 1.0)
    clip = None if a2c else float(cr(progress) if callable(cr) else cr)
    n_epochs = getattr(model, "n_epochs", 1)
    if isinstance(n_epochs, bool) or not isinstance(n_epochs, int) or n_epochs < 1:
        raise ValueError(f"n_epochs must be a positive int, got {n_epochs!r}")
    target_kl = None if a2c else getattr(model, "target_kl", None)
    if target_kl is not None:
        target_kl = float(target_kl)
        if not target_kl >= 0.0:                         # NaN fails the comparison
            raise ValueError(f"target_kl must be >= 0 or None, got {model.target_kl!r}")
    return dict(a2c=a2c, clip_range=clip, n_epochs=n_epochs, batch_size=getattr(model, "batch_size", None), target_kl=target_kl,
                ent_coef=getattr(model, "ent_coef", 0.0), vf_coef=getattr(model, "vf_coef", 0.5),
                normalize_advantage=bool(getattr(model, "normalize_advantage", not a2c)), max_grad_norm=getattr(model, "max_grad_norm", 0.5))


def update_learning_rate(model, optimizer) -> None:
    """SB3's ``_update_learning_rate``: ``lr_schedule(_current_progress_remaining)`` into every param group, when the model
    has a schedule.  It runs before the optimiser scalars of a ``train()`` are formed, so they carry the scheduled ``lr``."""
    schedule = getattr(model, "lr_schedule", None)
    if schedule is not None:
        lr = schedule(getattr(model, "_current_progress_remaining", 1.0))
        for group in optimizer.param_groups:
            group["lr"] = lr


def check_perms(perms, n_epochs: int, rows: int):
    """``perms`` as ``train`` takes it: an int32 or int64 tensor [n_epochs, rows], contiguous, one permutation of SB3's flat
    order ``i = env * T + t`` per epoch, on any device."""
    import torch
    if not torch.is_tensor(perms):
        raise ValueError(f"perms must be an int32 or int64 tensor, got {type(perms).__name__}")
    if perms.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"perms is {str(perms.dtype).replace('torch.', '')}, not int32 or int64")
    if tuple(perms.shape) != (n_epochs, rows):
        raise ValueError(f"perms has shape {tuple(perms.shape)}, not ({n_epochs}, {rows}): one permutation of the rows per epoch")
    if not perms.is_contiguous():
        raise ValueError("perms is not contiguous")
    return perms


def step_values(step0: float, K: int) -> List[float]:
    """[step0, step0 + 1, ..., step0 + K] as K float32 increments give them: what ``state['step'] += 1`` leaves, K times."""
    import numpy as np
    v, one, out = np.float32(step0), np.float32(1.0), [float(np.float32(step0))]
    for _ in range(K):
        v = v + one
        out.append(float(v))
    return out


def scalar_sets(spec: OptimStepSpec, plan: Plan, K: int):
    """(a C array of K ``MeshOptimScalars``, the step values per optimiser of the plan): the sets ``OptimStepSpec.commit`` would
    return over K successive steps from the state as it is, formed as it forms them (in doubles from the incremented step,
    rounded to float by the structure).  Nothing is stepped."""
    arr = (_capi.MeshOptimScalars * K)()
    values = []
    for b, (g, steps) in enumerate(plan.groups):
        vals = step_values(steps[0].item(), K)
        values.append(vals)
        if "betas" not in g:                             # RMSprop: the same block at every step
            lr, alpha, eps = g["lr"], g["alpha"], g["eps"]
            for S in arr:
                S.step_size[b], S.bc2_sqrt[b], S.w1[b] = lr, 1.0, 0.0
                S.beta2[b], S.w2[b], S.eps[b] = alpha, 1 - alpha, eps
            continue
        (beta1, beta2), lr, eps = g["betas"], g["lr"], g["eps"]
        for k, S in enumerate(arr):
            S.step_size[b], S.bc2_sqrt[b] = adam_scalars(vals[k + 1], lr, beta1, beta2)
            S.w1[b], S.beta2[b], S.w2[b], S.eps[b] = 1 - beta1, beta2, 1 - beta2, eps
    for S in arr:
        S.tau, S.one_minus_tau = spec.tau, 1 - spec.tau
    return arr, values


class OnPolicyTrainSpec:
    """The host half: the two specs a train() drives, built from an SB3-shaped PPO / A2C model, with their refusals
    (``clip_range_vf``, gSDE, the network's shape; the optimiser's class and flags)."""

    def __init__(self, model, grad: Optional[PPOGradSpec] = None, optim: Optional[OptimStepSpec] = None):
        self.model = model
        self.grad = PPOGradSpec.from_sb3(model) if grad is None else grad
        self.optim = OptimStepSpec.from_sb3(model) if optim is None else optim
        if self.optim.policy is None:
            raise ValueError("the optimiser spec has no policy optimiser: FusedOnPolicyTrain steps model.policy.optimizer")
        stepped = {id(p) for p in self.optim.policy.param_groups[0]["params"]}
        if stepped != {id(p) for p in self.grad.params}:
            raise ValueError("the policy optimiser's parameters are not the 13 tensors FusedPPOGrad writes gradients for")
        hyper(model)

    @classmethod
    def from_sb3(cls, model) -> "OnPolicyTrainSpec":
        return cls(model)


class TrainLogs:
    """What a ``train()`` leaves: ``device`` is the [12] float64 tensor on the GPU (``OUTPUTS``' order), ``read()`` the log
    dictionary under SB3's key names."""

    def __init__(self, device, a2c: bool, clip_range, model):
        self.device = device
        self._a2c, self._clip_range, self._model = a2c, clip_range, model
        self._host = None
        self.n_updates = None

    def values(self) -> dict:
        """OUTPUTS' names -> Python floats (the counts as ints): one copy, kept."""
        if self._host is None:
            self._host = self.device.cpu().tolist()
        return {k: int(v) if k in COUNTS else v for k, v in zip(OUTPUTS, self._host)}

    def read(self) -> dict:
        """SB3's ``logger.record`` keys of ``PPO.train`` (``A2C.train``) as Python floats, and ``grad_norm``, ``steps_applied``,
        ``epochs_run``, ``minibatches_evaluated`` under their own names."""
        v = self.values()
        n_updates = self.n_updates if self.n_updates is not None else getattr(self._model, "_n_updates", None)
        if self._a2c:
            logs = {"train/n_updates": n_updates}
            logs.update({"train/" + k: v["policy_gradient_loss" if k == "policy_loss" else k] for k in A2C_KEYS})
        else:
            logs = {"train/" + k: v[k] for k in PPO_KEYS}
            logs.update({"train/n_updates": n_updates, "train/clip_range": self._clip_range})
        logs.update({k: v[k] for k in ("grad_norm",) + COUNTS})
        return logs


class FusedOnPolicyTrain(Handle):
    """``train(out)``: one C call per ``PPO.train()`` / ``A2C.train()``.  Drives a FusedPPOGrad, a FusedOptimStep, a
    DeviceRolloutBuffer and (optionally) the FusedPolicy that collected the rollout; all four stay usable on their own."""
    PREFIX = "meshenv_onpolicy_train"

    def __init__(self, spec: OnPolicyTrainSpec, policy=None, pg: Optional[FusedPPOGrad] = None, fo: Optional[FusedOptimStep] = None,
                 rb: Optional[DeviceRolloutBuffer] = None, device: int = 0):
        self.spec, self.model = spec, spec.model
        super().__init__(device, check_device=spec.grad.check_device)
        self._owned = []              # the handles built here: close() closes them with this one
        self.pg = pg if pg is not None else self._own(FusedPPOGrad(spec.grad, device))
        self.fo = fo if fo is not None else self._own(FusedOptimStep(spec.optim, device))
        self.rb = rb if rb is not None else self._own(DeviceRolloutBuffer(device))
        self.policy = policy
        for name, h in (("pg", self.pg), ("fo", self.fo), ("rb", self.rb), ("policy", policy)):
            if h is not None and h.device != self.device:
                raise ValueError(f"{name} is on {h.device}, not on {self.device}")
        if policy is not None and getattr(policy, "_live", None) is None:
            raise ValueError("policy needs bind_live(model) first: train() ends with its refresh")
        self.calls = 0                # C calls so far: one per train()
        self.draw_ahead = True        # draw the next train()'s permutations at the end of this one (see train)
        self._ahead = None            # ((rows, n_epochs, stream), the permutations drawn ahead, the event after them)
        self._side = None             # the stream they are drawn on: beside the queue of train(), not behind it
        self._kept = None             # the plan of the policy program and the objects it was checked on (_prepared)

    def _own(self, h):
        self._owned.append(h)
        return h

    def close(self):
        super().close()               # waits for the stream the launches went to
        for h in getattr(self, "_owned", []):
            h.close()
        self._owned = []

    @classmethod
    def from_sb3(cls, model, policy=None, pg=None, fo=None, rb=None, device: int = 0):
        """model: SB3 2.x's PPO / A2C or anything shaped like it.  policy: the FusedPolicy with ``bind_live`` done, or None.
        pg, fo, rb: a FusedPPOGrad / FusedOptimStep / DeviceRolloutBuffer of the caller's for the same model, or None to
        build them.  Refuses, by name, what those classes refuse."""
        spec = OnPolicyTrainSpec(model, None if pg is None else pg.spec, None if fo is None else fo.spec)
        return cls(spec, policy, pg, fo, rb, device)

    def _prepared(self):
        """(plan, its key) of the policy program: ``_attach`` and ``OptimStepSpec.prepare``, whose checks look at every
        gradient and state tensor.  A plan is kept and handed out again while every OBJECT it was made from is still the one
        in place (the param group, each ``p.grad``, each state dict and the tensors in it: a tensor object cannot change its
        dtype, shape or storage behind that), the group's scalars are still Python floats and the ``step`` values still
        agree; anything else (a ``load_state_dict``, a gradient of the caller's, a new state entry) goes through the checks."""
        fo, opt = self.fo, self.fo.spec.policy
        kept = self._kept
        if kept is not None:
            plan, key, group, items = kept
            groups = opt.param_groups
            ok = len(groups) == 1 and groups[0] is group and fo.spec._group(opt, "the policy optimiser") is group
            ok = ok and all(type(group[k]) is float for k in (("lr", "alpha", "eps") if "betas" not in group else ("lr", "eps")))
            ok = ok and ("betas" not in group or all(type(b) is float for b in group["betas"]))
            if ok:
                state, step0 = opt.state, items[0][4].item()
                for p, grad, st, tensors, step in items:
                    now = state.get(p)
                    if p.grad is not grad or now is not st or len(st) != len(tensors) + 1 or st["step"] is not step or step.item() != step0 or \
                            any(st[k] is not x for k, x in tensors):
                        ok = False
                        break
            if ok:
                return plan, key
        self._kept = None
        self.pg._attach()
        plan = fo.spec.prepare("policy")
        key = plan.key()
        group = opt.param_groups[0]
        moments = ("square_avg",) if "betas" not in group else ("exp_avg", "exp_avg_sq")
        items = [(p, p.grad, opt.state[p], tuple((k, opt.state[p][k]) for k in moments), opt.state[p]["step"]) for p in group["params"]]
        if all(len(st) == len(tensors) + 1 for _, _, st, tensors, _ in items):
            self._kept = (plan, key, group, items)
        return plan, key

    def _draw(self, rows: int, n_epochs: int):
        """[n_epochs, rows]: one ``torch.randperm(rows)`` per epoch on the device."""
        t = self._torch
        if n_epochs == 1:
            return t.randperm(rows, device=self.device).unsqueeze(0)
        return t.stack([t.randperm(rows, device=self.device) for _ in range(n_epochs)])

    def train(self, out, perms=None, counted=None) -> TrainLogs:
        """The whole of ``train()`` on the rollout ``out`` (the dict ``collect_rollout(..., gamma=...)`` returns; references
        are kept, nothing is copied).  perms: None draws one ``torch.randperm(rows)`` per epoch on the device; else an int32 or
        int64 tensor [n_epochs, rows] (``np.random.permutation`` per epoch reproduces SB3's minibatches).

        With ``perms=None`` and ``draw_ahead`` (the default) the permutations of the NEXT ``train()`` are drawn at the end of
        this one, after the C call and on a stream of their own, while the device works through the queue:
        ``torch.randperm`` costs the host about as much as everything else in front of the call together.  They are used when the next call has the same rows, epochs
        and stream, and drawn again otherwise.  A ``torch.manual_seed`` between two calls therefore reaches the permutations
        one ``train()`` later; set ``draw_ahead = False`` (or pass ``perms``) where that matters.

        counted: a bound ``StepCounter`` (onpolicy_learn.py) makes this a COUNTED train(): the optimiser steps look their Adam
        scalars up by the counter's device-resident step count, the outputs go to the counter's next history row, and
        nothing is read back: ``step`` and ``_n_updates`` are the counter's to write at its one read-back (``StepCounter.read``).
        It refuses, before anything is enqueued, a train() whose K minibatches the counter's table has no entries left for."""
        t, model, pg, fo, rb = self._torch, self.model, self.pg, self.fo, self.rb
        hp = hyper(model)
        update_learning_rate(model, fo.spec.policy)
        rb.load(out)
        rows, n_epochs = rb.rows, hp["n_epochs"]
        bounds = minibatch_bounds(rows, hp["batch_size"])
        K = n_epochs * len(bounds)
        if K > MAX_MINIBATCHES:
            raise ValueError(f"{n_epochs} epochs x {len(bounds)} minibatches = {K}; at most {MAX_MINIBATCHES} per train()")
        batch = bounds[0][1] - bounds[0][0]
        a2c = hp["a2c"]
        clip = 0.0 if a2c else N.finite(hp["clip_range"], "clip_range")
        if not a2c and not clip > 0.0:
            raise ValueError(f"clip_range must be > 0 (or None for A2C's loss), got {hp['clip_range']!r}")
        ent, vf = N.finite(hp["ent_coef"], "ent_coef"), N.finite(hp["vf_coef"], "vf_coef")
        mgn = 0.0 if hp["max_grad_norm"] is None else N.finite(hp["max_grad_norm"], "max_grad_norm")
        if hp["max_grad_norm"] is not None and not mgn > 0.0:
            raise ValueError(f"max_grad_norm must be > 0 (or None), got {hp['max_grad_norm']!r}")
        if counted is not None:
            counted.check(self, K)
        stream = t.cuda.current_stream(self.device).cuda_stream
        drawn = perms is None
        if drawn:
            ahead, self._ahead = self._ahead, None
            if ahead is not None and ahead[0] == (rows, n_epochs, stream):
                perms = ahead[1]
                t.cuda.current_stream(self.device).wait_event(ahead[2])
            else:
                perms = self._draw(rows, n_epochs)
        else:
            perms = check_perms(perms, n_epochs, rows)
            if perms.device != self.device:
                perms = perms.to(self.device)
        gathered = rb._outputs()
        # prepare's checks once; the K scalar sets from the state as it is
        plan, key = self._prepared()
        for h in (self, pg, fo, rb, self.policy, counted):
            if h is not None and h._stream != stream:
                h._bind_stream()
        if fo._bound.get("policy") != key:
            fo._bind(plan, key)
        target_kl = hp["target_kl"]
        head = (self._h, pg._h, fo._h, PROGRAMS.index("policy"), rb._h, None if self.policy is None else self.policy._h, rb.T, rb.n_envs,
                self._ptrs(rb._in), self._ptrs(gathered), perms.data_ptr(), perms.element_size(), n_epochs, batch, 1 if a2c else 0,
                C.c_double(clip), C.c_float(ent), C.c_float(vf), 1 if hp["normalize_advantage"] else 0, 0 if hp["max_grad_norm"] is None else 1,
                C.c_float(mgn), C.c_double(math.inf if target_kl is None else target_kl))
        if counted is not None:
            out_dev = counted.run(self, head, fo.spec, plan, K)
        else:
            scalars, values = scalar_sets(fo.spec, plan, K)
            out_dev = t.empty(_capi.TRAIN_OUTPUTS, dtype=t.float64, device=self.device)
            rc = self._L.meshenv_onpolicy_train_run(*head, scalars, K, out_dev.data_ptr())
            self._check(rc, "meshenv_onpolicy_train_run")
        self.calls += 1
        rb.launches += n_epochs
        if drawn and self.draw_ahead:                    # the next train()'s permutations, while the device works through the queue
            if self._side is None:
                self._side = t.cuda.Stream(self.device)
            main = t.cuda.current_stream(self.device)
            with t.cuda.stream(self._side):
                nxt = self._draw(rows, n_epochs)
                done = t.cuda.Event()
                done.record(self._side)
            nxt.record_stream(main)                      # allocated on the side stream, read by the next train() on this one
            self._ahead = ((rows, n_epochs, stream), nxt, done)
        logs = TrainLogs(out_dev, a2c, hp["clip_range"], model)
        if counted is not None:                          # step and _n_updates: at the counter's one read-back
            counted.pending.append(logs)
            return logs
        if target_kl is None:                          # known on the host: nothing is read back
            steps, epochs = K, n_epochs
        else:                                            # ONE read-back per train(), after the queue drains
            v = logs.values()
            steps, epochs = v["steps_applied"], v["epochs_run"]
        for (g, step_tensors), vals in zip(plan.groups, values):
            for s in step_tensors:
                s.fill_(vals[steps])
        model._n_updates = getattr(model, "_n_updates", 0) + epochs
        logs.n_updates = model._n_updates
        return logs
