#!/usr/bin/env python
"""One PPO.train() / A2C.train(), rows = n_envs x 32 steps, done two ways on twin models in the same run:

  (a) one call   FusedOnPolicyTrain.train(out): ONE C call that enqueues every launch of every epoch; the early stop is a flag on
                 the device
  (b) composed   the loop of examples/ppo_train_step.py's train_iteration: per epoch rb.get(batch_size), per minibatch
                 FusedPPOGrad.backward + FusedOptimStep.policy_step(), then FusedPolicy.refresh(); with a target_kl also the
                 float(approx_kl) test per minibatch, a synchronisation each

for the reference's PPO recipe (ReLU [128, 128], Adam(eps=1e-5), n_epochs = 10, batch 256) at 2048 and 8192 rows, without a
target_kl and with one that never triggers, and for SB3's default A2C (Tanh [64, 64], RMSprop, one minibatch of all rows) at
8192 rows.  The kernels of the loss gradient are the same on both sides; the difference is the Python and ctypes of about five
calls per minibatch.  (a) and (b) are interleaved train() by train() after a warm-up; a figure is the median of PAIRS
CUDA-event pairs, host overhead included on both sides.  Before anything is timed, one train() of each side from twin models
with the same permutations is asserted to leave equal bits in every parameter.

The gate: (a) is not slower than (b) in every row; the exit status is 1 when it fails (the file is written first).  No ratio is
fixed in advance.

    python tools/bench_onpolicy_train.py [--out profiles/onpolicy_train_bench.json] [--trace-only N]
    --stages FILE: no gate; the host time of every stage of an A2C train() at 8192 rows and of the loop, written to FILE
    --trace-only N: no timing; N train() calls of the PPO recipe at 8192 rows and nothing else (the run a kernel trace is taken from)"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import on_policy_stubs as S  # noqa: E402
import policy_ref as R  # noqa: E402
import ppo_grad_ref as P  # noqa: E402
from reinforcementlearning4meshgeneration_amd import (DeviceRolloutBuffer, FusedOnPolicyTrain, FusedOptimStep, FusedPolicy,  # noqa: E402
                                                      FusedPPOGrad)

N_STEPS, PAIRS, WARMUP = 32, 15, 3
NEVER = 1.0e9                     # a target_kl no approx_kl reaches
CASES = (("ppo", 2048, None), ("ppo", 8192, None), ("ppo", 2048, NEVER), ("ppo", 8192, NEVER), ("a2c", 8192, None))


def rollout(kind, rows):
    """[T][n] histories on the device from tests/ppo_grad_ref.py's batch rows (no environment is needed to time a train())."""
    T, n = N_STEPS, rows // N_STEPS
    d = P.batch(P.modules(S.RECIPES[kind]), rows, R.input_rows())
    host = {"obs": d["observations"].reshape(T, n, 18), "buffer_actions": d["actions"].reshape(T, n, 3),
            "value": d["returns"].reshape(T, n) * np.float32(0.5), "log_prob": d["old_log_prob"].reshape(T, n),
            "advantages": d["advantages"].reshape(T, n), "returns": d["returns"].reshape(T, n)}
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in host.items()}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def interleaved(fns, pairs, warmup):
    """Median milliseconds of each of fns, called in turn `pairs` times after `warmup` rounds."""
    for _ in range(warmup):
        for f in fns:
            f()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(pairs):
        for i, f in enumerate(fns):
            ms[i].append(timed(f))
    return [statistics.median(x) for x in ms]


class Side:
    """A model of the recipe (the reference's n_epochs = 10 and batch 256 for PPO) with the handles both ways drive."""

    def __init__(self, kind, target_kl):
        self.model, self.params = S.model(kind, "cuda")
        if kind == "ppo":
            self.model.n_epochs, self.model.batch_size = 10, 256
        self.model.target_kl, self.model._n_updates = target_kl, 0
        self.fp = FusedPolicy.from_sb3(self.model)
        self.fp.bind_live(self.model)
        self.pg, self.fo, self.rb = FusedPPOGrad.from_sb3(self.model), FusedOptimStep.from_sb3(self.model), DeviceRolloutBuffer()
        self.tr = FusedOnPolicyTrain.from_sb3(self.model, self.fp, pg=self.pg, fo=self.fo, rb=self.rb)

    def train(self, out, perms=None):
        return self.tr.train(out, perms)

    def composed(self, out, perms=None):
        """train_iteration of examples/ppo_train_step.py, after its collect_rollout."""
        model, pg, rb, fo = self.model, self.pg, self.rb, self.fo
        rb.load(out)
        clip_range = None if model.clip_range is None else float(model.clip_range(model._current_progress_remaining))
        stop = False
        for e in range(model.n_epochs):
            for mb in rb.get(model.batch_size, perm=None if perms is None else perms[e]):
                last = pg.backward(mb, clip_range=clip_range, ent_coef=model.ent_coef, vf_coef=model.vf_coef,
                                   normalize_advantage=model.normalize_advantage, max_grad_norm=model.max_grad_norm)
                if model.target_kl is not None and clip_range is not None and float(last["approx_kl"]) > 1.5 * model.target_kl:
                    stop = True
                    break
                fo.policy_step()
            model._n_updates += 1
            if stop:
                break
        self.fp.refresh()

    def close(self):
        for h in (self.tr, self.fo, self.rb, self.pg, self.fp):
            h.close()


def agreement(kind, rows, target_kl, out):
    """One train() against one composed train() from twin models, the same permutations: equal bits in every parameter."""
    a, b = Side(kind, target_kl), Side(kind, target_kl)
    perms = torch.stack([torch.randperm(rows, device="cuda") for _ in range(a.model.n_epochs)])
    a.train(out, perms)
    b.composed(out, perms)
    torch.cuda.synchronize()
    same = all(torch.equal(p, q) for p, q in zip(a.params, b.params))
    a.close(); b.close()
    assert same, (kind, rows, target_kl)


def measure():
    results = []
    for kind, rows, target_kl in CASES:
        out = rollout(kind, rows)
        agreement(kind, rows, target_kl, out)
        f, s = Side(kind, target_kl), Side(kind, target_kl)
        calls, binds = f.tr.calls, f.fo.binds
        t_f, t_s = interleaved([lambda: f.train(out), lambda: s.composed(out)], PAIRS, WARMUP)
        assert f.tr.calls == calls + PAIRS + WARMUP and f.fo.binds <= binds + 1, "more than one C call per train(), or a table upload in the steady state"
        assert all(bool(torch.isfinite(p).all()) for p in f.params + s.params)
        batch = f.model.batch_size or rows
        per_epoch = -(-rows // batch)
        row = dict(recipe=kind, rows=rows, batch_size=batch, n_epochs=f.model.n_epochs, minibatches=f.model.n_epochs * per_epoch,
                   target_kl=target_kl, one_call_train_ms=round(t_f, 4), composed_train_ms=round(t_s, 4),
                   composed_over_one_call=round(t_s / t_f, 3), gate_one_call_not_slower=t_f <= t_s)
        print(json.dumps(row), flush=True)
        results.append(row)
        f.close(); s.close()
    return results


def trace_only(n):
    out = rollout("ppo", 8192)
    f = Side("ppo", None)
    for _ in range(n):
        f.train(out)
    torch.cuda.synchronize()
    print(json.dumps(dict(recipe="ppo", rows=8192, trains=n, c_calls=f.tr.calls, uploads=f.fo.binds)), flush=True)
    f.close()


def stages(kind, rows, rounds=40):
    """Host microseconds (medians over `rounds` synchronised calls) of the stages of one train() and of one pass of the loop, each
    wrapped by a perf_counter pair, with the CUDA-event time of the whole: where the host time in front of the first launch goes.
    The one call is measured with the next permutations drawn ahead (the default) and drawn at the call."""
    import time

    from reinforcementlearning4meshgeneration_amd import onpolicy_train as T
    out = rollout(kind, rows)
    f, s = Side(kind, None), Side(kind, None)
    spent = {}

    def wrap(owner, name, label):
        fn = getattr(owner, name)

        def timed_fn(*a, **k):
            t0 = time.perf_counter()
            r = fn(*a, **k)
            spent.setdefault(label, []).append((time.perf_counter() - t0) * 1e6)
            return r
        setattr(owner, name, timed_fn)

    for owner, name, label in ((f.rb, "load", "rb.load"), (f.tr, "_draw", "randperm"), (f.pg, "_attach", "attach"), (f.fo.spec, "prepare", "prepare"),
                               (T, "scalar_sets", "scalar_sets"), (f.tr._L, "meshenv_onpolicy_train_run", "c_call"), (f, "train", "train_host_total"),
                               (s.rb, "load", "rb.load"), (s.rb, "get", "rb.get_with_randperm"), (s.pg, "backward", "backward"),
                               (s.fo, "policy_step", "policy_step"), (s.fp, "refresh", "refresh"), (s, "composed", "loop_host_total")):
        wrap(owner, name, label)
    rows_out = []
    for what, fn, ahead in (("one_call_drawn_ahead", f.train, True), ("one_call_drawn_at_the_call", f.train, False), ("loop", s.composed, None)):
        if ahead is not None:
            f.tr.draw_ahead, f.tr._ahead = ahead, None
        for _ in range(5):
            fn(out)
        torch.cuda.synchronize()
        spent.clear()
        ms = []
        for _ in range(rounds):
            ms.append(timed(lambda: fn(out)))
            torch.cuda.synchronize()
        row = dict(stages=what, recipe=kind, rows=rows, events_total_us=round(1e3 * statistics.median(ms), 1),
                   host_us={k: round(statistics.median(v), 1) for k, v in spent.items()})
        print(json.dumps(row), flush=True)
        rows_out.append(row)
    f.close(); s.close()
    return rows_out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "onpolicy_train_bench.json"))
    ap.add_argument("--trace-only", type=int, default=0, metavar="N")
    ap.add_argument("--stages", default=None, metavar="FILE")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_onpolicy_train needs a ROCm GPU: there is no CPU fallback")
    if args.trace_only:
        return trace_only(args.trace_only)
    if args.stages:
        with open(args.stages, "w") as fh:
            json.dump(dict(summary="bench_onpolicy_train --stages", device=torch.cuda.get_device_name(0), results=stages("a2c", 8192)), fh, indent=1)
            fh.write("\n")
        return
    from source_state import state
    results = measure()
    ok = all(r["gate_one_call_not_slower"] for r in results)
    summary = dict(summary="bench_onpolicy_train", device=torch.cuda.get_device_name(0), pairs=PAIRS, warmup=WARMUP, n_steps=N_STEPS,
                   **state(), gate_holds=ok, results=results)
    with open(args.out, "w") as fh:
        json.dump(summary, fh, indent=1)
        fh.write("\n")
    print(json.dumps(dict(summary="bench_onpolicy_train", gate_holds=ok, out=os.path.relpath(args.out, ROOT))), flush=True)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
