#!/usr/bin/env python
"""The SAC learn() of tools/bench_offpolicy_learn.py (20 iterations of 32 vector steps of 4096 envs and one train() of 8 gradient
steps at batch 100) with an evaluation every 4 iterations (eval_freq = 128 vector steps: 5 evaluations per learn(), each of 256
eval envs, one deterministic episode per env), done two ways in the same run:

  (a) device     FusedOffPolicyLearn.learn(callback=DeviceEvalCallback): per evaluation a queued evaluation of eval_steps vector
                 steps, k_eval_reduce, k_keep_best -- nothing read back
  (b) host       the same loop cut at the evaluation points with the API as it was before the callback: MeshVecEnv.evaluate (the
                 polling loop: it reads the envs-still-short counter every 32 steps, stops when every env is done, and copies
                 every record to the host), np.mean, and clone() of the snapshot tensors when the mean improved.  The baseline.

(a) and (b) are interleaved run by run after warm-up rounds; a figure is the median of PAIRS CUDA-event pairs, host overhead
included on both sides; the spread of a side is its interquartile range over the PAIRS runs.

The queued evaluation cannot stop early, so what (a) costs depends on the budget the user gives it.  The deterministic episodes of
this model end at about vector step 105, and the polling loop, which looks every 32 steps, runs 128.  Two budgets are measured:

  eval_steps = 128   the steps the polling loop itself runs: both sides launch the same steps, and the difference is what the
                     callback removes (the read-backs, the copies of the records, the cuts of learn()).  THE GATE is on this row:
                     the device median is not above the host median by more than the larger of the two spreads; the exit
                     status is 1 when it fails (the file is written first).  No ratio is fixed in advance.
  eval_steps = 256   a budget 2.4 times the episodes' length: the price of the fixed budget, reported and not gated.  Here (a)
                     launches 128 steps per evaluation that (b) skips.

Next to them, per row: fixed_budget_extra_ms, the time of one queued evaluation of eval_steps steps minus one of polled_steps
steps (the step at which every env is done for the final policy, read with check_every=1), median of PAIRS interleaved pairs.

Before anything is timed the two ways are asserted to agree: the same evaluation stamps, equal mean rewards (np.mean of SB3's
order against the kernel's order: within the bound of any summation order), the same best evaluation with bit-equal kept
parameters, and bit-equal training state.  Not measured here: a kernel trace, the split of the host stages.

    python tools/bench_eval_callback.py [--out profiles/eval_callback_bench.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import offpolicy_train_ref as TR  # noqa: E402
from reinforcementlearning4meshgeneration_amd import DeviceEvalCallback, FusedOffPolicyLearn, MeshVecEnv, boundary  # noqa: E402
from reinforcementlearning4meshgeneration_amd.eval_callback import eval_points, snapshot_set  # noqa: E402

N_ENVS, T, GRADIENT_STEPS, BATCH, ITERATIONS, PAIRS, WARMUP = 4096, 32, 8, 100, 20, 11, 2
ROWS = 4 * T
N_EVAL, EVAL_FREQ, BUDGETS, SEED = 256, 4 * T, (128, 256), 1           # BUDGETS[0] carries the gate


def model():
    """bench_offpolicy_learn's SAC model with the actor's mean action moved to (0, 0.6, 0.75), the centre of the biased random
    actions of the evaluation tests: deterministic episodes that build elements and end at about vector step 105."""
    m = TR.model("sac", batch_size=BATCH, learning_starts=0, train_freq=T, gradient_steps=GRADIENT_STEPS, buffer_size=ROWS * N_ENVS,
                 num_timesteps=0)
    low, high, mean = np.array([-1.0, -1.5, 0.0]), np.array([1.0, 1.5, 1.5]), np.array([0.0, 0.6, 0.75])
    with torch.no_grad():
        m.actor.mu.weight.mul_(0.3)
        m.actor.mu.bias.copy_(torch.tensor(np.arctanh((mean - low) / (high - low) * 2 - 1)))
    return m


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def iqr(xs):
    q = statistics.quantiles(xs, n=4)
    return q[2] - q[0]


class Device:
    def __init__(self, eval_steps):
        self.m = model()
        self.env, self.eval_env = MeshVecEnv([boundary(0)], n_envs=N_ENVS), MeshVecEnv([boundary(0)], n_envs=N_EVAL, log_capacity=160)
        self.learn = FusedOffPolicyLearn.from_sb3(self.m, self.env)
        self.cb = DeviceEvalCallback(self.eval_env, self.m, eval_freq=EVAL_FREQ, eval_steps=eval_steps, capacity=(WARMUP + PAIRS + 1) * 8)

    def run(self):
        self.learn.learn(ITERATIONS * T * N_ENVS, seed=SEED, callback=self.cb)

    def close(self):
        self.cb.close(); self.learn.close(); self.env.close(); self.eval_env.close()


class Host:
    """The loop a user writes without the callback: learn() cut in front of every collect an evaluation falls on."""

    def __init__(self, eval_steps):
        self.m, self.eval_steps = model(), eval_steps
        self.env, self.eval_env = MeshVecEnv([boundary(0)], n_envs=N_ENVS), MeshVecEnv([boundary(0)], n_envs=N_EVAL, log_capacity=160)
        self.learn = FusedOffPolicyLearn.from_sb3(self.m, self.env)
        self.tensors = [x for _, x in snapshot_set(self.m)[1]]
        self.n_calls, self.best_mean, self.best, self.means, self.stamps, self.steps = 0, -np.inf, None, [], [], []

    def run(self):
        pending = 0
        for _ in range(ITERATIONS):
            points = eval_points(self.n_calls, T, EVAL_FREQ)
            if points:
                if pending:
                    self.learn.learn(pending * T * N_ENVS, seed=SEED)
                    pending = 0
                for j in points:
                    res = self.eval_env.evaluate(self.learn.behaviour, deterministic=True, max_steps=self.eval_steps, quality=False)
                    mean = float(np.mean(res.reward)) if len(res) else float("nan")
                    self.means.append(mean); self.stamps.append(self.m.num_timesteps + j * N_ENVS); self.steps.append(res.steps)
                    if mean > self.best_mean:
                        self.best_mean, self.best = mean, [x.detach().clone() for x in self.tensors]
            self.n_calls += T
            pending += 1
        if pending:
            self.learn.learn(pending * T * N_ENVS, seed=SEED)

    def close(self):
        self.learn.close(); self.env.close(); self.eval_env.close()


def fixed_budget(dev, host, eval_steps):
    """One queued evaluation of eval_steps against one of the steps the polling loop needs for the same (final) policy."""
    polled = host.eval_env.evaluate(dev.learn.behaviour, deterministic=True, max_steps=eval_steps, check_every=1, quality=False)
    cbs = [DeviceEvalCallback(dev.eval_env, dev.m, eval_freq=1, eval_steps=s, capacity=WARMUP + PAIRS) for s in (eval_steps, max(polled.steps, 1))]
    fns = [lambda cb=cb: cb.evaluate_now(dev.learn.behaviour, 0) for cb in cbs]
    for _ in range(WARMUP):
        for f in fns:
            f()
    torch.cuda.synchronize()
    ms = [[], []]
    for _ in range(PAIRS):
        for i, f in enumerate(fns):
            ms[i].append(timed(f))
    for cb in cbs:
        cb.close()
    full, short = (statistics.median(x) for x in ms)
    return dict(polled_steps=polled.steps, polled_finished=polled.finished, queued_eval_ms=round(full, 3),
                queued_eval_polled_steps_ms=round(short, 3), fixed_budget_extra_ms=round(full - short, 3),
                fixed_budget_extra_per_learn_ms=round((full - short) * (ITERATIONS * T // EVAL_FREQ), 3))


def measure(eval_steps, gated):
    dev, host = Device(eval_steps), Host(eval_steps)
    # agreement first: one run each from the same initial model
    dev.run(); host.run()
    torch.cuda.synchronize()
    got = dev.cb.read()
    assert got["timesteps"].tolist() == host.stamps, (got["timesteps"].tolist(), host.stamps)
    want = np.array(host.means)
    assert np.array_equal(np.isnan(got["mean_reward"]), np.isnan(want)) and got["recorded"].max() > 0, (got["mean_reward"], host.means)
    bound = N_EVAL * 2.0 ** -52 * np.nanmax(np.abs(want))           # two orders of the same sum: np.mean's and the kernel's
    assert np.nanmax(np.abs(got["mean_reward"] - want)) <= bound, (got["mean_reward"], host.means)
    assert got["best_eval"] == int(np.nanargmax(want)) and TR.differing(dev.m, host.m) == []
    kept = dev.cb.best_state()
    assert all(torch.equal(kept[k], b) for (k, _), b in zip(snapshot_set(dev.m)[1], host.best))
    fns = [dev.run, host.run]
    for _ in range(WARMUP):
        for f in fns:
            f()
    torch.cuda.synchronize()
    ms = [[], []]
    for _ in range(PAIRS):
        for i, f in enumerate(fns):
            ms[i].append(timed(f))
    t_dev, t_host = (statistics.median(x) for x in ms)
    spread = max(iqr(ms[0]), iqr(ms[1]))
    evals = ITERATIONS * T // EVAL_FREQ
    row = dict(recipe="sac", n_envs=N_ENVS, vector_steps=T, gradient_steps=GRADIENT_STEPS, batch_size=BATCH, iterations=ITERATIONS,
               eval_envs=N_EVAL, eval_freq=EVAL_FREQ, eval_steps=eval_steps, evaluations_per_learn=evals, device_ms=round(t_dev, 3),
               host_ms=round(t_host, 3), device_ms_min_max=[round(min(ms[0]), 3), round(max(ms[0]), 3)],
               host_ms_min_max=[round(min(ms[1]), 3), round(max(ms[1]), 3)], device_iqr_ms=round(iqr(ms[0]), 3), host_iqr_ms=round(iqr(ms[1]), 3),
               host_over_device=round(t_host / t_dev, 3), host_polled_steps_last=host.steps[-evals:], recorded_last=got["recorded"].tolist(),
               gated=gated, device_not_slower_beyond_spread=t_dev <= t_host + spread)
    row.update(fixed_budget(dev, host, eval_steps))
    print(json.dumps(row), flush=True)
    dev.close(); host.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_callback_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_eval_callback needs a ROCm GPU: there is no CPU fallback")
    from source_state import state
    results = [measure(s, gated=i == 0) for i, s in enumerate(BUDGETS)]
    ok = all(r["device_not_slower_beyond_spread"] for r in results if r["gated"])
    summary = dict(summary="bench_eval_callback", device=torch.cuda.get_device_name(0), pairs=PAIRS, warmup=WARMUP, **state(),
                   not_measured=["kernel trace", "host-stage split"], gate_holds=ok, results=results)
    with open(args.out, "w") as fh:
        json.dump(summary, fh, indent=1)
        fh.write("\n")
    print(json.dumps(dict(summary="bench_eval_callback", gate_holds=ok, out=os.path.relpath(args.out, ROOT))), flush=True)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
