#!/usr/bin/env python
"""One SAC.train(gradient_steps) / TD3.train(gradient_steps) done two ways on twin models in the same run:

  (a) one call   FusedOffPolicyTrain.train(gradient_steps): ONE C call that enqueues every launch of every gradient step (one
                 draw of all minibatches, the noted critic step, the log kernel)
  (b) composed   the loop of examples/sac_train_step.py / td3_train_step.py: per gradient step buf.sample, td.target,
                 cg.backward, fo.critic_step(), ag.backward, fo.actor_step(polyak=...), td.refresh(): seven ctypes calls

for the reference's SAC recipe (ReLU [128, 128, 128], learned entropy coefficient) and for TD3 (ReLU [256, 256], policy_delay 2)
at batch 100 (the reference's) and 256 with 1, 8 and 64 gradient steps, from a replay buffer of 4096 envs x 32 steps of
boundary(0).  The kernels of a step are the same on both sides; the difference is the Python and ctypes of the calls per
step.  (a) and (b) are interleaved train() by train() after a warm-up; a figure is the median of PAIRS CUDA-event pairs, host
overhead included on both sides.  Before anything is timed, one train() of each side from equal twins is asserted to leave
equal bits in every parameter, Adam moment and step.

The gate: (a) is not slower than (b) in every row; the exit status is 1 when it fails (the file is written first).  No ratio is
fixed in advance.

    python tools/bench_offpolicy_train.py [--out profiles/offpolicy_train_bench.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import torch  # noqa: E402

import offpolicy_train_ref as TR  # noqa: E402
from reinforcementlearning4meshgeneration_amd import (DeviceReplayBuffer, FusedActor, FusedOffPolicyTrain, MeshVecEnv,  # noqa: E402
                                                      boundary)

N_ENVS, N_STEPS, PAIRS, WARMUP = 4096, 32, 15, 3
CASES = [(kind, batch, K) for kind in ("sac", "td3") for batch in (100, 256) for K in (1, 8, 64)]


def replay_buffer():
    """4096 envs x 32 vector steps of boundary(0), collected by a random-initialised fused SAC actor."""
    env = MeshVecEnv([boundary(0)], n_envs=N_ENVS)
    buf = DeviceReplayBuffer(env, buffer_size=N_ENVS * N_STEPS)
    a = TR.model("sac", device="cpu").actor
    actor = FusedActor.from_torch([m for m in a.latent_pi if type(m).__name__ == "Linear"], a.mu, a.log_std)
    obs0 = env.reset().clone()
    out = env.step_actor_T(actor, actor.sample(obs0, 999, 0), N_STEPS, seed=999, counter=1, want_terminal_obs=True)
    buf.add_rollout(out, obs0=obs0)
    actor.close()
    assert buf.size() == N_STEPS and buf.full
    return env, buf


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


def agreement(kind, batch, K, buf):
    """One train() against one composed train() from equal twins, the same seed and counters: equal bits."""
    m = TR.model(kind, batch_size=batch)
    tw = TR.twin(m)
    tr, comp = FusedOffPolicyTrain.from_sb3(m, buf), TR.Composition(tw, buf)
    tr.train(K, seed=1)
    comp.train(K, seed=1, counter=0)
    torch.cuda.synchronize()
    bad = TR.differing(m, tw)
    tr.close(); comp.close()
    assert bad == [], (kind, batch, K, bad[:5])


def measure(buf):
    results = []
    for kind, batch, K in CASES:
        agreement(kind, batch, K, buf)
        m = TR.model(kind, batch_size=batch)
        tw = TR.twin(m)
        tr, comp = FusedOffPolicyTrain.from_sb3(m, buf), TR.Composition(tw, buf)
        state = dict(counter=0)

        def composed():
            comp.records.clear()
            comp.train(K, seed=1, counter=state["counter"])
            state["counter"] += K
        calls = tr.calls
        t_f, t_s = interleaved([lambda: tr.train(K, seed=1), composed], PAIRS, WARMUP)
        assert tr.calls == calls + PAIRS + WARMUP, "more than one C call per train()"
        assert TR.differing(m, tw) == [], "the two sides drifted apart while they were timed"
        assert all(bool(torch.isfinite(v).all()) for v in TR.state(m).values())
        row = dict(recipe=kind, batch_size=batch, gradient_steps=K, one_call_train_ms=round(t_f, 4), composed_train_ms=round(t_s, 4),
                   one_call_us_per_step=round(1e3 * t_f / K, 2), composed_us_per_step=round(1e3 * t_s / K, 2),
                   composed_over_one_call=round(t_s / t_f, 3), gate_one_call_not_slower=t_f <= t_s)
        print(json.dumps(row), flush=True)
        results.append(row)
        tr.close(); comp.close()
    return results


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "offpolicy_train_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_offpolicy_train needs a ROCm GPU: there is no CPU fallback")
    from source_state import state
    env, buf = replay_buffer()
    results = measure(buf)
    env.close()
    ok = all(r["gate_one_call_not_slower"] for r in results)
    summary = dict(summary="bench_offpolicy_train", device=torch.cuda.get_device_name(0), pairs=PAIRS, warmup=WARMUP, n_envs=N_ENVS,
                   n_steps=N_STEPS, **state(), gate_holds=ok, results=results)
    with open(args.out, "w") as fh:
        json.dump(summary, fh, indent=1)
        fh.write("\n")
    print(json.dumps(dict(summary="bench_offpolicy_train", gate_holds=ok, out=os.path.relpath(args.out, ROOT))), flush=True)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
