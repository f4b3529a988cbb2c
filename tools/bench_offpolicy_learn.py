#!/usr/bin/env python
"""One off-policy learn loop of 20 iterations (32 vector steps of 4096 envs, then one train() of 8 gradient steps at batch 100)
done two ways in the same run, for the reference's SAC recipe (ReLU [128, 128, 128], learned entropy coefficient) and for TD3
(ReLU [256, 256], policy_delay 2, action-noise sigma 0.1):

  (a) learn      FusedOffPolicyLearn.learn(20 * 32 * 4096): collect with the LIVE behaviour (FusedActor / FusedPolicy after
                 refresh(), first action sampled on the current observation), add_rollout, EpisodeStats.update, train(),
                 refresh() -- nothing read back
  (b) loop       the loop of examples/sac_train.py / td3_train.py: step_actor_T with the pipelined next action, add_rollout,
                 train(); SAC then closes its FusedActor and rebuilds it through the host (ten .cpu() copies, a host repack, a
                 blocking upload); TD3 collects with an unrelated random SAC-shaped actor that never follows the trained one

(a) does MORE than (b): the episode statistics, and for TD3 a behaviour policy that is the trained actor (a [256, 256] policy
launch per vector step in place of the fused step + [128, 128, 128] actor launch).  (a) and (b) are interleaved loop by loop
after warm-up rounds; a figure is the median of PAIRS CUDA-event pairs, host overhead included on both sides.  SAC's host
rebuild is also timed alone (the same event pairs around actor.close() + FusedActor.from_torch).

Before anything is timed, learn() is asserted to leave equal bits (parameters, Adam moments, steps, targets, the replay store,
the env's observation) as the same loop with the behaviour REBUILT THROUGH THE HOST before every collect, at the timed sizes.

The gate: (a) is not slower than (b) in every row; the exit status is 1 when it fails (the file is written first).  No ratio is
fixed in advance.  Not measured here: a kernel trace, the split of the host stages.

    python tools/bench_offpolicy_learn.py [--out profiles/offpolicy_learn_bench.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import torch  # noqa: E402

import offpolicy_train_ref as TR  # noqa: E402
from reinforcementlearning4meshgeneration_amd import (DeviceReplayBuffer, FusedActor, FusedOffPolicyLearn, FusedOffPolicyTrain,  # noqa: E402
                                                      FusedPolicy, MeshVecEnv, boundary)

N_ENVS, T, GRADIENT_STEPS, BATCH, ITERATIONS, PAIRS, WARMUP = 4096, 32, 8, 100, 20, 15, 3
ROWS = 4 * T
SIGMA, SEED = 0.1, 1


def model(kind):
    return TR.model(kind, batch_size=BATCH, learning_starts=0, train_freq=T, gradient_steps=GRADIENT_STEPS, buffer_size=ROWS * N_ENVS,
                    num_timesteps=0)


def sac_linears(m):
    return [x for x in m.actor.latent_pi if type(x).__name__ == "Linear"]


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


class ParentLoop:
    """examples/sac_train.py / td3_train.py as they stand before FusedOffPolicyLearn."""

    def __init__(self, kind, m):
        self.kind, self.m = kind, m
        self.env = MeshVecEnv([boundary(0)], n_envs=N_ENVS)
        self.buf = DeviceReplayBuffer(self.env, buffer_size=ROWS * N_ENVS)
        self.tr = FusedOffPolicyTrain.from_sb3(m, self.buf)
        if kind == "sac":
            self.actor = FusedActor.from_torch(sac_linears(m), m.actor.mu, m.actor.log_std)
        else:
            torch.manual_seed(5)
            self.actor = FusedActor.from_torch([torch.nn.Linear(18, 128), torch.nn.Linear(128, 128), torch.nn.Linear(128, 128)],
                                               torch.nn.Linear(128, 3), torch.nn.Linear(128, 3))
        self.obs0 = self.env.reset().clone()
        self.actions = self.actor.sample(self.obs0, 999, 0)
        self.draw = 1

    def rebuild(self):
        m = self.m
        self.actor.close()
        self.actor = FusedActor.from_torch(sac_linears(m), m.actor.mu, m.actor.log_std)

    def run(self, iterations=ITERATIONS):
        for _ in range(iterations):
            out = self.env.step_actor_T(self.actor, self.actions, T, seed=999, counter=self.draw, want_terminal_obs=True)
            self.buf.add_rollout(out, obs0=self.obs0)
            self.obs0, self.actions, self.draw = out["obs"][T - 1].clone(), out["actions"][T], self.draw + T
            self.tr.train(GRADIENT_STEPS, seed=SEED)
            if self.kind == "sac":
                self.rebuild()

    def close(self):
        self.tr.close(); self.actor.close(); self.env.close()


def agreement(kind):
    """learn() against the same loop with a host-rebuilt behaviour, two iterations at the timed sizes: equal bits."""
    m = model(kind)
    tw = TR.twin(m)
    env, env2 = (MeshVecEnv([boundary(0)], n_envs=N_ENVS) for _ in range(2))
    learn = FusedOffPolicyLearn.from_sb3(m, env, action_noise_sigma=None if kind == "sac" else SIGMA)
    buf2 = DeviceReplayBuffer(env2, buffer_size=ROWS * N_ENVS)
    tr2 = FusedOffPolicyTrain.from_sb3(tw, buf2)
    learn.learn(2 * T * N_ENVS, seed=SEED)
    for it in range(2):
        if kind == "sac":
            b = FusedActor.from_sb3(tw)
            obs0 = env2.obs.clone()
            out = env2.step_actor_T(b, b.sample(obs0, SEED, it * T), T, seed=SEED, counter=it * T + 1, want_terminal_obs=True)
            buf2.add_rollout(out, obs0=obs0)
        else:
            b = FusedPolicy.from_sb3(tw, sigma=SIGMA)
            buf2.add_rollout(env2.collect_rollout(b, T, seed=SEED, counter=it * T))
        b.close()
        tr2.train(GRADIENT_STEPS, seed=SEED)
    torch.cuda.synchronize()
    bad = TR.differing(m, tw)
    same = torch.equal(learn.buffer.store.view(torch.int32), buf2.store.view(torch.int32)) and torch.equal(env.obs, env2.obs)
    learn.close(); tr2.close(); env.close(); env2.close()
    assert bad == [] and same, (kind, bad[:5], same)


def measure(kind):
    agreement(kind)
    m = model(kind)
    env = MeshVecEnv([boundary(0)], n_envs=N_ENVS)
    learn = FusedOffPolicyLearn.from_sb3(m, env, action_noise_sigma=None if kind == "sac" else SIGMA)
    parent = ParentLoop(kind, model(kind))
    fns = [lambda: learn.learn(ITERATIONS * T * N_ENVS, seed=SEED), parent.run]
    for _ in range(WARMUP):
        for f in fns:
            f()
    torch.cuda.synchronize()
    ms = [[], []]
    for _ in range(PAIRS):
        for i, f in enumerate(fns):
            ms[i].append(timed(f))
    t_learn, t_loop = (statistics.median(x) for x in ms)
    assert learn.train.calls == (WARMUP + PAIRS) * ITERATIONS == parent.tr.calls
    assert all(bool(torch.isfinite(v).all()) for v in TR.state(m).values())
    row = dict(recipe=kind, n_envs=N_ENVS, vector_steps=T, gradient_steps=GRADIENT_STEPS, batch_size=BATCH, iterations=ITERATIONS,
               learn_ms=round(t_learn, 3), loop_ms=round(t_loop, 3), learn_ms_min_max=[round(min(ms[0]), 3), round(max(ms[0]), 3)],
               loop_ms_min_max=[round(min(ms[1]), 3), round(max(ms[1]), 3)], loop_over_learn=round(t_loop / t_learn, 3),
               gate_learn_not_slower=t_learn <= t_loop, episodes=learn.stats.read()["episodes"])
    if kind == "sac":
        for _ in range(WARMUP):
            parent.rebuild()
        torch.cuda.synchronize()
        rb = statistics.median(timed(parent.rebuild) for _ in range(PAIRS))
        row.update(host_rebuild_ms=round(rb, 4), host_rebuilds_per_loop_ms=round(rb * ITERATIONS, 3),
                   rebuild_share_of_difference=round(rb * ITERATIONS / (t_loop - t_learn), 3) if t_loop != t_learn else None)
    print(json.dumps(row), flush=True)
    learn.close(); parent.close(); env.close()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "offpolicy_learn_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_offpolicy_learn needs a ROCm GPU: there is no CPU fallback")
    from source_state import state
    results = [measure(kind) for kind in ("sac", "td3")]
    ok = all(r["gate_learn_not_slower"] for r in results)
    summary = dict(summary="bench_offpolicy_learn", device=torch.cuda.get_device_name(0), pairs=PAIRS, warmup=WARMUP, **state(),
                   not_measured=["kernel trace", "host-stage split"], gate_holds=ok, results=results)
    with open(args.out, "w") as fh:
        json.dump(summary, fh, indent=1)
        fh.write("\n")
    print(json.dumps(dict(summary="bench_offpolicy_learn", gate_holds=ok, out=os.path.relpath(args.out, ROOT))), flush=True)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
