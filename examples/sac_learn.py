#!/usr/bin/env python
"""SAC's whole ``learn()`` on the device: examples/sac_train.py with its loop (step_actor_T, add_rollout, train, close the
FusedActor and rebuild it through the host) replaced by ``FusedOffPolicyLearn.learn(total_timesteps)``: uniform Box actions while
``num_timesteps < learning_starts``, then the LIVE behaviour actor (``FusedActor.bind_live`` + ``refresh()``: one launch after
every ``train()``, no host copy), ``DeviceReplayBuffer.add_rollout``, the Monitor's episode statistics (``EpisodeStats``) and
``FusedOffPolicyTrain.train`` -- everything enqueued, nothing read back until the logs are.

The model is the SB3-shaped stand-in of examples/sac_train.py (MlpPolicy, ReLU, net_arch [128, 128, 128];
rl/baselines/RL_Mesh.py:183-196) with SB3's ``learning_starts``, ``train_freq``, ``gradient_steps``: SB3 is not installed in this image.

    python examples/sac_learn.py [--envs 4096] [--train-freq 32] [--iterations 20] [--gradient-steps 8] [--batch 100]
                                 [--learning-starts 10000] [--check]

--check runs the same loop on a deep-copied twin whose behaviour actor is rebuilt through the host before every collect and whose
train() is the composition of examples/sac_train_step.py, with the same seeds and counters, and prints how many parameter,
Adam-moment, step and replay-store tensors differ in any bit (0 is expected).
"""
import argparse
import copy
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]

from sac_train import SEED, Composition, sac_model, tensors  # noqa: E402


def twin_learn(twin, env, buf, plan, T):
    """The loop by hand on the twin: the public pieces, a host-rebuilt FusedActor per collect."""
    from reinforcementlearning4meshgeneration_amd import FusedActor
    steps = draws = 0
    for W, P, _, K in plan:
        if W:
            buf.add_rollout(env.collect_uniform(W, seed=SEED, counter=steps))
        if P:
            actor = FusedActor.from_sb3(twin.model)
            obs0 = env.obs.clone()
            out = env.step_actor_T(actor, actor.sample(obs0, SEED, steps + W), P, seed=SEED, counter=steps + W + 1,
                                   want_terminal_obs=True)
            buf.add_rollout(out, obs0=obs0)
            actor.close()
        steps += T
        if K:
            twin.train(K, draws)
            draws += K


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--train-freq", type=int, default=32, help="vector steps per collect")
    ap.add_argument("--iterations", type=int, default=20)
    ap.add_argument("--gradient-steps", type=int, default=8)
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--buffer-size", type=int, default=1_000_000)
    ap.add_argument("--learning-starts", type=int, default=10_000)
    ap.add_argument("--target-update-interval", type=int, default=1)
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    import torch

    from reinforcementlearning4meshgeneration_amd import DeviceReplayBuffer, FusedOffPolicyLearn, MeshVecEnv, boundary
    from reinforcementlearning4meshgeneration_amd.offpolicy_learn import plan
    torch.manual_seed(999)
    model = sac_model(torch, args.batch, args.target_update_interval)
    model.learning_starts, model.train_freq, model.gradient_steps = args.learning_starts, args.train_freq, args.gradient_steps
    model.buffer_size, model.num_timesteps = args.buffer_size, 0
    env = MeshVecEnv([boundary(0)], n_envs=args.envs)
    twin_model = copy.deepcopy(model) if args.check else None
    learn = FusedOffPolicyLearn.from_sb3(model, env)
    total = args.iterations * args.train_freq * args.envs
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    logs = learn.learn(total, seed=SEED)                  # every launch of every iteration enqueued; nothing read back
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    result = {"workload": f"{args.envs} envs of boundary(0), {logs.iterations} x ({args.train_freq} vector steps, one train() of "
                          f"{args.gradient_steps} gradient steps at batch {args.batch}), learning_starts {args.learning_starts}",
              "seconds": dt, "timesteps_per_s": model.num_timesteps / dt, "collect_calls": learn.collect_calls,
              "train_calls": learn.train.calls, "logs": logs.read()}
    if args.check:
        env2 = MeshVecEnv([boundary(0)], n_envs=args.envs)
        buf2 = DeviceReplayBuffer(env2, buffer_size=args.buffer_size)
        twin = Composition(twin_model, buf2)
        twin_learn(twin, env2, buf2, plan(0, total, args.envs, args.train_freq, args.learning_starts, args.gradient_steps),
                   args.train_freq)
        pairs = list(zip(tensors(model) + [learn.buffer.store, env.obs], tensors(twin.model) + [buf2.store, env2.obs]))
        result["tensors_compared"] = len(pairs)
        result["tensors_differing_in_any_bit"] = sum(not torch.equal(a.detach().cpu(), b.detach().cpu()) for a, b in pairs)
        env2.close()
    print(json.dumps(result))
    learn.close()
    env.close()


if __name__ == "__main__":
    main()
