#!/usr/bin/env python
"""examples/sac_learn.py with the reference's evaluation callback (rl/baselines/RL_Mesh.py:105-109: ``model.learn(total_timesteps,
callback=eval_callback)``; rl/baselines/CustomizeCallback.py:241-310) inside the device loop:

    cb = DeviceEvalCallback(eval_env, model, n_eval_episodes=..., eval_freq=..., eval_steps=...)
    learn.learn(total_timesteps, callback=cb)      every eval_freq vector steps: a queued evaluation on eval_env, one history
                                                   row (k_eval_reduce) and, when the mean reward improved, a copy of the live
                                                   parameters (k_keep_best) -- all enqueued, nothing read back
    cb.read()                                      one copy: timesteps, eval/mean_reward, eval/mean_ep_length, best_mean_reward, ...
    cb.save_npz("evaluations.npz")                 the reference's file: timesteps / results / ep_lengths
    cb.load_best(model); behaviour.refresh()       best_model's parameters back into the live model (no optimiser state)

An evaluation runs a FIXED number of vector steps (--eval-steps): nothing is read back, so it cannot stop early; episodes that do
not end within it are not recorded and show up in the ``short`` column.

    python examples/sac_learn_eval.py [--envs 4096] [--train-freq 32] [--iterations 20] [--eval-envs 64] [--eval-episodes 64]
                                      [--eval-freq 128] [--eval-steps 256] [--npz evaluations.npz]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.dirname(os.path.abspath(__file__))]

from sac_train import SEED, sac_model  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--train-freq", type=int, default=32, help="vector steps per collect")
    ap.add_argument("--iterations", type=int, default=20)
    ap.add_argument("--gradient-steps", type=int, default=8)
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--learning-starts", type=int, default=10_000)
    ap.add_argument("--eval-envs", type=int, default=64)
    ap.add_argument("--eval-episodes", type=int, default=64)
    ap.add_argument("--eval-freq", type=int, default=128, help="vector steps between evaluations (SB3's eval_freq)")
    ap.add_argument("--eval-steps", type=int, default=256, help="vector steps of every evaluation")
    ap.add_argument("--npz", default=None, help="write the reference's evaluations.npz here")
    args = ap.parse_args()
    import torch

    from reinforcementlearning4meshgeneration_amd import DeviceEvalCallback, FusedOffPolicyLearn, MeshVecEnv, boundary
    torch.manual_seed(999)
    model = sac_model(torch, args.batch, 1)
    model.learning_starts, model.train_freq, model.gradient_steps = args.learning_starts, args.train_freq, args.gradient_steps
    model.buffer_size, model.num_timesteps = 1_000_000, 0
    env = MeshVecEnv([boundary(0)], n_envs=args.envs)
    eval_env = MeshVecEnv([boundary(0)], n_envs=args.eval_envs, log_capacity=160)      # its own envs: an evaluation resets them
    learn = FusedOffPolicyLearn.from_sb3(model, env)
    total = args.iterations * args.train_freq * args.envs
    cb = DeviceEvalCallback(eval_env, model, n_eval_episodes=args.eval_episodes, eval_freq=args.eval_freq, eval_steps=args.eval_steps,
                            capacity=max(1, args.iterations * args.train_freq // args.eval_freq))
    logs = learn.learn(total, seed=SEED, callback=cb)          # evaluations included: everything enqueued, nothing read back
    got = cb.read()                                            # one copy
    result = {"evaluations": got["evaluations"], "timesteps": got["timesteps"].tolist(), "eval/mean_reward": got["mean_reward"].tolist(),
              "eval/mean_ep_length": got["mean_ep_length"].tolist(), "recorded": got["recorded"].tolist(), "short": got["short"].tolist(),
              "complete_rate": got["complete_rate"].tolist(), "improved": got["improved"].tolist(),
              "best_mean_reward": got["best_mean_reward"], "best_eval": got["best_eval"], "logs": logs.read()}
    if args.npz:
        cb.save_npz(args.npz)
    if got["best_eval"] >= 0:
        cb.load_best(model)                                    # a host call, outside learn()
        learn.behaviour.refresh()                              # the behaviour actor follows the restored parameters
        result["restored"] = f"the parameters of evaluation {got['best_eval']}"
    print(json.dumps(result))
    cb.close()
    learn.close()
    eval_env.close()
    env.close()


if __name__ == "__main__":
    main()
