#!/usr/bin/env python
"""SB3's ``PPO.learn`` / ``A2C.learn`` as ONE object: the loop of examples/ppo_train.py, the Monitor's episode figures and the
placement of EvalCallback's evaluations, all enqueued with nothing read back in between:

    learn = FusedOnPolicyLearn.from_sb3(model, env)      builds the FusedPolicy (bind_live done), the FusedOnPolicyTrain and the
                                                         EpisodeStats it drives; close() closes them
    logs = learn.learn(total_timesteps, callback=cb)     while num_timesteps < total: collect_rollout(gamma=...), EpisodeStats,
                                                         num_timesteps, train() with the refresh at its tail.  With a target_kl
                                                         every train() is counted on the device (k_optim_step_counted) and the
                                                         whole learn() ends in ONE small read-back; without one nothing is read
    logs.read()                                          the last train()'s keys, rollout/ep_rew_mean, time/total_timesteps, ...
    logs.history()                                       [iterations, 12]: every train()'s outputs

``model`` is anything shaped like SB3 2.x's PPO / A2C (``n_steps`` included); without stable_baselines3 installed the script
builds the stand-in of examples/ppo_train_step.py.

    python examples/ppo_learn.py [--a2c] [--target-kl 0.02] [--eval] [--iterations 5] [--n-envs 256] [--n-steps 32]"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402

from ppo_train_step import stand_in  # noqa: E402
from reinforcementlearning4meshgeneration_amd import DeviceEvalCallback, FusedOnPolicyLearn, MeshVecEnv, boundary  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--a2c", action="store_true")
    ap.add_argument("--target-kl", type=float, default=None)
    ap.add_argument("--eval", action="store_true", help="evaluate every 2 * n_steps vector steps on 16 envs of their own")
    ap.add_argument("--iterations", type=int, default=5)
    ap.add_argument("--n-envs", type=int, default=256)
    ap.add_argument("--n-steps", type=int, default=32)
    args = ap.parse_args()
    torch.manual_seed(0)
    model = stand_in(args.a2c)
    model.target_kl, model.n_steps, model.num_timesteps = args.target_kl, args.n_steps, 0
    env = MeshVecEnv([boundary(0)], n_envs=args.n_envs)
    env.reset()
    learn = FusedOnPolicyLearn.from_sb3(model, env)
    cb = eval_env = None
    if args.eval:
        eval_env = MeshVecEnv([boundary(0)], n_envs=16, log_capacity=160)      # its own envs: an evaluation resets them
        cb = DeviceEvalCallback(eval_env, model, eval_freq=2 * args.n_steps, eval_steps=128)
    logs = learn.learn(args.iterations * args.n_steps * args.n_envs, seed=0, callback=cb)   # everything queued
    for k, v in logs.read().items():                                                         # one copy (and the statistics')
        print(f"{k} = {v:.5g}" if isinstance(v, float) else f"{k} = {v}")
    print("steps applied per iteration:", [int(v) for v in logs.history()[:, 8]], "read-backs inside learn():", learn.readbacks)
    if cb is not None:
        got = cb.read()
        print("evaluations at", list(got["timesteps"]), "mean_reward", [round(float(x), 4) for x in got["mean_reward"]],
              "best", got["best_mean_reward"])
        cb.close()
        eval_env.close()
    learn.close(); env.close()


if __name__ == "__main__":
    main()
