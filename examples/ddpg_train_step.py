#!/usr/bin/env python
"""A full DDPG gradient step as a fixed, short sequence of the library's own launches, examples/td3_train_step.py for DDPG:
DeviceReplayBuffer.sample, FusedTDTarget.target (the one-critic target), FusedDDPGGrad.critic_backward,
FusedOptimStep.critic_step(), FusedDDPGGrad.actor_backward (it reads the stepped critic), actor_step(polyak=True), which
steps the actor and moves both targets in one launch, and td.refresh() / policy.refresh(), which make the next target and the
next rollout see the new values.  DDPG is TD3 with one critic, policy_delay 1 and no target noise.

The model is a stand-in laid out as SB3 builds DDPG('MlpPolicy', env) (rl/baselines/RL_Mesh.py:113-228): actor.mu =
Linear(18, 400), ReLU, Linear(400, 300), ReLU, Linear(300, 3), Tanh; one q_network 21 -> 400 -> 300 -> 1; random weights --
SB3 is not installed in this image and there is no checkpoint to load.  The behaviour policy is the live actor with
NormalActionNoise (FusedPolicy, bound live).

    python examples/ddpg_train_step.py [--envs 4096] [--chunk 32] [--iterations 20] [--gradient-steps 8] [--batch 256] [--policy-delay 1]
                                       [--check]

--check keeps a stock-torch twin (clones of the parameters, torch.optim.Adam.step() and SB3's polyak_update fed the same
gradients) and prints the largest parameter difference between the two after the last step.
"""
import argparse
import copy
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

GAMMA, TAU, LR = 0.99, 0.005, 3e-4    # the learning rate of examples/td3_train_step.py and of its StockTwin


def ddpg_stand_in(torch):
    def mlp(n_in, n_out, tail=()):
        return torch.nn.Sequential(torch.nn.Linear(n_in, 400), torch.nn.ReLU(), torch.nn.Linear(400, 300), torch.nn.ReLU(),
                                   torch.nn.Linear(300, n_out), *tail).cuda()
    actor = types.SimpleNamespace(mu=mlp(18, 3, (torch.nn.Tanh(),)))
    critic = types.SimpleNamespace(q_networks=[mlp(21, 1)], n_critics=1)
    model = types.SimpleNamespace(actor=actor, actor_target=copy.deepcopy(actor), critic=critic, critic_target=copy.deepcopy(critic),
                                  gamma=GAMMA, tau=TAU, target_policy_noise=0.1, target_noise_clip=0.0)
    actor.optimizer = torch.optim.Adam(list(actor.mu.parameters()), lr=LR)
    critic.optimizer = torch.optim.Adam(list(critic.q_networks[0].parameters()), lr=LR)
    return model


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--chunk", type=int, default=32, help="vector steps per rollout call")
    ap.add_argument("--iterations", type=int, default=20)
    ap.add_argument("--gradient-steps", type=int, default=8)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--buffer-size", type=int, default=1_000_000)
    ap.add_argument("--sigma", type=float, default=0.1, help="NormalActionNoise sigma of the behaviour policy")
    ap.add_argument("--policy-delay", type=int, default=1, help="DDPG is TD3 with policy_delay 1; the flag of td3_train_step.py")
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    import torch

    from reinforcementlearning4meshgeneration_amd import (DeviceReplayBuffer, FusedDDPGGrad, FusedOptimStep, FusedPolicy, FusedTDTarget,
                                                          MeshVecEnv, boundary)
    from td3_train_step import StockTwin
    torch.manual_seed(999)
    model = ddpg_stand_in(torch)
    params, target_params = list(model.critic.q_networks[0].parameters()), list(model.critic_target.q_networks[0].parameters())
    actor_params, actor_target_params = list(model.actor.mu.parameters()), list(model.actor_target.mu.parameters())
    td = FusedTDTarget.from_sb3(model)                            # the TARGET networks
    dg = FusedDDPGGrad.from_sb3(model)                            # the LIVE actor and critic; loss_scale 1.0: SB3's statement
    fo = FusedOptimStep.from_sb3(model)
    policy = FusedPolicy.from_sb3(model, sigma=args.sigma)        # the behaviour policy: the live actor
    policy.bind_live(model)
    twin = StockTwin(torch, [params, actor_params], [target_params, actor_target_params]) if args.check else None

    env = MeshVecEnv([boundary(0)], n_envs=args.envs)
    buf = DeviceReplayBuffer(env, buffer_size=args.buffer_size)
    T = args.chunk
    env.reset_tensor()
    draw, batch_no, critic_losses, actor_losses = 0, 0, [], []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.iterations):
        out = env.collect_rollout(policy, T, seed=999, counter=draw)
        buf.add_rollout(out)
        draw += T
        for _ in range(args.gradient_steps):
            batch_no += 1
            s = buf.sample(args.batch, seed=1, counter=batch_no)
            y = td.target(s, seed=2, counter=batch_no)
            critic_losses.append(dg.critic_backward(s, y))                 # critic_loss; the gradients are in p.grad
            fo.critic_step()                                               # critic.optimizer.step(): one launch
            if twin:
                twin.step(0, params)
            if batch_no % args.policy_delay == 0:                          # every step at DDPG's policy_delay 1
                actor_losses.append(dg.actor_backward(s))                  # reads the stepped critic
                fo.actor_step(polyak=True)                                 # actor step and both polyak_updates: one launch
                if twin:
                    twin.step(1, actor_params)
                    twin.polyak()
                td.refresh()                                               # the next target reads the updated targets
        policy.refresh()                                                   # the next rollout acts with the stepped actor
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    result = {"workload": f"{args.envs} envs of boundary(0), {args.iterations} x ({T} vector steps, {args.gradient_steps} gradient "
                          f"steps at batch {args.batch})", "seconds": dt, "gradient_steps_per_s": batch_no / dt,
              "first_critic_loss": float(critic_losses[0]), "last_critic_loss": float(critic_losses[-1]),
              "first_actor_loss": float(actor_losses[0]) if actor_losses else None,
              "last_actor_loss": float(actor_losses[-1]) if actor_losses else None, "stored": buf.size() * args.envs}
    if args.check:
        result["max_abs_fused_minus_stock_parameter"] = twin.worst([params, actor_params], [target_params, actor_target_params])
        result["optimizer_steps"] = [float(model.critic.optimizer.state[params[0]]["step"]),
                                     float(model.actor.optimizer.state[actor_params[0]]["step"]) if actor_losses else 0.0]
    print(json.dumps(result))
    fo.close()
    dg.close()
    td.close()
    policy.close()
    env.close()


if __name__ == "__main__":
    main()
