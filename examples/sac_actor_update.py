#!/usr/bin/env python
"""A full SAC gradient step with every loss on the GPU: the loop of examples/sac_critic_update.py (rollout with the fused
actor, DeviceReplayBuffer, FusedTDTarget.target, FusedCriticGrad.backward and the critic step) followed by the actor and
entropy-coefficient statements of SB3's SAC.train in two launches (FusedActorGrad.backward: action_log_prob, both critics,
the min, `actor_loss.backward()` and the ent_coef loss).  The gradients land in p.grad of the live actor parameters and of
log_ent_coef, so the three optimiser steps are stock torch; they and the Polyak update write in place, the next backward reads
the parameters as they are then, and td.refresh() (one launch) makes the next target see the new actor and target critics.
The rollout actor holds a host-loaded copy of the weights: it is loaded again once per iteration.

The networks are the reference's architecture (MlpPolicy, ReLU, net_arch [128, 128, 128]; rl/baselines/RL_Mesh.py:183-196),
random-initialised stand-in modules: SB3 is not installed in this image and there is no checkpoint to load.

    python examples/sac_actor_update.py [--envs 4096] [--chunk 32] [--iterations 20] [--gradient-steps 8] [--batch 256] [--check]

--check prints the largest critic-gradient difference between the fused call and eager torch autograd on the same batch.
"""
import argparse
import copy
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GAMMA, TAU = 0.99, 0.005


def mlp(sizes):
    import torch
    mods = []
    for i in range(len(sizes) - 2):
        mods += [torch.nn.Linear(sizes[i], sizes[i + 1]), torch.nn.ReLU()]
    return torch.nn.Sequential(*mods, torch.nn.Linear(sizes[-2], sizes[-1]))


def eager_grads(torch, critic, params, s, y):
    """SAC.train's critic loss and backward in eager torch on the same modules; returns clones of the gradients."""
    keep = [p.grad for p in params]
    for p in params:
        p.grad = None
    qin = torch.cat([s.observations, s.actions], dim=1)
    loss = 0.5 * sum(torch.nn.functional.mse_loss(q(qin), y) for q in critic)
    loss.backward()
    out = [p.grad.clone() for p in params]
    for p, g in zip(params, keep):
        p.grad = g
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--chunk", type=int, default=32, help="vector steps per rollout call")
    ap.add_argument("--iterations", type=int, default=20)
    ap.add_argument("--gradient-steps", type=int, default=8)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--buffer-size", type=int, default=1_000_000)
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    import torch

    from reinforcementlearning4meshgeneration_amd import (DeviceReplayBuffer, FusedActor, FusedActorGrad, FusedCriticGrad, FusedTDTarget,
                                                          MeshVecEnv, boundary)
    torch.manual_seed(999)
    latent_pi = torch.nn.Sequential(*[m for i in range(3) for m in (torch.nn.Linear(18 if i == 0 else 128, 128), torch.nn.ReLU())])
    mu, log_std = torch.nn.Linear(128, 3), torch.nn.Linear(128, 3)
    critic = [mlp([21, 128, 128, 128, 1]) for _ in range(2)]
    lin = [m for m in latent_pi if isinstance(m, torch.nn.Linear)]
    actor = FusedActor.from_torch(lin, mu, log_std)                       # the rollout actor (host-packed once)
    for m in (latent_pi, mu, log_std, *critic):
        m.cuda()
    critic_target = copy.deepcopy(critic)
    log_ent_coef = torch.zeros(1, device="cuda", requires_grad=True)
    actor_params = [p for m in (latent_pi, mu, log_std) for p in m.parameters()]
    params = [p for q in critic for p in q.parameters()]
    target_params = [p for q in critic_target for p in q.parameters()]
    opt = torch.optim.Adam(params, lr=3e-4)
    opt_actor, opt_ent = torch.optim.Adam(actor_params, lr=3e-4), torch.optim.Adam([log_ent_coef], lr=3e-4)
    td = FusedTDTarget.sac(lin, mu, log_std, critic_target[0], critic_target[1], GAMMA, log_ent_coef=log_ent_coef)
    cg = FusedCriticGrad.sac(critic[0], critic[1])                        # the LIVE critics
    ag = FusedActorGrad.sac(lin, mu, log_std, critic[0], critic[1], log_ent_coef=log_ent_coef, target_entropy=-3.0)

    env = MeshVecEnv([boundary(0)], n_envs=args.envs)
    buf = DeviceReplayBuffer(env, buffer_size=args.buffer_size)
    T = args.chunk
    obs0 = env.reset().clone()
    actions = actor.sample(obs0, 999, 0)
    draw, batch_no, worst, losses = 1, 0, 0.0, []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.iterations):
        out = env.step_actor_T(actor, actions, T, seed=999, counter=draw, want_terminal_obs=True)
        buf.add_rollout(out, obs0=obs0)
        obs0, actions, draw = out["obs"][T - 1].clone(), out["actions"][T], draw + T
        for _ in range(args.gradient_steps):
            batch_no += 1
            s = buf.sample(args.batch, seed=1, counter=batch_no)
            y = td.target(s, seed=2, counter=batch_no)
            if args.check:
                want = eager_grads(torch, critic, params, s, y)
            loss = cg.backward(s, y)                                       # critic_loss; the gradients are in p.grad
            if args.check:
                worst = max(worst, max(float((p.grad - w).abs().max()) for p, w in zip(params, want)))
            opt.step()                                                     # stock torch
            actor_loss, ent_coef_loss = ag.backward(s, seed=3, counter=batch_no)   # before the ent_coef step: SB3's order
            opt_actor.step()
            opt_ent.step()
            with torch.no_grad():
                for p, pt in zip(params, target_params):
                    pt.data.mul_(1 - TAU).add_(p.data, alpha=TAU)
            td.refresh()                                                   # the next target reads the updated critics
            losses.append(torch.stack([loss, actor_loss, ent_coef_loss]))
        actor.close()
        actor = FusedActor.from_torch(lin, mu, log_std)                    # the rollout follows the trained actor
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    result = {"workload": f"{args.envs} envs of boundary(0), {args.iterations} x ({T} vector steps, {args.gradient_steps} gradient "
                          f"steps at batch {args.batch})", "seconds": dt, "gradient_steps_per_s": batch_no / dt,
              "first_critic_actor_ent_coef_loss": losses[0].tolist(), "last_critic_actor_ent_coef_loss": losses[-1].tolist(),
              "ent_coef": float(log_ent_coef.detach().exp()), "stored": buf.size() * args.envs}
    if args.check:
        result["max_abs_fused_minus_eager_gradient"] = worst
    print(json.dumps(result))
    ag.close()
    cg.close()
    td.close()
    actor.close()
    env.close()


if __name__ == "__main__":
    main()
