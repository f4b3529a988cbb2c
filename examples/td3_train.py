#!/usr/bin/env python
"""TD3 training with the whole of `TD3.train(gradient_steps)` as ONE call: examples/td3_train_step.py with its inner loop
(buf.sample, td.target, cg.backward, fo.critic_step and, every policy_delay-th update, ag.backward, fo.actor_step(polyak=True),
td.refresh) replaced by `tr.train(gradient_steps)` of FusedOffPolicyTrain, which enqueues the same launches in the same order
from one C call and leaves SB3's logs (train/critic_loss, train/actor_loss when an actor step ran, train/n_updates) on the
device.  `_n_updates` carries the delay across calls as SB3's does.

The model is an SB3-shaped stand-in (actor.mu ending in Tanh, actor_target, critic.q_networks, critic_target, the two
optimisers, tau, batch_size, policy_delay) with the reference's TD3 architecture (MlpPolicy, ReLU, net_arch [256, 256];
rl/baselines/RL_Mesh.py:206-222), random-initialised: SB3 is not installed in this image.  The replay buffer is filled by a
stochastic behaviour policy (a random-initialised FusedActor): TD3 is off-policy, and the rollout is not what this example is about.

    python examples/td3_train.py [--envs 4096] [--chunk 32] [--iterations 20] [--gradient-steps 8] [--batch 100]
                                 [--policy-delay 2] [--check]

--check runs the composition of examples/td3_train_step.py on a deep-copied twin with the same seeds and counters and prints
how many parameter, Adam-moment and step tensors differ in any bit after the last step (0 is expected).
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

GAMMA, TAU, SEED = 0.99, 0.005, 1


def mlp(sizes, tail=None):
    import torch
    mods = []
    for i in range(len(sizes) - 2):
        mods += [torch.nn.Linear(sizes[i], sizes[i + 1]), torch.nn.ReLU()]
    return torch.nn.Sequential(*mods, torch.nn.Linear(sizes[-2], sizes[-1]), *([tail] if tail else []))


def td3_model(torch, batch, policy_delay):
    actor = torch.nn.Module()
    actor.mu = mlp([18, 256, 256, 3], torch.nn.Tanh())
    critic = torch.nn.Module()
    critic.q_networks = torch.nn.ModuleList([mlp([21, 256, 256, 1]) for _ in range(2)])
    actor.cuda(), critic.cuda()
    actor_target, critic_target = copy.deepcopy(actor), copy.deepcopy(critic)
    actor.optimizer = torch.optim.Adam(actor.parameters(), lr=3e-4)
    critic.optimizer = torch.optim.Adam(critic.parameters(), lr=3e-4)
    return types.SimpleNamespace(actor=actor, actor_target=actor_target, critic=critic, critic_target=critic_target, gamma=GAMMA, tau=TAU,
                                 target_policy_noise=0.2, target_noise_clip=0.5, batch_size=batch, policy_delay=policy_delay, _n_updates=0)


def tensors(model):
    """Every parameter, then every Adam moment and step of the two optimisers."""
    out = [*model.actor.parameters(), *model.actor_target.parameters(), *model.critic.parameters(), *model.critic_target.parameters()]
    for opt in (model.critic.optimizer, model.actor.optimizer):
        out += [st[k] for st in opt.state.values() for k in ("exp_avg", "exp_avg_sq", "step")]
    return out


class Composition:
    """The loop of examples/td3_train_step.py on a twin."""

    def __init__(self, model, buf):
        from reinforcementlearning4meshgeneration_amd import FusedCriticGrad, FusedOptimStep, FusedTD3ActorGrad, FusedTDTarget
        self.model, self.buf = model, buf
        self.td, self.cg = FusedTDTarget.from_sb3(model), FusedCriticGrad.from_sb3(model)
        self.ag, self.fo = FusedTD3ActorGrad.from_sb3(model), FusedOptimStep.from_sb3(model)

    def train(self, gradient_steps, counter):
        m = self.model
        for k in range(gradient_steps):
            m._n_updates += 1
            s = self.buf.sample(m.batch_size, seed=SEED, counter=counter + k)
            y = self.td.target(s, seed=SEED, counter=counter + k)
            self.cg.backward(s, y)
            self.fo.critic_step()
            if m._n_updates % m.policy_delay == 0:
                self.ag.backward(s)
                self.fo.actor_step(polyak=True)
                self.td.refresh()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--chunk", type=int, default=32, help="vector steps per rollout call")
    ap.add_argument("--iterations", type=int, default=20)
    ap.add_argument("--gradient-steps", type=int, default=8)
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--buffer-size", type=int, default=1_000_000)
    ap.add_argument("--policy-delay", type=int, default=2)
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    import torch

    from reinforcementlearning4meshgeneration_amd import DeviceReplayBuffer, FusedActor, FusedOffPolicyTrain, MeshVecEnv, boundary
    torch.manual_seed(999)
    model = td3_model(torch, args.batch, args.policy_delay)
    env = MeshVecEnv([boundary(0)], n_envs=args.envs)
    buf = DeviceReplayBuffer(env, buffer_size=args.buffer_size)
    twin = Composition(copy.deepcopy(model), buf) if args.check else None
    tr = FusedOffPolicyTrain.from_sb3(model, buf)
    behaviour = FusedActor.from_torch([torch.nn.Linear(18, 128), torch.nn.Linear(128, 128), torch.nn.Linear(128, 128)],
                                      torch.nn.Linear(128, 3), torch.nn.Linear(128, 3))
    T = args.chunk
    obs0 = env.reset().clone()
    actions = behaviour.sample(obs0, 999, 0)
    draw, logs = 1, []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.iterations):
        out = env.step_actor_T(behaviour, actions, T, seed=999, counter=draw, want_terminal_obs=True)
        buf.add_rollout(out, obs0=obs0)
        obs0, actions, draw = out["obs"][T - 1].clone(), out["actions"][T], draw + T
        counter = tr.counter
        logs.append(tr.train(args.gradient_steps, seed=SEED))               # TD3.train(gradient_steps): one C call, nothing read back
        if twin:
            twin.train(args.gradient_steps, counter)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    result = {"workload": f"{args.envs} envs of boundary(0), {args.iterations} x ({T} vector steps, one train() of {args.gradient_steps} "
                          f"gradient steps at batch {args.batch}, policy_delay {args.policy_delay})", "seconds": dt,
              "gradient_steps_per_s": model._n_updates / dt, "c_calls": tr.calls, "first_logs": logs[0].read(), "last_logs": logs[-1].read(),
              "stored": buf.size() * args.envs}
    if args.check:
        pairs = list(zip(tensors(model), tensors(twin.model)))
        result["tensors_compared"] = len(pairs)
        result["tensors_differing_in_any_bit"] = sum(not torch.equal(a.detach().cpu(), b.detach().cpu()) for a, b in pairs)
    print(json.dumps(result))
    tr.close()
    behaviour.close()
    env.close()


if __name__ == "__main__":
    main()
