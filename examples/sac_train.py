#!/usr/bin/env python
"""SAC training with the whole of `SAC.train(gradient_steps)` as ONE call: examples/sac_train_step.py with its inner loop
(buf.sample, td.target, cg.backward, fo.critic_step, ag.backward, fo.actor_step, td.refresh per gradient step) replaced by
`tr.train(gradient_steps)` of FusedOffPolicyTrain, which enqueues the same launches in the same order from one C call and
leaves SB3's logs (train/critic_loss, train/actor_loss, train/ent_coef, train/ent_coef_loss, train/n_updates) on the device.

The model is an SB3-shaped stand-in (actor.latent_pi / .mu / .log_std, critic.q_networks, critic_target, log_ent_coef, the
three optimisers, tau, batch_size, target_update_interval) with the reference's architecture (MlpPolicy, ReLU, net_arch
[128, 128, 128]; rl/baselines/RL_Mesh.py:183-196), random-initialised: SB3 is not installed in this image.

    python examples/sac_train.py [--envs 4096] [--chunk 32] [--iterations 20] [--gradient-steps 8] [--batch 100]
                                 [--target-update-interval 1] [--check]

--check runs the composition of examples/sac_train_step.py on a deep-copied twin with the same seeds and counters and prints
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


def mlp(sizes):
    import torch
    mods = []
    for i in range(len(sizes) - 2):
        mods += [torch.nn.Linear(sizes[i], sizes[i + 1]), torch.nn.ReLU()]
    return torch.nn.Sequential(*mods, torch.nn.Linear(sizes[-2], sizes[-1]))


def sac_model(torch, batch, interval):
    actor = torch.nn.Module()
    actor.latent_pi = torch.nn.Sequential(*[m for i in range(3) for m in (torch.nn.Linear(18 if i == 0 else 128, 128), torch.nn.ReLU())])
    actor.mu, actor.log_std = torch.nn.Linear(128, 3), torch.nn.Linear(128, 3)
    critic = torch.nn.Module()
    critic.q_networks = torch.nn.ModuleList([mlp([21, 128, 128, 128, 1]) for _ in range(2)])
    actor.cuda(), critic.cuda()
    actor.optimizer = torch.optim.Adam(actor.parameters(), lr=3e-4)
    critic.optimizer = torch.optim.Adam(critic.parameters(), lr=3e-4)
    log_ent_coef = torch.zeros(1, device="cuda", requires_grad=True)
    return types.SimpleNamespace(actor=actor, critic=critic, critic_target=copy.deepcopy(critic), log_ent_coef=log_ent_coef,
                                 ent_coef_optimizer=torch.optim.Adam([log_ent_coef], lr=3e-4), target_entropy=-3.0, gamma=GAMMA, tau=TAU,
                                 batch_size=batch, target_update_interval=interval, _n_updates=0)


def tensors(model):
    """Every parameter, then every Adam moment and step of the three optimisers."""
    out = [*model.actor.parameters(), *model.critic.parameters(), *model.critic_target.parameters(), model.log_ent_coef]
    for opt in (model.critic.optimizer, model.actor.optimizer, model.ent_coef_optimizer):
        out += [st[k] for st in opt.state.values() for k in ("exp_avg", "exp_avg_sq", "step")]
    return out


class Composition:
    """The loop of examples/sac_train_step.py on a twin."""

    def __init__(self, model, buf):
        from reinforcementlearning4meshgeneration_amd import FusedActorGrad, FusedCriticGrad, FusedOptimStep, FusedTDTarget
        self.model, self.buf = model, buf
        self.td, self.cg = FusedTDTarget.from_sb3(model), FusedCriticGrad.from_sb3(model)
        self.ag, self.fo = FusedActorGrad.from_sb3(model), FusedOptimStep.from_sb3(model)

    def train(self, gradient_steps, counter):
        m = self.model
        for k in range(gradient_steps):
            s = self.buf.sample(m.batch_size, seed=SEED, counter=counter + k)
            y = self.td.target(s, seed=SEED, counter=counter + k)
            self.cg.backward(s, y)
            self.fo.critic_step()
            self.ag.backward(s, seed=SEED, counter=counter + k)
            self.fo.actor_step(polyak=k % m.target_update_interval == 0)
            self.td.refresh()
        m._n_updates += gradient_steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--chunk", type=int, default=32, help="vector steps per rollout call")
    ap.add_argument("--iterations", type=int, default=20)
    ap.add_argument("--gradient-steps", type=int, default=8)
    ap.add_argument("--batch", type=int, default=100)
    ap.add_argument("--buffer-size", type=int, default=1_000_000)
    ap.add_argument("--target-update-interval", type=int, default=1)
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    import torch

    from reinforcementlearning4meshgeneration_amd import DeviceReplayBuffer, FusedActor, FusedOffPolicyTrain, MeshVecEnv, boundary
    torch.manual_seed(999)
    model = sac_model(torch, args.batch, args.target_update_interval)
    lin = [m for m in model.actor.latent_pi if isinstance(m, torch.nn.Linear)]
    env = MeshVecEnv([boundary(0)], n_envs=args.envs)
    buf = DeviceReplayBuffer(env, buffer_size=args.buffer_size)
    twin = Composition(copy.deepcopy(model), buf) if args.check else None
    tr = FusedOffPolicyTrain.from_sb3(model, buf)
    actor = FusedActor.from_torch(lin, model.actor.mu, model.actor.log_std)      # the rollout actor (host-packed once)
    T = args.chunk
    obs0 = env.reset().clone()
    actions = actor.sample(obs0, 999, 0)
    draw, logs = 1, []
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.iterations):
        out = env.step_actor_T(actor, actions, T, seed=999, counter=draw, want_terminal_obs=True)
        buf.add_rollout(out, obs0=obs0)
        obs0, actions, draw = out["obs"][T - 1].clone(), out["actions"][T], draw + T
        counter = tr.counter
        logs.append(tr.train(args.gradient_steps, seed=SEED))               # SAC.train(gradient_steps): one C call, nothing read back
        if twin:
            twin.train(args.gradient_steps, counter)
        actor.close()
        actor = FusedActor.from_torch(lin, model.actor.mu, model.actor.log_std)   # the rollout follows the trained actor
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    result = {"workload": f"{args.envs} envs of boundary(0), {args.iterations} x ({T} vector steps, one train() of {args.gradient_steps} "
                          f"gradient steps at batch {args.batch})", "seconds": dt, "gradient_steps_per_s": model._n_updates / dt,
              "c_calls": tr.calls, "first_logs": logs[0].read(), "last_logs": logs[-1].read(), "stored": buf.size() * args.envs}
    if args.check:
        pairs = list(zip(tensors(model), tensors(twin.model)))
        result["tensors_compared"] = len(pairs)
        result["tensors_differing_in_any_bit"] = sum(not torch.equal(a.detach().cpu(), b.detach().cpu()) for a, b in pairs)
    print(json.dumps(result))
    tr.close()
    actor.close()
    env.close()


if __name__ == "__main__":
    main()
