"""Policy evaluation on the device (MeshVecEnv.evaluate: policy, step and k_eval_tally per vector step, one C call) against
(b) collect_rollout / step_actor_T for the same policy and number of steps and (c) the SB3-shaped host loop --
SB3MeshVecEnv.step, FusedPolicy.forward / FusedActor.forward, evaluate_policy's bookkeeping in numpy and
element_quality('last') on the steps where an env is done.

    python tools/bench_eval.py [--envs 4096] [--host-steps 300] [--out FILE]

Workloads: 4096 x boundary() and 4096 from_random envs (log_capacity 256, quality on), a deterministic TD3-kind policy
([256, 256] ReLU) and the SAC actor ([128, 128, 128]), one episode per env.  Host clock around synchronised work (median of
three runs after a warm-up); env-steps/s = vector steps x envs / s, episodes/s = recorded episodes / s.  The host loop runs
--host-steps steps (or until every env has its episode) and its rate is per step.  One JSON line per workload and a summary
line with the library's source hash (tools/source_state.py).  k_eval_tally durations come from a separate rocprofv3
--kernel-trace --stats run of this script."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

LOW = np.array([-1.0, -1.5, 0.0]); HIGH = np.array([1.0, 1.5, 1.5])
MEAN = np.array([0.0, 0.6, 0.75])


def _scaled(x):
    return (x - LOW) / (HIGH - LOW) * 2 - 1


def td3_policy(torch):
    from reinforcementlearning4meshgeneration_amd.policy import FusedPolicy
    torch.manual_seed(0)
    H = 256
    head = torch.nn.Linear(H, 3)
    with torch.no_grad():
        head.weight.mul_(0.3); head.bias.copy_(torch.tensor(np.arctanh(_scaled(MEAN))))
    return FusedPolicy.deterministic([torch.nn.Linear(18, H), torch.nn.Linear(H, H)], head, activation="relu")


def sac_actor(torch):
    from reinforcementlearning4meshgeneration_amd.actor import FusedActor
    torch.manual_seed(1)
    lin = [torch.nn.Linear(18, 128), torch.nn.Linear(128, 128), torch.nn.Linear(128, 128)]
    mu, ls = torch.nn.Linear(128, 3), torch.nn.Linear(128, 3)
    with torch.no_grad():
        mu.weight.mul_(0.3); mu.bias.copy_(torch.tensor(np.arctanh(_scaled(MEAN))))
    return FusedActor.from_torch(lin, mu, ls)


def make_env(kind, n, cls=None):
    from reinforcementlearning4meshgeneration_amd import MeshVecEnv, boundary
    cls = cls or MeshVecEnv
    if kind == "boundary":
        return cls([boundary(0)], n_envs=n, log_capacity=256)
    return cls.from_random(n, seed=11, log_capacity=256)


def timed(torch, fn, reps=3):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0, r))
    out.sort(key=lambda x: x[0])
    return out[len(out) // 2]


def host_loop(torch, kind, n, pol, steps):
    """evaluate_policy's loop around SB3MeshVecEnv (numpy per step) with the fused forward and element_quality('last')."""
    from reinforcementlearning4meshgeneration_amd.actor import FusedActor
    from reinforcementlearning4meshgeneration_amd.vec_env import SB3MeshVecEnv
    env = make_env(kind, n, SB3MeshVecEnv)
    targets = np.ones(n, int)
    counts = np.zeros(n, int)
    cur = np.zeros(n); length = np.zeros(n, int)
    rewards_out, lengths_out, quality = [], [], []
    obs = env.reset()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    t = 0
    while (counts < targets).any() and t < steps:
        o = torch.from_numpy(obs).cuda()
        act = pol.forward(o) if isinstance(pol, FusedActor) else pol.forward(o, deterministic=True)["actions"]
        obs, rew, dones, infos = env.step(act.cpu().numpy())
        cur += rew; length += 1
        if dones.any():
            _, stats, _ = env.element_quality("last", per_element=False)
            stats = stats.cpu().numpy()
        for i in range(n):
            if counts[i] < targets[i] and dones[i]:
                rewards_out.append(cur[i]); lengths_out.append(length[i]); quality.append(stats[i]); counts[i] += 1
                cur[i] = 0; length[i] = 0
        t += 1
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    env.close()
    return dict(steps=t, seconds=dt, env_steps_per_s=t * n / dt, episodes=len(rewards_out), episodes_per_s=len(rewards_out) / dt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--host-steps", type=int, default=300)
    ap.add_argument("--max-steps", type=int, default=2000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from source_state import state
    n = args.envs
    lines = []
    for pname, mk in (("td3", td3_policy), ("sac", sac_actor)):
        pol = mk(torch)
        for kind in ("boundary", "random"):
            env = make_env(kind, n)
            dt, res = timed(torch, lambda: env.evaluate(pol, episodes_per_env=1, max_steps=args.max_steps, check_every=32))
            T = res.steps
            if pname == "td3":
                dt_roll, _ = timed(torch, lambda: (env.reset(), env.collect_rollout(pol, T, deterministic=True)))
            else:
                dt_roll, _ = timed(torch, lambda: (env.reset(), env.step_actor_T(pol, pol.forward(env.obs), T, sample=False)))
            env.close()
            host = host_loop(torch, kind, n, pol, args.host_steps)
            row = dict(workload=f"evaluate_{pname}_{kind}", envs=n, steps=T, episodes=len(res), finished=res.finished,
                       complete=int(res.complete.sum()), mean_reward=res.mean_reward,
                       evaluate_s=dt, evaluate_env_steps_per_s=T * n / dt, evaluate_episodes_per_s=len(res) / dt,
                       rollout_s=dt_roll, rollout_env_steps_per_s=T * n / dt_roll,
                       evaluate_over_rollout=(T * n / dt) / (T * n / dt_roll),
                       host_loop=host, evaluate_over_host_loop=(T * n / dt) / host["env_steps_per_s"])
            print(json.dumps(row), flush=True)
            lines.append(row)
        pol.close()
    summary = dict(summary=True, source=state(), gpu=torch.cuda.get_device_name(0))
    print(json.dumps(summary), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(rows=lines, **summary), f, indent=1)


if __name__ == "__main__":
    main()
