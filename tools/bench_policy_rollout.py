"""Closed-loop rollout throughput with the fused PPO / A2C / TD3 policies (MeshVecEnv.collect_rollout: a policy launch and a
step launch per vector step, one C call per T steps) beside the SAC actor's step_actor_T, at 4096 envs of boundary() and of
the d1 domain (boundary16), plus the policy forward alone (FusedPolicy.sample back to back).

    python tools/bench_policy_rollout.py [--envs 4096] [--T 128] [--reps 5] [--out FILE]

One JSON line per configuration, then a summary line with the library's source hash (tools/source_state.py).  Kernel
durations come from a rocprofv3 --kernel-trace --stats run of this script (k_policy_forward<H, act, kind> rows)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

CASES = {"ppo": ("actor_critic", 128, "relu"), "a2c": ("actor_critic", 64, "tanh"), "td3": ("deterministic", 256, "relu")}


def make_policy(torch, case):
    from reinforcementlearning4meshgeneration_amd.policy import FusedPolicy
    kind, H, act = CASES[case]
    torch.manual_seed(999)
    tower = lambda: [torch.nn.Linear(18, H), torch.nn.Linear(H, H)]   # noqa: E731
    if kind == "actor_critic":
        head = torch.nn.Linear(H, 3)
        with torch.no_grad():
            head.weight.mul_(6.0)   # actions spread over the rule types, as in the closed-loop tests
        return FusedPolicy.actor_critic(tower(), tower(), head, torch.nn.Linear(H, 1), torch.full((3,), -0.5), activation=act)
    mu = torch.nn.Linear(H, 3)
    with torch.no_grad():
        mu.weight.mul_(6.0)
    return FusedPolicy.deterministic(tower(), mu, activation=act, sigma=0.1)


def make_sac(torch):
    from reinforcementlearning4meshgeneration_amd.actor import FusedActor
    torch.manual_seed(999)
    lin = [torch.nn.Linear(18, 128), torch.nn.Linear(128, 128), torch.nn.Linear(128, 128)]
    mu, ls = torch.nn.Linear(128, 3), torch.nn.Linear(128, 3)
    with torch.no_grad():
        mu.weight.mul_(6.0)
        ls.bias.fill_(-0.5)
    return FusedActor.from_torch(lin, mu, ls)


def domain(name):
    from reinforcementlearning4meshgeneration_amd.domains import boundary
    if name == "boundary":
        return list(boundary(0))
    tr = np.load(os.path.join(ROOT, "tests", "golden", "boundary16_biased_s2.npz"))
    return [tuple(p) for p in tr["domain_xy"]]


def timed(torch, fn, reps):
    """median milliseconds of fn() over reps (after one warm-up call), CUDA events around each call"""
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--T", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--forward-calls", type=int, default=200)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    from reinforcementlearning4meshgeneration_amd.vec_env import MeshVecEnv
    from source_state import state
    n, T = args.envs, args.T
    rows = []
    for dom in ("boundary", "d1"):
        for case in ("sac", *CASES):
            env = MeshVecEnv([domain(dom)], n_envs=n, auto_reset=True)
            if case == "sac":
                pol = make_sac(torch)
                acts = [torch.zeros((n, 3), device=env.device)]

                def run():
                    out = env.step_actor_T(pol, acts[0], T, seed=1, counter=run.k)
                    acts[0] = out["actions"][T]
                    run.k += T
            else:
                pol = make_policy(torch, case)

                def run():
                    env.collect_rollout(pol, T, seed=1, counter=run.k)
                    run.k += T
            run.k = 0
            ms = timed(torch, run, args.reps)
            row = dict(case=case, domain=dom, envs=n, T=T, us_per_vector_step=round(1e3 * ms / T, 3),
                       env_steps_per_s=round(n * T / (ms / 1e3), 1))
            if case != "sac":   # the policy launch alone, back to back (includes the per-call host overhead)
                obs = env.obs.clone()
                k = args.forward_calls

                def fwd():
                    for i in range(k):
                        pol.sample(obs, 1, i)
                row["us_per_policy_call"] = round(1e3 * timed(torch, fwd, 3) / k, 3)
            print(json.dumps(row), flush=True)
            rows.append(row)
            pol.close()
            env.close()
    summary = dict(summary="bench_policy_rollout", **state(), rows=rows)
    print(json.dumps(summary), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(summary, f, indent=1)


if __name__ == "__main__":
    main()
