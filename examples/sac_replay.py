#!/usr/bin/env python
"""The data path of an SAC training loop with nothing leaving the GPU: the fused SAC actor in the loop on 4096 envs
(step_actor_T), its transitions stored in a DeviceReplayBuffer (add_rollout: what SB3's _store_transition +
ReplayBuffer.add do, with SAC's action scaling), and batches drawn from it (sample: SB3's ReplayBuffer.sample) at the
reference's batch size (rl/baselines/RL_Mesh.py:183-196: batch_size=100) and at 4096.  The gradient step itself is the
user's (torch); this example stops at the ReplayBufferSamples it would consume.

The actor is the reference's architecture (MlpPolicy, ReLU, net_arch [128, 128, 128]), random-initialised with seed 999:
SB3 is not installed in this image and there is no checkpoint to load.

    python examples/sac_replay.py [--envs 4096] [--chunk 32] [--chunks 40] [--buffer-size 1000000]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--chunk", type=int, default=32, help="vector steps per step_actor_T / add_rollout call")
    ap.add_argument("--chunks", type=int, default=40)
    ap.add_argument("--buffer-size", type=int, default=1_000_000)
    ap.add_argument("--batches", type=int, default=200)
    args = ap.parse_args()
    import torch

    from reinforcementlearning4meshgeneration_amd import DeviceReplayBuffer, FusedActor, MeshVecEnv, boundary
    torch.manual_seed(999)
    lin = [torch.nn.Linear(18, 128), torch.nn.Linear(128, 128), torch.nn.Linear(128, 128)]
    actor = FusedActor.from_torch(lin, torch.nn.Linear(128, 3), torch.nn.Linear(128, 3))
    env = MeshVecEnv([boundary(0)], n_envs=args.envs)
    buf = DeviceReplayBuffer(env, buffer_size=args.buffer_size)
    T, n = args.chunk, args.envs
    obs0 = env.reset().clone()                       # what the first action is chosen on (the calls overwrite env.obs)
    actions = actor.sample(obs0, 999, 0)
    draw = 1

    def chunk():
        nonlocal obs0, actions, draw
        out = env.step_actor_T(actor, actions, T, seed=999, counter=draw, want_terminal_obs=True)
        buf.add_rollout(out, obs0=obs0)              # Box actions -> [-1, 1] as SAC stores them; one launch
        obs0, actions, draw = out["obs"][T - 1].clone(), out["actions"][T], draw + T

    chunk()                                          # warm-up
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.chunks):
        chunk()
    torch.cuda.synchronize()
    dt_roll = time.perf_counter() - t0
    # the store alone, on the last chunk's histories
    out = env.step_actor_T(actor, actions, T, seed=999, counter=draw, want_terminal_obs=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.chunks):
        buf.add_rollout(out, obs0=obs0)
    torch.cuda.synchronize()
    dt_add = time.perf_counter() - t0
    result = {"workload": f"{n} envs of boundary(0), fused SAC actor 18-128-128-128-3, {T} vector steps per call, buffer of "
                          f"{buf.buffer_size} rows x {n} envs ({buf.record_floats * 4} B records)",
              "rollout_and_store_transitions_per_s": args.chunks * T * n / dt_roll,
              "store_alone_transitions_per_s": args.chunks * T * n / dt_add, "stored": buf.size() * n}
    for B in (100, 4096):
        batch = buf.sample(B, seed=1, counter=0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(args.batches):
            batch = buf.sample(B, seed=1, counter=1 + k)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        result[f"sample_{B}_transitions_per_s"] = args.batches * B / dt
        result[f"sample_{B}_us_per_batch"] = 1e6 * dt / args.batches
    result["last_batch"] = {k: list(getattr(batch, k).shape) for k in batch._fields}
    result["non_terminal_fraction_of_last_batch"] = float((batch.dones == 0).float().mean())
    print(json.dumps(result))
    actor.close()
    env.close()


if __name__ == "__main__":
    main()
