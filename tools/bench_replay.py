"""The device replay buffer (DeviceReplayBuffer: one k_replay_add / k_replay_sample launch per call) against the eager torch
composition a user would write today on the same data: six [rows, n, .] tensors, torch.where(done, terminal_obs, obs_after)
and slice copy_ for add, six advanced-index gathers and the dones * (1 - timeouts) product for sample.

    python tools/bench_replay.py [--reps 50] [--out FILE] [--variant-lib LIB]

Shapes: add at T = 1, 32, 128 x 4096 envs; sample at B = 100, 256, 4096, 65 536 from a 10^6-transition buffer (244 rows) and
from one whose records pass 256 MiB (512 rows: beyond L2 and Infinity Cache).  Before anything is timed the eager results are
asserted equal, bit for bit, to the kernels' on the same indices.  One JSON line per shape: median milliseconds by CUDA events
around each call after a warm-up call (host overhead and output allocation included on both sides), the algorithmic bytes
(add: 166 read + 4 R written per transition; sample: 4 R read + 164 written + 8 of indices per sample) and the fraction of
5.65 TB/s (random whole rows, gathered once) they imply -- context, not a gate.  The gate: at every shape the fused median is
not above the eager median; the exit status is 1 otherwise.  --variant-lib runs the same measurement first in a child
process on another build of the library (MESHENV_LIB; the other record size R) and records its rows next to these.  Then a
summary line with the library's source hash (tools/source_state.py).  Kernel durations come from a
rocprofv3 --kernel-trace --stats run of this script (k_replay_add / k_replay_sample rows)."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

N_ENVS = 4096
ADD_T = [1, 32, 128]
SAMPLE_B = [100, 256, 4096, 65536]
BUFFERS = [("1e6_transitions", 1_000_000 // N_ENVS), ("beyond_256MiB", 512)]   # 512 rows: 384 MiB at R = 48, 512 MiB at 64
RANDOM_ROW_BYTES_PER_S = 5.65e12


def timed(torch, fn, reps):
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


class Eager:
    """SB3's layout on the device and the torch calls a user would write around it."""

    def __init__(self, torch, rows, n):
        f32 = dict(dtype=torch.float32, device="cuda")
        self.torch = torch
        self.obs, self.next = torch.zeros((rows, n, 18), **f32), torch.zeros((rows, n, 18), **f32)
        self.act = torch.zeros((rows, n, 3), **f32)
        self.rew, self.done, self.tout = (torch.zeros((rows, n), **f32) for _ in range(3))

    def load(self, buf):
        for mine, theirs in ((self.obs, buf.observations), (self.next, buf.next_observations), (self.act, buf.actions),
                             (self.rew, buf.rewards), (self.done, buf.dones), (self.tout, buf.timeouts)):
            mine.copy_(theirs)

    def add(self, pos, d, obs0):
        t = self.torch
        T = d["done"].shape[0]
        self.obs[pos].copy_(obs0)
        if T > 1:
            self.obs[pos + 1:pos + T].copy_(d["obs"][:T - 1])
        done = d["done"] != 0
        self.next[pos:pos + T].copy_(t.where(done[:, :, None], d["terminal_obs"], d["obs"]))
        self.act[pos:pos + T].copy_(d["actions"][:T])
        self.rew[pos:pos + T].copy_(d["reward"])
        self.done[pos:pos + T].copy_(done)
        self.tout[pos:pos + T].copy_(done & (d["complete"] == 0))

    def sample(self, b, e):
        return (self.obs[b, e], self.act[b, e], self.next[b, e], (self.done[b, e] * (1 - self.tout[b, e])).reshape(-1, 1),
                self.rew[b, e].reshape(-1, 1))

    def fields(self):
        return (self.obs, self.next, self.act, self.rew, self.done, self.tout)


def same_bits(torch, x, y):
    return x.shape == y.shape and torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))


def measure(reps):
    import torch

    import replay_ref
    from reinforcementlearning4meshgeneration_amd import DeviceReplayBuffer
    from reinforcementlearning4meshgeneration_amd.domains import boundary
    from reinforcementlearning4meshgeneration_amd.vec_env import MeshVecEnv
    env = MeshVecEnv([boundary(0)], n_envs=N_ENVS)
    rows_out = []
    R = env._L.meshenv_replay_record_floats()

    def emit(row):
        row = dict(record_floats=R, **row)
        row["fused_over_eager"] = round(row["fused_ms"] / row["eager_ms"], 3)
        row["eager_over_fused"] = round(row["eager_ms"] / row["fused_ms"], 2)
        row["achieved_TBps"] = round(row["bytes"] / (row["fused_ms"] * 1e-3) / 1e12, 3)
        row["fraction_of_random_row_rate"] = round(row["bytes"] / (row["fused_ms"] * 1e-3) / RANDOM_ROW_BYTES_PER_S, 3)
        row["gate_fused_not_above_eager"] = bool(row["fused_ms"] <= row["eager_ms"])
        print(json.dumps(row), flush=True)
        rows_out.append(row)

    # ---- add: T vector steps into a 10^6-transition buffer, unscaled actions on both sides
    rows = BUFFERS[0][1]
    buf = DeviceReplayBuffer(env, buffer_size=rows * N_ENVS)
    eager = Eager(torch, rows, N_ENVS)
    for T in ADD_T:
        h = replay_ref.synthetic(T, N_ENVS, seed=T, special=False)
        d = dict(actions=np.concatenate([h["actions"], h["actions"][:1]]), obs=h["obs_after"], reward=h["reward"], done=h["done"],
                 complete=h["complete"], terminal_obs=h["terminal_obs"])
        d = {k: torch.from_numpy(v).cuda() for k, v in d.items()}
        obs0 = torch.from_numpy(h["obs0"]).cuda()
        pos = 7

        def fused():
            buf.pos = pos
            buf.add_rollout(d, obs0=obs0, scale_actions=False)

        fused()
        eager.add(pos, d, obs0)
        mine = (buf.observations, buf.next_observations, buf.actions, buf.rewards, buf.dones, buf.timeouts)
        assert all(same_bits(torch, x[pos:pos + T], y[pos:pos + T]) for x, y in zip(mine, eager.fields())), f"add T={T}"
        f_ms, e_ms = timed(torch, fused, reps), timed(torch, lambda: eager.add(pos, d, obs0), reps)
        emit(dict(op="add", T=T, envs=N_ENVS, rows=rows, fused_ms=round(f_ms, 4), eager_ms=round(e_ms, 4),
                  bytes=T * N_ENVS * (166 + 4 * R)))
    del buf, eager

    # ---- sample: B transitions from a full buffer of random records
    for name, rows in BUFFERS:
        buf = DeviceReplayBuffer(env, buffer_size=rows * N_ENVS)
        g = torch.Generator(device="cuda")
        g.manual_seed(rows)
        buf.store.normal_(generator=g)
        flag = torch.rand((rows, N_ENVS), device="cuda", generator=g)
        buf.dones.copy_(flag < 0.1)
        buf.timeouts.copy_(flag < 0.05)
        buf.full = True
        eager = Eager(torch, rows, N_ENVS)
        eager.load(buf)
        for B in SAMPLE_B:
            got, b32, e32 = buf.sample(B, seed=3, counter=B, return_indices=True)
            b, e = b32.long(), e32.long()          # the index tensors torch's gathers want, made outside the timed region
            want = eager.sample(b, e)
            assert all(same_bits(torch, x, y) for x, y in zip(got, want)), f"sample {name} B={B}"
            assert all(same_bits(torch, x, y) for x, y in zip(buf.gather(b32, e32, check=False), want)), f"gather {name} B={B}"
            f_ms = timed(torch, lambda: buf.sample(B, seed=3, counter=B), reps)
            e_ms = timed(torch, lambda: eager.sample(b, e), reps)
            emit(dict(op="sample", B=B, envs=N_ENVS, rows=rows, buffer=name, store_MiB=round(rows * N_ENVS * R * 4 / 2 ** 20, 1),
                      fused_ms=round(f_ms, 4), eager_ms=round(e_ms, 4), bytes=B * (4 * R + 164 + 8)))
        del buf, eager
        torch.cuda.empty_cache()
    env.close()
    return rows_out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--variant-lib", default=None, help="another build of the library (the other record size), measured first")
    ap.add_argument("--rows-only", action="store_true", help="print the rows as one JSON list and nothing else (the child)")
    args = ap.parse_args()
    variant = None
    if args.variant_lib:       # a fresh process: one process loads one library
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--reps", str(args.reps), "--rows-only"],
                               env=dict(os.environ, MESHENV_LIB=os.path.abspath(args.variant_lib)), capture_output=True, text=True,
                               timeout=900)
        if child.returncode not in (0, 1):
            sys.stderr.write(child.stdout[-2000:] + child.stderr[-2000:])
            raise SystemExit(f"the variant run failed ({child.returncode})")
        variant = json.loads(child.stdout.strip().splitlines()[-1])
    if args.rows_only:
        devnull, stdout = open(os.devnull, "w"), sys.stdout
        sys.stdout = devnull
        try:
            rows = measure(args.reps)
        finally:
            sys.stdout = stdout
        print(json.dumps(rows), flush=True)
        sys.exit(0 if all(r["gate_fused_not_above_eager"] for r in rows) else 1)
    from source_state import state
    rows = measure(args.reps)
    ok = all(r["gate_fused_not_above_eager"] for r in rows)
    summary = dict(summary="bench_replay", **state(), gate_holds_at_every_shape=ok, rows=rows)
    if variant is not None:
        summary["variant_library"] = os.path.relpath(os.path.abspath(args.variant_lib), ROOT)
        summary["variant_rows"] = variant
    print(json.dumps(summary), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(summary, f, indent=1)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
