#!/usr/bin/env python
"""Meshing 4096 random domains with the supervised network for 64 moves (general/EBRD.py:541-548), done three ways in one run:

  (a) device     MeshVecEnv.mesh_with(FusedFNN, max_steps=64, check_every=64): one call enqueues 64 x (k_fnn_forward, the launches
                 of meshenv_move under the finished mask, k_fnn_advance); one read of finished.all() at the end
  (b) hand       the loop (a) replaces, written against the API as it was: per move the eager torch module (seven Linear layers
                 on the GPU), argmax, two dtype conversions, venv.move, and -- because move() has neither an auto-reset nor a
                 mask -- a read of done / code to the host and the finished / steps bookkeeping in numpy.  A finished env cannot
                 be frozen this way: it keeps being moved, its bookkeeping alone stops.
  (c) hand_blind (b) without the read-back and the bookkeeping: launches only.  Not a usable loop (nobody knows which env
                 finished when); the floor of what any host loop over the old API costs.

The three are interleaved round by round after warm-up rounds, each from reset(static=True) (inside the timed region for all of
them); a figure is the median of ROUNDS host-clock times around work that ends in a device synchronise, its spread the
interquartile range.  No ratio is required of this bench: nobody had measured either side.

Separately, untimed by the host clock: the forward kernel's own time from the handle's events (set_timing(1) brackets every
k_fnn_forward launch of a mesh_with call), and its share of the (a) loop.

Before anything is timed (a) and (b) are compared: the moves-to-finish of every env.  They may differ where the eager forward
and the kernel round an action differently and a validity check flips; the fraction of envs that agree is reported.

    python tools/bench_fnn_mesh.py [--out profiles/fnn_mesh_bench.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from reinforcementlearning4meshgeneration_amd import FusedFNN, MeshVecEnv  # noqa: E402

N_ENVS, MOVES, ROUNDS, WARMUP, SEED = 4096, 64, 11, 3, 1
LAYERS = (("fc1", 18, 64), ("fc2", 64, 128), ("fc3", 128, 64), ("fc4", 64, 32), ("fc5", 32, 16), ("action_head", 16, 2),
          ("type_head", 16, 3))


class Policy(torch.nn.Module):
    """The reference's network shape, default initialisation, the action bias at a point move() accepts now and then."""

    def __init__(self):
        super().__init__()
        for name, n_in, n_out in LAYERS:
            setattr(self, name, torch.nn.Linear(n_in, n_out))
        with torch.no_grad():
            self.action_head.bias.copy_(torch.tensor([0.25, 0.85]))

    def forward(self, x):
        for fc in (self.fc1, self.fc2, self.fc3, self.fc4, self.fc5):
            x = torch.relu(fc(x))
        return self.action_head(x), self.type_head(x)


def iqr(xs):
    q = statistics.quantiles(xs, n=4)
    return q[2] - q[0]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fnn_mesh_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_fnn_mesh needs a ROCm GPU: there is no CPU fallback")
    from source_state import state
    torch.manual_seed(SEED)
    module = Policy().eval()
    fnn = FusedFNN.from_module(module)
    module = module.cuda()
    env = MeshVecEnv.from_random(N_ENVS, seed=5000, auto_reset=False, log_capacity=512)
    out = {}

    def device():
        out["device"] = env.mesh_with(fnn, max_steps=MOVES, check_every=MOVES)

    def hand(poll=True):
        obs = env.reset(static=True)
        finished, steps = np.zeros(N_ENVS, bool), np.zeros(N_ENVS, np.int32)
        with torch.no_grad():
            for _ in range(MOVES):
                action, type_values = module(obs)
                types = torch.argmax(type_values, dim=1).double() / 2
                obs, done, _, code = env.move(action.double(), types)
                if poll:
                    ended = (done.cpu().numpy() != 0) | (code.cpu().numpy() >= 2)
                    steps += ~finished
                    finished |= ended
        out["hand" if poll else "hand_blind"] = (finished, steps)

    fns = dict(device=device, hand=hand, hand_blind=lambda: hand(False))
    for _ in range(WARMUP):
        for f in fns.values():
            f()
    res, (h_finished, h_steps) = out["device"], out["hand"]
    d_finished, d_steps = res.finished.cpu().numpy() != 0, res.steps.cpu().numpy()
    agree = float(((d_finished == h_finished) & (d_steps == h_steps)).mean())
    ms = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, f in fns.items():
            ms[k].append(timed(f))
    # the forward kernel alone: every k_fnn_forward launch of one mesh_with call between two events
    env.set_timing(1)
    device()
    fwd = env.kernel_times_ms() * 1e3
    env.set_timing(0)
    med = {k: statistics.median(v) for k, v in ms.items()}
    spread = {k: iqr(v) for k, v in ms.items()}
    fwd_us = float(np.median(fwd))
    row = dict(n_envs=N_ENVS, moves=MOVES, rounds=ROUNDS, warmup=WARMUP,
               **{f"{k}_ms": round(med[k], 3) for k in ms}, **{f"{k}_iqr_ms": round(spread[k], 3) for k in ms},
               **{f"{k}_ms_min_max": [round(min(v), 3), round(max(v), 3)] for k, v in ms.items()},
               hand_over_device=round(med["hand"] / med["device"], 3), hand_blind_over_device=round(med["hand_blind"] / med["device"], 3),
               device_faster_than_hand_beyond_both_iqr=bool(med["hand"] - med["device"] > spread["hand"] + spread["device"]),
               device_faster_than_hand_blind_beyond_both_iqr=bool(med["hand_blind"] - med["device"] > spread["hand_blind"] + spread["device"]),
               forward_launches_timed=int(len(fwd)), forward_us_median=round(fwd_us, 2),
               forward_us_min_max=[round(float(fwd.min()), 2), round(float(fwd.max()), 2)],
               forward_share_of_device_loop=round(fwd_us * MOVES / (med["device"] * 1e3), 4),
               envs_finished_device=int(d_finished.sum()), envs_finished_hand=int(h_finished.sum()),
               envs_with_equal_steps_and_finished=round(agree, 5), elements_device=int(res.n_elements.sum()))
    print(json.dumps(row), flush=True)
    summary = dict(summary="bench_fnn_mesh", device=torch.cuda.get_device_name(0), **state(),
                   not_measured=["kernel trace of the move launches", "the training half (train_ch3)"], results=[row])
    with open(args.out, "w") as fh:
        json.dump(summary, fh, indent=1)
        fh.write("\n")
    print(json.dumps(dict(summary="bench_fnn_mesh", out=os.path.relpath(args.out, ROOT))), flush=True)
    env.close()


if __name__ == "__main__":
    main()
