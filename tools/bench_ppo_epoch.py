#!/usr/bin/env python
"""One epoch of PPO.train / A2C.train, rows = n_envs x n_steps, composed two ways on twin models in the same run:

  (a) fused   rb.get(batch_size): ONE k_rollout_gather launch, then per minibatch FusedPPOGrad.backward(view) + FusedOptimStep.policy_step()
  (b) stock   the composition of the example before DeviceRolloutBuffer: torch.randperm, five flat[k][idx] per minibatch,
              FusedPPOGrad.backward, the stock torch policy.optimizer.step()

for PPO ReLU [128, 128] at batch 256 with Adam(eps=1e-5) and for SB3's default A2C, Tanh [64, 64], full batch, with
RMSprop(alpha=0.99, eps=1e-5), at rows 2048, 8192 and 65 536.  (a) and (b) are interleaved epoch by epoch after a warm-up; a
figure is the median of PAIRS CUDA-event pairs, host overhead included on both sides.  The loss gradient is the same kernel
on both sides: the difference is the gathers and the optimiser step.  Before anything is timed, the gathered fields are
asserted equal to torch's indexing and one policy_step() within twice the fp64 bound of one stock step.

Also: the median microseconds of the gather launch alone (4-byte pieces, and the 8-byte variant of the observations) against
torch's five whole-epoch index operations, and of policy_step() against optimizer.step(), per recipe.

The gate: (a) is not slower than (b) at every size for both recipes; the exit status is 1 when it fails (the file is written
first).  No ratio is fixed in advance.

    python tools/bench_ppo_epoch.py [--out profiles/ppo_epoch_bench.json] [--trace-only N]
    --trace-only N: no timing; N gathers and N policy steps per recipe and nothing else (the run a kernel trace is taken from)"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import on_policy_stubs as S  # noqa: E402
import optim_step_ref as O  # noqa: E402
import policy_ref as R  # noqa: E402
import ppo_grad_ref as P  # noqa: E402
import rmsprop_ref as Q  # noqa: E402
from reinforcementlearning4meshgeneration_amd import DeviceRolloutBuffer, FusedOptimStep, FusedPPOGrad  # noqa: E402

ROWS, N_STEPS, PAIRS, WARMUP, MICRO_PAIRS = (2048, 8192, 65536), 32, 15, 3, 200
RECIPES = {"ppo": dict(batch_size=256), "a2c": dict(batch_size=None)}
GATHERED = ("obs", "buffer_actions", "log_prob", "advantages", "returns")      # what the parent's loop indexed per minibatch


def rollout(kind, rows):
    """[T][n] histories on the device from tests/ppo_grad_ref.py's batch rows (no environment is needed to time an epoch)."""
    T, n = N_STEPS, rows // N_STEPS
    d = P.batch(P.modules(S.RECIPES[kind]), rows, R.input_rows())
    host = {"obs": d["observations"].reshape(T, n, 18), "buffer_actions": d["actions"].reshape(T, n, 3),
            "value": d["returns"].reshape(T, n) * np.float32(0.5), "log_prob": d["old_log_prob"].reshape(T, n),
            "advantages": d["advantages"].reshape(T, n), "returns": d["returns"].reshape(T, n)}
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in host.items()}


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def interleaved(fns, pairs, warmup):
    """Median milliseconds of each of fns, called in turn `pairs` times after `warmup` rounds."""
    for _ in range(warmup):
        for f in fns:
            f()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(pairs):
        for i, f in enumerate(fns):
            ms[i].append(timed(f))
    return [statistics.median(x) for x in ms]


class Side:
    def __init__(self, kind):
        self.kind = kind
        self.model, self.params = S.model(kind, "cuda")
        self.opt = self.model.policy.optimizer
        self.pg = FusedPPOGrad.from_sb3(self.model)
        self.hp = dict(clip_range=None if kind == "a2c" else 0.2, ent_coef=0.0, vf_coef=0.5, normalize_advantage=kind == "ppo",
                       max_grad_norm=0.5)

    def close(self):
        self.pg.close()


def agreement(kind, f, s, fo, rb, out):
    """The gathered fields against torch's indexing (equal), one policy_step against one stock step (twice the bound)."""
    rows = out["returns"].numel()
    perm = torch.randperm(rows, device="cuda")
    got = next(iter(rb.get(None, perm=perm)))
    flat = {k: v.transpose(0, 1).reshape(rows, *v.shape[2:]) for k, v in out.items()}
    for x, k in zip(got, ("obs", "buffer_actions", "value", "log_prob", "advantages", "returns")):
        assert torch.equal(x, flat[k][perm]), k
    mb = next(iter(rb.get(256, perm=perm)))
    for side in (f, s):
        side.pg.backward(mb, **side.hp)
    host = lambda x: x.detach().cpu().numpy().copy()   # noqa: E731
    before = [(host(p), host(p.grad)) for p in f.params]
    fo.policy_step()
    s.opt.step()
    worst = 0.0
    for p, q, (p0, g) in zip(f.params, s.params, before):
        z = np.zeros_like(p0)
        ref = Q.rmsprop(p0, z, g, Q.scalars())["p"] if kind == "a2c" else O.adam(p0, z, z, g, O.scalars(1, lr=3e-4, eps=1e-5))["p"]
        d = np.abs(host(p).astype(np.float64) - host(q))
        assert (d <= 2.0 * ref[1]).all(), kind
        worst = max(worst, float((d[ref[1] > 0] / ref[1][ref[1] > 0]).max()))
    return worst


def measure():
    results, micro = [], []
    for kind, cfg in RECIPES.items():
        for rows in ROWS:
            f, s = Side(kind), Side(kind)
            fo, rb = FusedOptimStep.from_sb3(f.model), DeviceRolloutBuffer()
            out = rollout(kind, rows)
            rb.load(out)
            worst = agreement(kind, f, s, fo, rb, out)
            batch = cfg["batch_size"] or rows
            flat = {k: out[k].reshape(rows, *out[k].shape[2:]) for k in GATHERED}

            def fused():
                for mb in rb.get(cfg["batch_size"]):
                    f.pg.backward(mb, **f.hp)
                    fo.policy_step()

            def stock():
                perm = torch.randperm(rows, device="cuda")
                for start in range(0, rows, batch):
                    idx = perm[start:start + batch]
                    s.pg.backward(observations=flat["obs"][idx], actions=flat["buffer_actions"][idx], old_log_prob=flat["log_prob"][idx],
                                  advantages=flat["advantages"][idx], returns=flat["returns"][idx], **s.hp)
                    s.opt.step()

            binds, launches = fo.binds, rb.launches
            t_f, t_s = interleaved([fused, stock], PAIRS, WARMUP)
            assert fo.binds == binds and rb.launches == launches + PAIRS + WARMUP, "the steady state uploaded a table or gathered twice"
            assert all(bool(torch.isfinite(p).all()) for p in f.params + s.params)
            row = dict(recipe=kind, rows=rows, batch_size=batch, minibatches=-(-rows // batch), fused_epoch_ms=round(t_f, 4),
                       stock_epoch_ms=round(t_s, 4), stock_over_fused=round(t_s / t_f, 3), gate_fused_not_slower=t_f <= t_s,
                       max_step_difference_over_bound=round(worst, 4))
            print(json.dumps(row), flush=True)
            results.append(row)
            # ---- the two new launches alone, each against its torch counterpart
            perm = torch.randperm(rows, device="cuda")
            g4, g8, gt = interleaved([lambda: rb._gather(perm, 0), lambda: rb._gather(perm, 1), lambda: [flat[k][perm] for k in GATHERED]],
                                     MICRO_PAIRS, 10)
            mb = next(iter(rb.get(cfg["batch_size"], perm=perm)))
            for side in (f, s):
                side.pg.backward(mb, **side.hp)
            torch.cuda.synchronize()
            st_f, st_s = interleaved([fo.policy_step, s.opt.step], MICRO_PAIRS, 10)
            m = dict(recipe=kind, rows=rows, optimizer=type(f.opt).__name__, gather_us=round(1e3 * g4, 2), gather_obs_8_byte_us=round(1e3 * g8, 2),
                     torch_five_index_ops_us=round(1e3 * gt, 2), policy_step_us=round(1e3 * st_f, 2), torch_optimizer_step_us=round(1e3 * st_s, 2))
            print(json.dumps(m), flush=True)
            micro.append(m)
            fo.close(); rb.close(); f.close(); s.close()
    return results, micro


def trace_only(n):
    for kind, cfg in RECIPES.items():
        f = Side(kind)
        fo, rb = FusedOptimStep.from_sb3(f.model), DeviceRolloutBuffer()
        rb.load(rollout(kind, 8192))
        perm = torch.randperm(8192, device="cuda")
        f.pg.backward(next(iter(rb.get(cfg["batch_size"], perm=perm))), **f.hp)
        torch.cuda.synchronize()
        for _ in range(n):
            rb._gather(perm, 0)
            rb._gather(perm, 1)
            fo.policy_step()
        torch.cuda.synchronize()
        print(json.dumps(dict(recipe=kind, rows=8192, gathers=2 * n, policy_steps=n, uploads=fo.binds)), flush=True)
        fo.close(); rb.close(); f.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppo_epoch_bench.json"))
    ap.add_argument("--trace-only", type=int, default=0, metavar="N")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_ppo_epoch needs a ROCm GPU: there is no CPU fallback")
    if args.trace_only:
        return trace_only(args.trace_only)
    from source_state import state
    results, micro = measure()
    ok = all(r["gate_fused_not_slower"] for r in results)
    summary = dict(summary="bench_ppo_epoch", device=torch.cuda.get_device_name(0), pairs=PAIRS, warmup=WARMUP, micro_pairs=MICRO_PAIRS,
                   n_steps=N_STEPS, **state(), gate_holds=ok, results=results, launches=micro)
    with open(args.out, "w") as fh:
        json.dump(summary, fh, indent=1)
        fh.write("\n")
    print(json.dumps(dict(summary="bench_ppo_epoch", gate_holds=ok, out=os.path.relpath(args.out, ROOT))), flush=True)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
