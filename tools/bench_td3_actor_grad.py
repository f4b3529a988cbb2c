"""The fused TD3 / DDPG actor-loss statement (FusedTD3ActorGrad.backward: one k_td3_actor_grad and one
k_td3_actor_grad_reduce launch) against the eager torch statements of SB3's TD3.train on the same modules and batch:

    actor_loss = -critic.q1_forward(obs, actor(obs)).mean();  actor.optimizer.zero_grad();  actor_loss.backward()

    python tools/bench_td3_actor_grad.py [--reps 50] [--out FILE]

At B = 100, 256, 4096, 65 536: the median milliseconds of `reps` CUDA-event pairs after a warm-up call of (a)
ag.backward(observations=obs) and (b) the eager statements, zero_grad() included.  Host overhead and output allocation are
included on both sides.  Eager also accumulates into the critic's .grad, which is part of what the statement costs there.
There is no fused predecessor: eager torch is the yardstick.  Before anything is timed the two are asserted to agree at the
gated sizes: test 4's criterion of tests/test_gpu_td3_actor_grad.py (2 x bound).  One JSON line per shape.  The gate: at
B = 100, 256 and 4096 the median of (a) is not above the median of (b); B = 65 536 is reported without a gate (and without
the fp64 reference): the two workgroups of a tile set both run the forward pass there.  The exit status is 1 if the gate
fails.  Then a summary line with the library's source hash (tools/source_state.py).  Kernel durations come from a
rocprofv3 --kernel-trace --stats run of this script."""
import argparse
import copy
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

BATCHES = [100, 256, 4096, 65536]
GATED = (100, 256, 4096)


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


def measure(reps):
    import torch

    import policy_ref as R
    import td3_actor_grad_ref as A
    from reinforcementlearning4meshgeneration_amd.td3_actor_grad import FusedTD3ActorGrad
    obs_rows = R.input_rows()
    m = A.modules()

    def cuda():
        d = {k: [copy.deepcopy(l).cuda() for l in m[k]] for k in ("lin", "q1")}
        d["mu"] = copy.deepcopy(m["mu"]).cuda()
        return d
    mf, me = cuda(), cuda()
    actor_params = lambda d: [p for l in (*d["lin"], d["mu"]) for p in (l.weight, l.bias)]   # noqa: E731
    pf, pe = actor_params(mf), actor_params(me)
    opt_a = torch.optim.Adam(pe, lr=3e-4)
    ag = FusedTD3ActorGrad.td3(mf["lin"], mf["mu"], mf["q1"])

    def eager_loss(obs):
        h = obs
        for l in me["lin"]:
            h = torch.relu(l(h))
        hc = torch.cat([obs, torch.tanh(me["mu"](h))], dim=1)
        for l in me["q1"][:-1]:
            hc = torch.relu(l(hc))
        return -me["q1"][-1](hc).mean()

    rows = []
    for B in BATCHES:
        obs_np, _ = A.batch(B, obs_rows)
        obs = torch.from_numpy(obs_np).cuda()

        def fused():
            return ag.backward(observations=obs)

        def eager():
            loss = eager_loss(obs)
            opt_a.zero_grad()
            loss.backward()
            return loss

        worst, info = None, None
        if B in GATED:       # agreement first
            loss, parts = ag.backward(observations=obs, return_parts=True)
            hp = {k: [a.cpu().numpy() for a in parts[k]] for k in ("acts", "acts1")}
            ref, info = A.td3_actor_grad(m, obs_np, other=hp)
            A.assert_conditions(info, f"B={B}")
            for p in pe:
                p.grad = None
            loss_e = eager_loss(obs)
            loss_e.backward()
            worst = 0.0
            for name, a, b in [("actor_loss", loss, loss_e)] + [(n, p.grad, q.grad) for n, p, q in zip(A.GRADS, pf, pe)]:
                bound = ref[name][1]
                d = np.abs(a.detach().cpu().numpy().astype(np.float64) - b.detach().cpu().numpy().astype(np.float64)).reshape(bound.shape)
                assert (d <= 2.0 * bound).all(), (B, name)
                worst = max(worst, float((d / np.maximum(2.0 * bound, 1e-300)).max()))
        t_f, t_e = timed(torch, fused, reps), timed(torch, eager, reps)
        row = dict(kind="td3", batch=B, fused_ms=t_f, eager_ms=t_e, eager_over_fused=t_e / t_f, gated=B in GATED,
                   gate_fused_not_above_eager=(t_f <= t_e) if B in GATED else None, max_fused_minus_eager_over_twice_the_bound=worst,
                   ambiguous=A.describe(info) if info else None)
        print(json.dumps(row), flush=True)
        rows.append(row)
    ag.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from source_state import state
    rows = measure(args.reps)
    ok = all(r["gate_fused_not_above_eager"] for r in rows if r["gated"])
    summary = dict(summary="bench_td3_actor_grad", **state(), gate_holds_at_100_256_4096=ok, rows=rows)
    print(json.dumps(summary), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(summary, f, indent=1)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
