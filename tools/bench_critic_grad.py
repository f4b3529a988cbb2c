"""The fused critic update (FusedCriticGrad.backward: one k_critic_grad and one k_critic_grad_reduce launch) against the
eager torch statements of SB3's SAC.train / TD3.train on the same modules and batch:

    qin = torch.cat([obs, actions], dim=1)
    loss = 0.5 * sum(F.mse_loss(q(qin), y) for q in critic);  opt.zero_grad();  loss.backward()

    python tools/bench_critic_grad.py [--reps 50] [--out FILE]

For SAC (ReLU [128, 128, 128]) and TD3 (ReLU [256, 256]) at B = 100, 256, 4096, 65 536: the median milliseconds of `reps`
CUDA-event pairs after a warm-up call of (a) cg.backward(...) and (b) the eager statements, zero_grad() included.  Host
overhead and output allocation are included on both sides.  Before anything is timed the two are asserted to agree: every
gradient element and the loss within 2 x bound of each other (tests/critic_grad_ref.py; both are fp32 evaluations within one
bound of fp64).  One JSON line per shape.  The gate: at B = 100, 256 and 4096, the batch sizes the recipes train at, the median
of (a) is not above the median of (b); B = 65 536 is reported without a gate.  The exit status is 1 if the gate fails.  Then a
summary line with the library's source hash (tools/source_state.py).  Kernel durations come from a rocprofv3 --kernel-trace
--stats run of this script."""
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

    import critic_grad_ref as G
    import policy_ref as R
    from reinforcementlearning4meshgeneration_amd.critic_grad import FusedCriticGrad
    obs_rows = R.input_rows()
    rows = []
    for kind in ("sac", "td3"):
        m = G.critic_modules(kind)
        cuda = lambda: {c: [copy.deepcopy(l).cuda() for l in m[c]] for c in ("q1", "q2")}   # noqa: E731
        mf, me = cuda(), cuda()
        nets = [torch.nn.Sequential(*[x for l in me[c][:-1] for x in (l, torch.nn.ReLU())], me[c][-1]) for c in ("q1", "q2")]
        pf = [p for c in ("q1", "q2") for l in mf[c] for p in (l.weight, l.bias)]
        pe = [p for c in ("q1", "q2") for l in me[c] for p in (l.weight, l.bias)]
        names = ["q%d.%s%d" % (c, n, i) for c in (1, 2) for i in range(len(m["q1"])) for n in ("w", "b")]
        opt = torch.optim.Adam(pe, lr=3e-4)
        cg = (FusedCriticGrad.sac if kind == "sac" else FusedCriticGrad.td3)(mf["q1"], mf["q2"])
        for B in BATCHES:
            obs_np, act_np, y_np = G.batch(B, obs_rows)
            obs, act = torch.from_numpy(obs_np).cuda(), torch.from_numpy(act_np).cuda()
            y = torch.from_numpy(y_np).cuda().reshape(-1, 1)

            def fused():
                return cg.backward(observations=obs, actions=act, target_q_values=y)

            def eager():
                qin = torch.cat([obs, act], dim=1)
                loss = 0.5 * sum(torch.nn.functional.mse_loss(q(qin), y) for q in nets)
                opt.zero_grad()
                loss.backward()
                return loss

            # agreement first: test 5's criterion of tests/test_gpu_critic_grad.py
            loss_f, parts = cg.backward(observations=obs, actions=act, target_q_values=y, return_parts=True)
            loss_e = eager()
            acts = {1: [a.cpu().numpy() for a in parts["acts1"]], 2: [a.cpu().numpy() for a in parts["acts2"]]}
            ref, info = G.critic_grad(m, obs_np, act_np, y_np, other_acts=acts)
            G.assert_share(info, f"{kind} B={B}")
            worst = 0.0
            for name, a, b in [("loss", loss_f, loss_e)] + [(n, p.grad, q.grad) for n, p, q in zip(names, pf, pe)]:
                bound = ref[name][1]
                d = np.abs(a.detach().cpu().numpy().astype(np.float64) - b.detach().cpu().numpy().astype(np.float64)).reshape(bound.shape)
                assert (d <= 2.0 * bound).all(), (kind, B, name)
                worst = max(worst, float((d / np.maximum(bound, 1e-300)).max()))
            t_f, t_e = timed(torch, fused, reps), timed(torch, eager, reps)
            row = dict(kind=kind, batch=B, fused_ms=t_f, eager_ms=t_e, eager_over_fused=t_e / t_f, gated=B in GATED,
                       gate_fused_not_above_eager=(t_f <= t_e) if B in GATED else None,
                       max_fused_minus_eager_over_bound=worst, ambiguous_pairs=info["ambiguous_pairs"])
            print(json.dumps(row), flush=True)
            rows.append(row)
        cg.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from source_state import state
    rows = measure(args.reps)
    ok = all(r["gate_fused_not_above_eager"] for r in rows if r["gated"])
    summary = dict(summary="bench_critic_grad", **state(), gate_holds_at_100_256_4096=ok, rows=rows)
    print(json.dumps(summary), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(summary, f, indent=1)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
