#!/usr/bin/env python
"""FusedPPOGrad.backward against the eager torch statement (evaluate_actions, losses, zero_grad, backward, clip_grad_norm_) on
the same modules in the same run: medians of 50 CUDA-event pairs, host overhead and output allocation included on both
sides, the two interleaved call by call after a warm-up, agreement within twice the fp64 bound asserted first.
Writes profiles/ppo_grad_bench.json.  The gate: fused not above eager at B = 64, 256 and 4096 (65 536 is reported only); the
exit status is 1 when it fails (the file is written first).

    python tools/bench_ppo_grad.py [--out profiles/ppo_grad_bench.json] [--trace-only]   (--trace-only: calls for rocprofv3)"""
import argparse
import copy
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import policy_ref as R  # noqa: E402
import ppo_grad_ref as P  # noqa: E402
from reinforcementlearning4meshgeneration_amd.ppo_grad import FusedPPOGrad  # noqa: E402

SIZES, GATED, PAIRS, WARMUP = (64, 256, 4096, 65536), (64, 256, 4096), 50, 10


def cuda(m):
    d = {k: v for k, v in m.items() if k in ("act", "H", "a2c")}
    d.update(pi=[copy.deepcopy(l).cuda() for l in m["pi"]], vf=[copy.deepcopy(l).cuda() for l in m["vf"]],
             action_net=copy.deepcopy(m["action_net"]).cuda(), value_net=copy.deepcopy(m["value_net"]).cuda(),
             log_std=torch.nn.Parameter(m["log_std"].detach().clone().cuda()))
    return d


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ppo_grad_bench.json"))
    ap.add_argument("--trace-only", action="store_true")
    args = ap.parse_args()
    rows, results = R.input_rows(), []
    for case in P.BOTH_SETS:
        m = P.modules(case)
        mc, me = cuda(m), cuda(m)
        pg = FusedPPOGrad.actor_critic(mc["pi"], mc["vf"], mc["action_net"], mc["value_net"], mc["log_std"], mc["act"])
        hp = P.hyper(clip_range=None if m["a2c"] else 0.2, max_grad_norm=0.5)
        for B in SIZES:
            data = P.batch(m, B, rows)
            dd = {k: torch.from_numpy(v).cuda() for k, v in data.items()}
            fused = lambda: pg.backward(observations=dd["observations"], actions=dd["actions"], old_log_prob=dd["old_log_prob"],   # noqa: E731
                                        advantages=dd["advantages"], returns=dd["returns"], **hp)
            eager = lambda: P.eager(torch, me, dd, hp)   # noqa: E731
            if args.trace_only:
                for _ in range(PAIRS):
                    fused()
                torch.cuda.synchronize()
                continue
            res, e = fused(), eager()
            worst = 0.0
            if B <= 4096:      # agreement first, within twice the fp64 bound (the reference is host fp64: skipped at 65 536)
                ref, _ = P.ppo_grad(m, data, hp)
                got = dict({k: p.grad for k, p in zip(P.GRADS, P.params(mc))}, loss=res["loss"])
                for k in (*P.GRADS, "loss"):
                    d = np.abs(got[k].detach().cpu().numpy().astype(np.float64).reshape(np.shape(ref[k][0])) - e[k].cpu().numpy().reshape(np.shape(ref[k][0])))
                    r = float((d / np.maximum(2.0 * np.asarray(ref[k][1]), 1e-300)).max())
                    assert r <= 1.0, (case, B, k, r)
                    worst = max(worst, r)
            for _ in range(WARMUP):
                fused(); eager()
            torch.cuda.synchronize()
            tf, te = [], []
            for _ in range(PAIRS):                        # interleaved: both sides see the same clocks and cache state
                tf.append(timed(fused)); te.append(timed(eager))
            f_ms, e_ms = statistics.median(tf), statistics.median(te)
            results.append(dict(case=case, B=B, fused_ms=round(f_ms, 4), eager_ms=round(e_ms, 4), eager_over_fused=round(e_ms / f_ms, 2),
                                gated=B in GATED, gate_holds=bool(f_ms <= e_ms), agreement_over_twice_bound=round(worst, 4)))
            print(json.dumps(results[-1]))
        pg.close()
    if not args.trace_only:
        gate = all(r["gate_holds"] for r in results if r["gated"])
        with open(args.out, "w") as f:
            json.dump(dict(device=torch.cuda.get_device_name(0), pairs=PAIRS, warmup=WARMUP, gate_holds=gate, results=results), f, indent=1)
        print(json.dumps(dict(gate_holds=gate)))
        if not gate:
            sys.exit("the gate fails: fused above eager at " + ", ".join(f"{r['case']} B={r['B']}" for r in results if r["gated"] and not r["gate_holds"]))


if __name__ == "__main__":
    main()
