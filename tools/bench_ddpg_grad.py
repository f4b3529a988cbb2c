"""DDPG's two fused gradient statements (FusedDDPGGrad.critic_backward / actor_backward: three launches each, k_wgrad_*_rows,
k_wgrad_weights, k_wgrad_reduce) against the eager torch statements of SB3's TD3.train on the same modules and batch:

    critic: q = critic(cat(obs, actions)); loss = F.mse_loss(q, y); critic.optimizer.zero_grad(); loss.backward()
    actor:  loss = -critic(cat(obs, actor(obs))).mean();             actor.optimizer.zero_grad();  loss.backward()

    python tools/bench_ddpg_grad.py [--rounds 7] [--reps 20] [--out profiles/ddpg_grad_bench.json]

At B = 100, 256, 4096, 65 536 and for both statements: fused and eager are timed in the same process in interleaved rounds
(fused, eager, fused, eager, ...), `reps` CUDA-event pairs each per round after a warm-up call; the medians and the
interquartile ranges are over all rounds' samples.  Host overhead and output allocation are included on both sides.  Eager's
actor statement also accumulates into the critic's .grad, which is part of what the statement costs there.  There is no
fused predecessor: eager torch is the yardstick.  Before anything is timed the two are asserted to agree within twice the
fp64 bound of tests/ddpg_grad_ref.py at every size.  One JSON line per row.  The gate: at B = 100, 256 and 4096 the fused
median is not above the eager median, for both statements; B = 65 536 is reported without a gate.  The exit status is 1 if
the gate fails.  Then a summary line with the library's source hash (tools/source_state.py).  Kernel durations come from a
separate rocprofv3 --kernel-trace --stats run of this script (the program after --; never with --pmc)."""
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


def samples(torch, fn, reps):
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
    return ms


def stats(ms):
    q1, med, q3 = np.percentile(ms, [25, 50, 75])
    return float(med), float(q3 - q1)


def agree(name_pairs, ref, B, statement):
    worst = 0.0
    for name, a, b in name_pairs:
        bound = ref[name][1]
        d = np.abs(a.detach().cpu().numpy().astype(np.float64) - b.detach().cpu().numpy().astype(np.float64)).reshape(bound.shape)
        assert (d <= 2.0 * bound).all(), (statement, B, name)
        worst = max(worst, float((d / np.maximum(2.0 * bound, 1e-300)).max()))
    return worst


def measure(rounds, reps):
    import torch
    import torch.nn.functional as F

    import ddpg_grad_ref as G
    import ddpg_ref as D
    import policy_ref as R
    from reinforcementlearning4meshgeneration_amd import FusedDDPGGrad
    obs_rows = R.input_rows()
    m = G.model()
    mf, me = (G.attach_optimizers(D.to_cuda(copy.deepcopy(m))) for _ in range(2))
    lin = lambda seq: [l for l in seq if type(l).__name__ == "Linear"]   # noqa: E731
    params = lambda seq: [p for l in lin(seq) for p in (l.weight, l.bias)]   # noqa: E731
    dg = FusedDDPGGrad.from_sb3(mf)
    mu_e, q_e = me.actor.mu, me.critic.q_networks[0]

    rows = []
    for B in BATCHES:
        obs_np, act_np, y_np = G.batch(B, obs_rows)
        obs, act, y = (torch.from_numpy(x).cuda() for x in (obs_np, act_np, y_np))
        y2 = y.reshape(B, 1)

        def critic_eager():
            loss = F.mse_loss(q_e(torch.cat([obs, act], dim=1)), y2)
            me.critic.optimizer.zero_grad()
            loss.backward()
            return loss

        def actor_eager():
            loss = -q_e(torch.cat([obs, mu_e(obs)], dim=1)).mean()
            me.actor.optimizer.zero_grad()
            loss.backward()
            return loss

        calls = {"critic": (lambda: dg.critic_backward(observations=obs, actions=act, target_q_values=y), critic_eager),
                 "actor": (lambda: dg.actor_backward(observations=obs), actor_eager)}
        # ---- agreement first, at every size
        loss, parts = dg.critic_backward(observations=obs, actions=act, target_q_values=y, return_parts=True)
        ref, info = G.critic_grad(m, obs_np, act_np, y_np, other_acts=[a.cpu().numpy() for a in parts["acts1"]])
        G.assert_critic_conditions(info, f"critic B={B}")
        loss_e = critic_eager()
        pairs = [("critic_loss", loss, loss_e)] + [(n, p.grad, q.grad) for n, p, q in zip(G.CRITIC_GRADS, params(mf.critic.q_networks[0]), params(q_e))]
        worst = {"critic": agree(pairs, ref, B, "critic")}
        loss, parts = dg.actor_backward(observations=obs, return_parts=True)
        ref, info = G.actor_grad(m, obs_np, other={k: [a.cpu().numpy() for a in parts[k]] for k in ("acts", "acts1")})
        G.assert_actor_conditions(info, f"actor B={B}")
        loss_e = actor_eager()
        pairs = [("actor_loss", loss, loss_e)] + [(n, p.grad, q.grad) for n, p, q in zip(G.ACTOR_GRADS, params(mf.actor.mu), params(mu_e))]
        worst["actor"] = agree(pairs, ref, B, "actor")
        del ref, info, parts
        # ---- interleaved rounds
        ms = {(s, side): [] for s in calls for side in ("fused", "eager")}
        for _ in range(rounds):
            for s, (fused, eager) in calls.items():
                ms[(s, "fused")] += samples(torch, fused, reps)
                ms[(s, "eager")] += samples(torch, eager, reps)
        for s in calls:
            (t_f, iqr_f), (t_e, iqr_e) = stats(ms[(s, "fused")]), stats(ms[(s, "eager")])
            row = dict(statement=s, batch=B, fused_ms=t_f, fused_iqr_ms=iqr_f, eager_ms=t_e, eager_iqr_ms=iqr_e, eager_over_fused=t_e / t_f,
                       samples=rounds * reps, gated=B in GATED, gate_fused_not_above_eager=(t_f <= t_e) if B in GATED else None,
                       max_fused_minus_eager_over_twice_the_bound=worst[s])
            print(json.dumps(row), flush=True)
            rows.append(row)
    dg.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from source_state import state
    rows = measure(args.rounds, args.reps)
    ok = all(r["gate_fused_not_above_eager"] for r in rows if r["gated"])
    summary = dict(summary="bench_ddpg_grad", **state(), gate_holds_at_100_256_4096=ok, rows=rows)
    print(json.dumps(summary), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(summary, f, indent=1)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
