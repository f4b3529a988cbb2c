"""The fused SAC actor / entropy-coefficient statement (FusedActorGrad.backward: one k_actor_grad and one
k_actor_grad_reduce launch) against the eager torch statements of SB3's SAC.train on the same modules and batch:

    actions_pi, log_prob = actor.action_log_prob(obs);  ent_coef = th.exp(log_ent_coef.detach())
    ent_coef_loss = -(log_ent_coef * (log_prob + target_entropy).detach()).mean()
    min_qf_pi = th.min(th.cat(critic(obs, actions_pi), dim=1), dim=1, keepdim=True)[0]
    actor_loss = (ent_coef * log_prob - min_qf_pi).mean();  actor_opt.zero_grad();  actor_loss.backward()

    python tools/bench_actor_grad.py [--reps 50] [--out FILE]

At B = 100, 256, 4096, 65 536: the median milliseconds of `reps` CUDA-event pairs after a warm-up call of (a)
ag.backward(obs, seed=..., counter=...) and (b) the eager statements, zero_grad() included; the noise is drawn inside the timed
region on both sides, as SB3 does (Philox in the kernel; torch.randn_like for eager).  Host overhead and output allocation are
included on both sides.  Eager also accumulates into the critics' .grad, which is part of what the statement costs there.
Before anything is timed the two are asserted to agree on a shared eps at the gated sizes: test 6's criterion of
tests/test_gpu_actor_grad.py (2 x bound plus the allowance for eager's uncancelled pair).  One JSON line per shape.  The
gate: at B = 100, 256 and 4096 the median of (a) is not above the median of (b); B = 65 536 is reported without a gate (and
without the fp64 reference).  The exit status is 1 if the gate fails.  Then a summary line with the library's source hash
(tools/source_state.py).  Kernel durations come from a rocprofv3 --kernel-trace --stats run of this script."""
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
LEC = -0.5


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

    import actor_grad_ref as A
    import policy_ref as R
    import td_target_ref as T
    from reinforcementlearning4meshgeneration_amd.actor_grad import FusedActorGrad
    obs_rows = R.input_rows()
    m = T.sac_modules()

    def cuda():
        d = {k: [copy.deepcopy(l).cuda() for l in m[k]] for k in ("lin", "q1", "q2")}
        d.update(mu=copy.deepcopy(m["mu"]).cuda(), ls=copy.deepcopy(m["ls"]).cuda(),
                 lec=torch.full((1,), LEC, device="cuda", requires_grad=True))
        return d
    mf, me = cuda(), cuda()
    actor_params = lambda d: [p for l in (*d["lin"], d["mu"], d["ls"]) for p in (l.weight, l.bias)]   # noqa: E731
    pf, pe = actor_params(mf) + [mf["lec"]], actor_params(me) + [me["lec"]]
    names = list(A.GRADS) + ["ent.grad"]
    opt_a, opt_e = torch.optim.Adam(pe[:-1], lr=3e-4), torch.optim.Adam(pe[-1:], lr=3e-4)
    ag = FusedActorGrad.sac(mf["lin"], mf["mu"], mf["ls"], mf["q1"], mf["q2"], log_ent_coef=mf["lec"])

    def eager_losses(obs, eps):
        h = obs
        for l in me["lin"]:
            h = torch.relu(l(h))
        mean, std = me["mu"](h), torch.clamp(me["ls"](h), -20.0, 2.0).exp()
        g = mean + std * eps
        a = torch.tanh(g)
        lp = (torch.distributions.Normal(mean, std).log_prob(g).sum(dim=1) - torch.log(1.0 - a ** 2 + 1e-6).sum(dim=1)).reshape(-1, 1)
        ent_coef = torch.exp(me["lec"].detach())
        le = -(me["lec"] * (lp - 3.0).detach()).mean()
        x = torch.cat([obs, a], dim=1)
        qs = []
        for c in ("q1", "q2"):
            hc = x
            for l in me[c][:-1]:
                hc = torch.relu(l(hc))
            qs.append(me[c][-1](hc))
        return (ent_coef * lp - torch.min(torch.cat(qs, dim=1), dim=1, keepdim=True)[0]).mean(), le

    rows, step = [], [0]
    for B in BATCHES:
        obs_np, eps_np = A.batch(B, obs_rows)
        obs, eps = torch.from_numpy(obs_np).cuda(), torch.from_numpy(eps_np).cuda()

        def fused():
            step[0] += 1
            return ag.backward(observations=obs, seed=5, counter=step[0])

        def eager():
            la, le = eager_losses(obs, torch.randn_like(eps))
            opt_e.zero_grad()
            le.backward()
            opt_a.zero_grad()
            la.backward()
            return la, le

        worst, info = None, None
        if B in GATED:       # agreement first, on a shared eps
            la, le, parts = ag.backward(observations=obs, noise=eps, return_parts=True)
            hp = {k: parts[k].cpu().numpy() for k in A.PARTS}
            hp.update({k: [a.cpu().numpy() for a in parts[k]] for k in ("acts", "acts1", "acts2")})
            ref, info = A.actor_grad(m, obs_np, eps_np, log_ent_coef=LEC, other=hp)
            A.assert_conditions(info, f"B={B}")
            for p in pe:
                p.grad = None
            la_e, le_e = eager_losses(obs, eps)
            la_e.backward()
            le_e.backward()
            a_mu, a_ls = A.eager_pair_allowance(info, eps_np)
            grow = 1.0 + max(float(np.max(a_mu / ref["d_mu"][1])), float(np.max(a_ls / ref["d_log_std"][1])))
            worst = 0.0
            pairs = [("actor_loss", la, la_e), ("ent_coef_loss", le, le_e)] + [(n, p.grad, q.grad) for n, p, q in zip(names, pf, pe)]
            for name, a, b in pairs:
                bound = ref[name][1] * (grow if name in A.GRADS else 1.0)
                d = np.abs(a.detach().cpu().numpy().astype(np.float64) - b.detach().cpu().numpy().astype(np.float64)).reshape(bound.shape)
                assert (d <= 2.0 * bound).all(), (B, name)
                worst = max(worst, float((d / np.maximum(bound, 1e-300)).max()))
        t_f, t_e = timed(torch, fused, reps), timed(torch, eager, reps)
        row = dict(kind="sac", batch=B, fused_ms=t_f, eager_ms=t_e, eager_over_fused=t_e / t_f, gated=B in GATED,
                   gate_fused_not_above_eager=(t_f <= t_e) if B in GATED else None, max_fused_minus_eager_over_bound=worst,
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
    summary = dict(summary="bench_actor_grad", **state(), gate_holds_at_100_256_4096=ok, rows=rows)
    print(json.dumps(summary), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(summary, f, indent=1)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
