"""The fused optimiser step (FusedOptimStep.critic_step + actor_step(polyak=True): two k_optim_step launches) against the
stock statements of SB3's SAC.train / TD3.train it replaces, on twin modules in the same run:

    critic.optimizer.step();  actor.optimizer.step();  ent_coef_optimizer.step()            (SAC; TD3 has no third)
    polyak_update(critic.parameters(), critic_target.parameters(), tau)                    (TD3: the actor's too)

    python tools/bench_optim_step.py [--reps 50] [--out FILE]

For the SAC recipe (actor and twin critics ReLU [128, 128, 128], log_ent_coef) and the TD3 recipe ([256, 256]): the median
milliseconds of `reps` CUDA-event pairs after a warm-up call, host overhead included on every side, of
  (a) fused     critic_step() + actor_step(polyak=True)
  (b) stock     the optimizer.step() calls with torch's defaults and SB3's polyak_update loop (mul_ then add with alpha)
  (c) strongest torch.optim.Adam(fused=True) and a _foreach Polyak (for information only)
The gradients are fixed random tensors (views into one flat buffer per network for (a), as FusedCriticGrad / FusedActorGrad
hand them out).  Before anything is timed, one step of (a) and (b) from identical state is asserted to agree within twice the
bound of tests/optim_step_ref.py on every parameter, target and Adam state tensor.  One JSON line per recipe.  The gate: (a)
is not above (b) for both recipes; the exit status is 1 if it fails.  Then a summary line with the library's source hash
(tools/source_state.py).  Kernel durations come from a rocprofv3 --kernel-trace --stats run of this script."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

TAU, LR = 0.005, 3e-4


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


def networks(torch, kind):
    """dict(actor=[params], critic=[params], ent=[param] or []) on the GPU, torch's default init."""
    import td_target_ref as T
    m = T.sac_modules() if kind == "sac" else T.td3_modules()
    par = lambda ls: [torch.nn.Parameter(t.detach().clone().cuda()) for l in ls for t in (l.weight, l.bias)]   # noqa: E731
    actor = par(m["lin"] + [m["mu"]] + ([m["ls"]] if kind == "sac" else []))
    critic = par(m["q1"]) + par(m["q2"])
    ent = [torch.nn.Parameter(torch.full((1,), -0.5, device="cuda"))] if kind == "sac" else []
    return dict(actor=actor, critic=critic, ent=ent)


def side(torch, kind, flat, **adam_kw):
    """One side of the comparison: parameters, targets, optimisers and fixed gradients from fixed seeds."""
    import optim_step_ref as O
    n = networks(torch, kind)
    n["critic_target"] = [p.detach().clone().mul_(0.75) for p in n["critic"]]
    n["actor_target"] = [p.detach().clone().mul_(0.75) for p in n["actor"]] if kind == "td3" else []
    gen = torch.Generator(device="cuda").manual_seed(7)
    for ps in (n["critic"], n["actor"] + n["ent"]):        # one flat buffer per backward call: the critics'; the actor's and log_ent_coef's
        if flat:
            O.flat_grads(torch, ps, "cuda", lead=0)
        for p in ps:
            g = 1e-2 * torch.randn(p.shape, device="cuda", generator=gen)
            if flat:
                p.grad.copy_(g)
            else:
                p.grad = g
    n["opts"] = [torch.optim.Adam(n[g], lr=LR, **adam_kw) for g in ("critic", "actor", "ent") if n[g]]
    return n


def measure(reps):
    import torch

    import optim_step_ref as O
    from reinforcementlearning4meshgeneration_amd.optim_step import FusedOptimStep
    rows = []
    for kind in ("sac", "td3"):
        f, s, c = side(torch, kind, True), side(torch, kind, False), side(torch, kind, False, fused=True)
        if kind == "sac":
            fo = FusedOptimStep.sac(*f["opts"], f["critic"], f["critic_target"], tau=TAU)
        else:
            fo = FusedOptimStep.td3(*f["opts"], f["critic"], f["critic_target"], f["actor"], f["actor_target"], tau=TAU)
        pairs = lambda n: list(zip(n["critic"] + (n["actor"] if kind == "td3" else []), n["critic_target"] + n["actor_target"]))   # noqa: E731

        def fused():
            fo.critic_step()
            fo.actor_step(polyak=True)

        def stock():
            for o in s["opts"]:
                o.step()
            with torch.no_grad():                          # stable_baselines3.common.utils.polyak_update
                for p, t in pairs(s):
                    t.data.mul_(1 - TAU)
                    torch.add(t.data, p.data, alpha=TAU, out=t.data)

        def strongest():
            for o in c["opts"]:
                o.step()
            with torch.no_grad():
                src, dst = [p.data for p, _ in pairs(c)], [t.data for _, t in pairs(c)]
                torch._foreach_mul_(dst, 1 - TAU)
                torch._foreach_add_(dst, src, alpha=TAU)

        # ---- agreement first: one step of each from identical state
        host = lambda x: x.detach().cpu().numpy().copy()   # noqa: E731
        before = {g: [(host(p), np.zeros(p.shape, np.float32), np.zeros(p.shape, np.float32), host(p.grad)) for p in f[g]]
                  for g in ("critic", "actor", "ent")}
        t_before = [host(t) for _, t in pairs(f)]
        fused()
        stock()
        sc, worst = O.scalars(1, lr=LR), 0.0
        names = [g for g in ("critic", "actor", "ent") if f[g]]
        for g, of, os_ in zip(names, f["opts"], s["opts"]):
            for p, q, b in zip(f[g], s[g], before[g]):
                ref = O.adam(*b, sc)
                for k, x, y in (("p", p, q), ("exp_avg", of.state[p]["exp_avg"], os_.state[q]["exp_avg"]),
                                ("exp_avg_sq", of.state[p]["exp_avg_sq"], os_.state[q]["exp_avg_sq"])):
                    d = np.abs(host(x).astype(np.float64) - host(y))
                    assert (d <= 2.0 * ref[k][1]).all(), (kind, g, k)
                    worst = max(worst, float((d / ref[k][1]).max()))
        for (p, t), (_, tt), t0 in zip(pairs(f), pairs(s), t_before):
            ref = O.polyak(t0, host(p), TAU)
            d = np.abs(host(t).astype(np.float64) - host(tt))
            assert (d <= 2.0 * ref[1]).all(), (kind, "target")
            worst = max(worst, float((d / ref[1]).max()))
        binds = fo.binds
        t_a, t_b, t_c = timed(torch, fused, reps), timed(torch, stock, reps), timed(torch, strongest, reps)
        assert fo.binds == binds, "the steady state uploaded a table"
        row = dict(kind=kind, tensors=sum(len(f[g]) for g in names), elements=sum(p.numel() for g in names for p in f[g]),
                   fused_ms=t_a, stock_ms=t_b, strongest_torch_ms=t_c, stock_over_fused=t_b / t_a, strongest_over_fused=t_c / t_a,
                   gate_fused_not_above_stock=t_a <= t_b, max_fused_minus_stock_over_bound=worst)
        print(json.dumps(row), flush=True)
        rows.append(row)
        fo.close()
    return rows


def fused_only(n):
    """N x (critic_step, actor_step(polyak=True)) per recipe between two synchronisations: in a kernel trace the steady state
    is 2 N consecutive k_optim_step launches per recipe with nothing in between."""
    import torch
    from reinforcementlearning4meshgeneration_amd.optim_step import FusedOptimStep
    for kind in ("sac", "td3"):
        f = side(torch, kind, True)
        if kind == "sac":
            fo = FusedOptimStep.sac(*f["opts"], f["critic"], f["critic_target"], tau=TAU)
        else:
            fo = FusedOptimStep.td3(*f["opts"], f["critic"], f["critic_target"], f["actor"], f["actor_target"], tau=TAU)
        torch.cuda.synchronize()
        for _ in range(n):
            fo.critic_step()
            fo.actor_step(polyak=True)
        torch.cuda.synchronize()
        print(json.dumps(dict(kind=kind, fused_steps=n, launches=2 * n, uploads=fo.binds)), flush=True)
        fo.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    ap.add_argument("--fused-only", type=int, default=0, metavar="N",
                    help="no timing: N fused gradient steps per recipe and nothing else (the run a kernel trace is taken from)")
    args = ap.parse_args()
    if args.fused_only:
        return fused_only(args.fused_only)
    from source_state import state
    rows = measure(args.reps)
    ok = all(r["gate_fused_not_above_stock"] for r in rows)
    summary = dict(summary="bench_optim_step", **state(), gate_holds_for_sac_and_td3=ok, rows=rows)
    print(json.dumps(summary), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(summary, f, indent=1)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
